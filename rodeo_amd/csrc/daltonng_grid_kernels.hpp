// daltonng_grid / solve_mv_nn_grid (an addition): the forward filter of DALTON for non-Gaussian
// observations on a non-uniform grid shared by the batch, every observation on a node.  Always a hiprtc build (rhs_jit.hip, its
// daltonng_grid kinds): OBS is user code (rodeo_amd.trace).  RTC-safe: no host code.
//
// The step is daltonng_fwd_kernel's (daltonng_kernels.hpp), helper for helper in the same order -- predict_block,
// interrogate_traj, ng_pseudo_obs at the predicted mean, update_block_m1, ng_observe_block (z first, yhat second), the stores
// written out -- inside grid_walk (dalton_grid_kernels.hpp): step n -> n + 1 predicts with the pair (q, r)[slot[n]], which lives
// where grid_two_sets puts it, and interrogates at the table's time t[n+1], not at step_time(a, n).  The gain records of the two
// backward log-density passes re-evaluate the prediction from filt[n] with step n's own pair (daltonng_grid.hip), which is what
// this filter predicted; daltonng_chain_kernel and daltonng_obs_kernel read records and never the prior.
#pragma once
#include "rk_enums.hpp"
#include "kalman_small.hpp"
#include "philox.hpp"
#include "solve_args.hpp"
#include "solve_small_kernels.hpp"
#include "grid_kernels.hpp"
#include "dalton_grid_kernels.hpp"
#include "daltonng_kernels.hpp"

namespace rk {

// BOTH = true (rk_daltonng_grid_loglik): a wave holds 32 trajectories, lanes 0..31 run their joint filters and lanes 32..63 their
// filters on Z alone; the joint filter stores its filtered moments into a.mean / a.var, the other into zm / zv.
// BOTH = false (rk_daltonng_grid_solve): one joint lane per trajectory.  o.obs_ind holds the NODE of every observation, strictly
// increasing; a node past N never matches and an observation on node 0 does not enter the filter (it enters logy_x).  The node
// of the next observation is held in a register and fetched again only behind an observation (dalton_grid_fwd_kernel); the
// schedule (i, its node) advances in every lane alike, only the conditioning is the joint lanes'.  A lane without a trajectory
// walks only where the wave stages a shared pair together (grid_walk_needs_helpers) and stores nothing.
template <class RHS, class OBS, int P, int ITG, int MO, bool BOTH>
__global__ void __launch_bounds__(64) daltonng_grid_fwd_kernel(SolveArgs a, NgObs o, GridArgs g, double* __restrict__ zm,
                                                               double* __restrict__ zv) {
    constexpr int D = RHS::D;
    constexpr bool SPLIT = BOTH && !grid_two_sets<RHS, P>();
    static_assert(OBS::D == D && OBS::P == P && OBS::NTHETA == RHS::NTHETA && OBS::MO == MO,
                  "the observation model was traced for another configuration");
    const int lane = threadIdx.x;
    const bool joint = !BOTH || lane < 32;
    const int lane_b = BOTH ? blockIdx.x * 32 + (lane & 31) : blockIdx.x * 64 + lane;
    const bool live = lane_b < a.B;
    const int b = live ? lane_b : a.B - 1;                                  // (a lane past B reads a trajectory that exists)
    if (!(live || grid_walk_needs_helpers<RHS, P>(g))) return;
    const size_t B = (size_t)a.B;
    double W[D][P], th[RHS::NTHETA], mu[D][P], S[D][P][P];
    {
        double Q0[D][P][P], R0[D][P][P];
        lane_load_model<RHS, P>(a, b, Q0, R0, W, th);                       // W and theta: the plan's own pair is not read
    }
    lane_load_init<D, P>(a, b, mu, S);
    if (live) store_moments_all<D, P>(joint ? a.mean : zm, joint ? a.var : zv, B, 0, b, mu, S);     // time 0: (ode_init, 0)
    int i = (o.n_obs > 0 && o.obs_ind[0] == 0) ? 1 : 0;
    int obs_node = i < o.n_obs ? o.obs_ind[i] : -1;                         // node of observation i; -1: none left

    const uint32_t traj = (uint32_t)(a.traj_offset + (uint64_t)b);
    const size_t mstride = (size_t)D * P * B, vstride = (size_t)D * P * P * B;
    // (always_inline: the walk calls the step from more than one loop, and an outlined step would keep the state in scratch)
    grid_walk<RHS, P>(a, g, b, live, [&](const double (&Q)[D][P][P], const double (&R)[D][P][P], double t, int n)
                                         __attribute__((always_inline)) {
        double mup[D][P], Sp[D][P][P];
#pragma unroll
        for (int blk = 0; blk < D; ++blk) {
            predict_block<P>(Q[blk], R[blk], mu[blk], S[blk], mup[blk], Sp[blk]);
            // (a pair staged in LDS: the next block's reads stay behind this block's products -- hoisted above them they take a
            // hundred registers more at n_bstate = 5, and the store form of n_bstate = 6 then needs more scratch than
            // daltonng_fwd_kernel's)
            if constexpr (!grid_two_sets<RHS, P>()) asm volatile("" ::: "memory");
        }
        double wgt[D][P], am[D], V[D];
        interrogate_traj<RHS, P, ITG>(W, th, t, mup, Sp, a.seed, traj, (uint32_t)n, wgt, am, V);
        // (the same in every lane of the wave: the expansion is evaluated under a scalar branch, by the lanes of the filter on Z
        // alone too, which drop it)
        const bool at_node = obs_node == n + 1;
        double Dm[D][MO][P], yh[D][MO], Om[D][MO][MO];
        if (at_node) {
            double y[D][OBS::NY];
#pragma unroll
            for (int blk = 0; blk < D; ++blk)
#pragma unroll
                for (int k = 0; k < OBS::NY; ++k) y[blk][k] = o.y[((size_t)i * D + blk) * OBS::NY + k];
            ng_pseudo_obs<OBS, P, MO, 0>(y, mup, (double)i, th, Dm, yh, Om);
        }
#pragma unroll
        for (int blk = 0; blk < D; ++blk) {
            double Wm[P];
#pragma unroll
            for (int j = 0; j < P; ++j) Wm[j] = W[blk][j] + wgt[blk][j];
            update_block_m1<P>(Wm, am[blk], V[blk], mup[blk], Sp[blk], mu[blk], S[blk]);
            if (at_node && joint) ng_observe_block<OBS, P, MO, 0>(blk, Dm, yh, Om, mu[blk], S[blk]);
            if (live) {
                // store_moments, written out (daltonng_fwd_kernel).  SPLIT: each half of the wave stores from a branch of its own,
                // so that every store has a scalar base -- a per-lane base costs a 64-bit address per store in vector registers,
                // and with the pair staged in LDS the kernel then spills where daltonng_fwd_kernel does not.  With two register
                // sets nothing spills, and there the one sequence of stores keeps the count of stores in flight known, so that
                // the wait for the slot fetched a step ahead does not wait for them too.
                const auto store = [&](double* __restrict__ mean, double* __restrict__ var) __attribute__((always_inline)) {
                    double* mo = mean + (size_t)(n + 1) * mstride + b;
                    double* vo = var + (size_t)(n + 1) * vstride + b;
#pragma unroll
                    for (int r = 0; r < P; ++r) {
                        const size_t em = (size_t)blk * P + r;
                        mo[em * B] = mu[blk][r];
#pragma unroll
                        for (int c = 0; c < P; ++c) vo[(em * P + c) * B] = S[blk][r][c];
                    }
                };
                if constexpr (SPLIT) {
                    // (the two statements differ, so the branches are not merged back into one with per-lane bases)
                    if (joint) { store(a.mean, a.var); asm volatile("; stored: the joint filter's half"); }
                    else { store(zm, zv); asm volatile("; stored: the half of the filter on Z alone"); }
                } else {
                    store(joint ? a.mean : zm, joint ? a.var : zv);
                }
            }
        }
        if (at_node) {
            ++i;
            obs_node = i < o.n_obs ? o.obs_ind[i] : -1;
            asm volatile("" : "+v"(obs_node));                              // waited for here, on the rare path, not behind the next prefetch
        }
    });
}

}  // namespace rk
