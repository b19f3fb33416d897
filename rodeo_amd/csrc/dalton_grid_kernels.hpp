// dalton_grid / dalton.solve_mv_grid / dalton.solve_sim_grid (an addition): DALTON's forward filters on
// a non-uniform grid shared by the batch, every observation on a node.  Shared by the ahead-of-time build (dalton_grid.hip,
// built-in right-hand sides) and the hiprtc build for user-supplied right-hand sides (rhs_jit.hip, its dalton_grid kinds only).
// RTC-safe: no host code.
//
// The filter is grid_fwd_kernel's (grid_kernels.hpp) -- step n -> n + 1 predicts with the pair (q, r)[slot[n]] and interrogates
// at the table's time t[n+1] -- whose z update accumulates the forecast log-density (dalton_update_z) and which conditions on
// y_i at the node obs_ind[i] (dalton_observe), z first and y second, as dalton_fwd_kernel does on the uniform grid
// (dalton_kernels.hpp).  The marginal filter is the same recursion without observations.  The store form writes the batch-minor
// filtered moments that grid_bwd_mv_kernel / grid_bwd_sim_kernel (grid.hip) read: they re-evaluate the prediction from filt[n]
// with step n's own pair, which is what this filter predicted.
#pragma once
#include "rk_enums.hpp"
#include "kalman_small.hpp"
#include "philox.hpp"
#include "solve_args.hpp"
#include "solve_small_kernels.hpp"
#include "grid_kernels.hpp"
#include "dalton_kernels.hpp"

namespace rk {

// The time loop of a forward lane on the grid: step(Q, R, t, n) for n = 0 .. N - 1 with step n's pair and the time t[n+1].  The
// pair lives where grid_fwd_kernel keeps it, by the same rule grid_two_sets, and the three loops are that kernel's: two register
// sets with a one-step prefetch; beyond, a shared pair staged in LDS by the whole wave one step ahead; a pair with a batch axis in
// a row of LDS per lane, filled at the top of its step.  The time is fetched one step ahead, the slot two, and a fetched slot
// is first looked at one step after its load was issued.  `live`: false for a lane without a trajectory of its own; it takes
// part only where the wave stages a shared pair (its step then runs on trajectory b, which exists, and must store nothing).
// Returns without a barrier pending; the caller's cross-lane traffic stays outside.
// A SIBLING of grid_fwd_kernel's loops, not their replacement: with grid_fwd_kernel on this walk all 56 of its instances
// disassembled to another text than the parent build's, so that kernel keeps its own three loops.
template <class RHS, int P, class Step>
__device__ __forceinline__ void grid_walk(const SolveArgs& a, const GridArgs& g, int b, bool live, Step&& step) {
    constexpr int D = RHS::D, E = D * P * P;
    double t = g.t[1];
    int s_next = a.N >= 2 ? g.slot[1] : 0;                   // slot of step n + 1 as the table has it: clamped where it is used

    if constexpr (grid_two_sets<RHS, P>()) {
        if (!live) return;
        double Q[D][P][P], R[D][P][P];
#pragma unroll
        for (int blk = 0; blk < D; ++blk) grid_load_pair<P>(g, a.B, D, grid_slot(g, 0), blk, b, Q[blk], R[blk]);
        // every load so far is complete before the loop is entered, so that no step waits for its own prefetch (grid_fwd_kernel)
        __builtin_amdgcn_s_waitcnt(0x0F70);
        for (int n = 0; n < a.N; ++n) {
            const bool more = n + 1 < a.N;
            double Qn[D][P][P], Rn[D][P][P], tn = t;
            int s_after = 0;
            if (more) {
#pragma unroll
                for (int blk = 0; blk < D; ++blk) grid_load_pair<P>(g, a.B, D, grid_clamp(g, s_next), blk, b, Qn[blk], Rn[blk]);
                tn = g.t[n + 2];
                if (n + 2 < a.N) s_after = g.slot[n + 2];
            }
            step(Q, R, t, n);
            if (more) {
                t = tn;
                asm volatile("" : "+v"(s_after));            // the fetched slot stays in a vector register until here (grid_fwd_kernel)
                s_next = s_after;
#pragma unroll
                for (int blk = 0; blk < D; ++blk)
#pragma unroll
                    for (int i = 0; i < P; ++i)
#pragma unroll
                        for (int j = 0; j < P; ++j) {
                            Q[blk][i][j] = Qn[blk][i][j];
                            R[blk][i][j] = Rn[blk][i][j];
                        }
            }
        }
    } else {
        // LDS of the workgroup, which is one wave: a row of 2 E + 1 doubles per lane for pairs with a batch axis (the odd
        // length keeps the 64 rows off each other's banks), or two buffers of 2 E at its start for a shared pair
        __shared__ double lds[64 * (2 * E + 1)];
        using Mats = const double[D][P][P];
        if (g.q_b || g.r_b) {                            // (wave-uniform) every lane stages its own pair at the top of the step
            if (!live) return;
            double* mine = lds + threadIdx.x * (2 * E + 1);
            int s = g.slot[0];
            for (int n = 0; n < a.N; ++n) {
                const size_t at = (size_t)grid_clamp(g, s) * E;
                const double* qs = g.q + at * (g.q_b ? (size_t)a.B : 1);
                const double* rs = g.r + at * (g.r_b ? (size_t)a.B : 1);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    mine[e] = ld(qs, e, g.q_b, a.B, b);
                    mine[E + e] = ld(rs, e, g.r_b, a.B, b);
                }
                double tn = t;
                int s_after = 0;
                if (n + 1 < a.N) {
                    tn = g.t[n + 2];
                    if (n + 2 < a.N) s_after = g.slot[n + 2];
                }
                step(*reinterpret_cast<Mats*>(mine), *reinterpret_cast<Mats*>(mine + E), t, n);
                t = tn;
                s = s_next;
                s_next = s_after;
            }
        } else {                                         // a shared pair, staged by the whole wave one step ahead
            constexpr int KE = (2 * E + 63) / 64;
            // element e of a staged pair: Q (D, P, P) row-major for e < E, then R, as the slot lies in global memory
            const auto src = [&](int slot, int e) { return e < E ? g.q + (size_t)slot * E + e : g.r + (size_t)slot * E + (e - E); };
            {
                const int s0 = grid_slot(g, 0);
#pragma unroll
                for (int k = 0; k < KE; ++k) {
                    const int e = (int)threadIdx.x + 64 * k;
                    if (e < 2 * E) lds[e] = *src(s0, e);
                }
            }
            __syncthreads();
            for (int n = 0; n < a.N; ++n) {
                const bool more = n + 1 < a.N;
                const double* cur = lds + (n & 1) * 2 * E;
                double* nxt = lds + ((n & 1) ^ 1) * 2 * E;
                double pre[KE], tn = t;
                int s_after = 0;
                if (more) {
#pragma unroll
                    for (int k = 0; k < KE; ++k) {
                        const int e = (int)threadIdx.x + 64 * k;
                        pre[k] = e < 2 * E ? *src(grid_clamp(g, s_next), e) : 0.0;
                    }
                    tn = g.t[n + 2];
                    if (n + 2 < a.N) s_after = g.slot[n + 2];
                }
                step(*reinterpret_cast<Mats*>(cur), *reinterpret_cast<Mats*>(cur + E), t, n);
                if (more) {
                    t = tn;
                    asm volatile("" : "+v"(s_after));    // (as in the two-set loop above)
                    s_next = s_after;
#pragma unroll
                    for (int k = 0; k < KE; ++k) {
                        const int e = (int)threadIdx.x + 64 * k;
                        if (e < 2 * E) nxt[e] = pre[k];
                    }
                }
                __syncthreads();                         // the staged pair of step n + 1 is written, that of step n read
            }
        }
    }
}

// Does a lane without a trajectory still walk?  Only where the wave stages a shared pair in LDS together (wave-uniform).
template <class RHS, int P>
__device__ __forceinline__ bool grid_walk_needs_helpers(const GridArgs& g) {
    return !grid_two_sets<RHS, P>() && !(g.q_b || g.r_b);
}

// STORE = false (rk_dalton_grid_loglik): a wave holds 32 trajectories, lanes 0..31 run their joint filters and lanes 32..63
// their marginal filters; logdens[b] = joint - marginal leaves through store_joint_minus_marginal, outside every branch a lane
// without a trajectory skips.  STORE = true (rk_dalton_grid_solve): one lane per trajectory runs the joint filter and writes the
// batch-minor filtered moments.  obs_ind holds the NODE of every observation, strictly increasing; a node past N never matches.
// The node of the next observation is held in a register and fetched again only behind an observation, so the steps between
// two observations issue no load besides the walk's prefetches; the schedule (i, its node) advances in every lane alike, only
// the conditioning is the joint lanes'.
template <class RHS, int P, int ITG, int MO, bool STORE>
__global__ void __launch_bounds__(64) dalton_grid_fwd_kernel(SolveArgs a, DaltonObs o, GridArgs g, double* __restrict__ logdens) {
    constexpr int D = RHS::D;
    const int lane = threadIdx.x;
    const bool joint = STORE || lane < 32;
    const int lane_b = STORE ? blockIdx.x * 64 + lane : blockIdx.x * 32 + (lane & 31);
    const bool live = lane_b < a.B;
    const int b = live ? lane_b : a.B - 1;                                  // (a lane past B reads a trajectory that exists)
    double acc = 0.0;
    if (live || grid_walk_needs_helpers<RHS, P>(g)) {
        const size_t B = (size_t)a.B;
        double W[D][P], th[RHS::NTHETA], mu[D][P], S[D][P][P];
        {
            double Q0[D][P][P], R0[D][P][P];
            lane_load_model<RHS, P>(a, b, Q0, R0, W, th);                   // W and theta: the plan's own pair is not read
        }
        lane_load_init<D, P>(a, b, mu, S);
        if constexpr (STORE) {
            if (live) store_moments_all<D, P>(a.mean, a.var, B, 0, b, mu, S);   // time index 0: (ode_init, 0)
        }
        // an observation on node 0 adds log p(y_0 | x_0) to the joint density and does not update x_0 (dalton_fwd_kernel)
        int i = 0;
        if (o.n_obs > 0 && o.obs_ind[0] == 0) {
            if constexpr (!STORE) {
                if (joint) {
#pragma unroll
                    for (int blk = 0; blk < D; ++blk) {
                        double m0[P], S0[P][P];
#pragma unroll
                        for (int r = 0; r < P; ++r) {
                            m0[r] = mu[blk][r];
#pragma unroll
                            for (int c = 0; c < P; ++c) S0[r][c] = 0.0;
                        }
                        dalton_observe<P, MO>(o, (size_t)blk, m0, S0, acc);
                    }
                }
            }
            i = 1;
        }
        int obs_node = i < o.n_obs ? o.obs_ind[i] : -1;                     // node of observation i; -1: none left

        const uint32_t traj = (uint32_t)(a.traj_offset + (uint64_t)b);
        // (always_inline: the walk calls the step from more than one loop, and an outlined step would keep the state in scratch)
        grid_walk<RHS, P>(a, g, b, live, [&](const double (&Q)[D][P][P], const double (&R)[D][P][P], double t, int n)
                                             __attribute__((always_inline)) {
            double mup[D][P], Sp[D][P][P];
#pragma unroll
            for (int blk = 0; blk < D; ++blk) predict_block<P>(Q[blk], R[blk], mu[blk], S[blk], mup[blk], Sp[blk]);
            double wgt[D][P], am[D], V[D];
            interrogate_traj<RHS, P, ITG>(W, th, t, mup, Sp, a.seed, traj, (uint32_t)n, wgt, am, V);
            const bool obs_here = obs_node == n + 1;                        // (the same in every lane of the wave)
#pragma unroll
            for (int blk = 0; blk < D; ++blk) {
                double Wm[P];
#pragma unroll
                for (int j = 0; j < P; ++j) Wm[j] = W[blk][j] + wgt[blk][j];
                dalton_update_z<P>(Wm, am[blk], V[blk], mup[blk], Sp[blk], mu[blk], S[blk], acc);
                if (obs_here && joint) dalton_observe<P, MO>(o, (size_t)i * D + blk, mu[blk], S[blk], acc);
            }
            if (obs_here) {
                ++i;
                obs_node = i < o.n_obs ? o.obs_ind[i] : -1;
                asm volatile("" : "+v"(obs_node));                          // waited for here, on the rare path, not behind the next prefetch
            }
            if constexpr (STORE) {
                if (live) store_moments_all<D, P>(a.mean, a.var, B, n + 1, b, mu, S);
            }
        });
    }
    if constexpr (!STORE) store_joint_minus_marginal(acc, lane, lane_b, a.B, logdens);
}

}  // namespace rk
