// fenrir_grid_jvp / fenrir_grid_grad / fenrir_grad (an addition): the forward half of the directional
// derivatives of fenrir_grid's log p(Y | Z) with respect to the ODE parameters and the initial state, forward mode, one tangent
// direction per lane.  RTC-safe: no host code.  The backward half has no right-hand side and is ahead-of-time code only
// (fenrir_grad.hip: fenrir_grid_jvp_bwd_kernel).
//
// The primal filter is grid_fwd_kernel's data-free one (grid_kernels.hpp), grid_step's own calls in its order -- predict_block,
// interrogate_traj, update_block_m1 -- inside grid_walk (dalton_grid_kernels.hpp).  Next to (mu, Sigma) a lane carries
// (mu., Sigma.) by dalton_grad_kernels.hpp's pieces, called, not copied: jvp_predict_block, jvp_interrogate, jvp_update.  The
// log-density derivative that jvp_update accumulates is discarded: Fenrir's forward pass has no density.  jvp_update
// differentiates K = SW / s, a division; the primal step multiplies by fast_rcp(s).  That difference is rounding (fast_rcp is
// good to about an ulp), not another formula: the tangent is the derivative of the quotient either way.
//
// What leaves the kernel: the tangent record (mu._f, Sigma._f) of every node 0 .. N of every item, item-minor -- dmean (N+1, D, P,
// B K), dvar (N+1, D, P, P, B K), the batch-minor layout of lane_filter.hpp with B K items in place of B trajectories, so that
// consecutive lanes hit consecutive addresses -- and, from the k = 0 item of each trajectory, the primal filtered record in the
// plan's batch-minor mean / var, by grid_fwd_kernel's store_moments calls.  Node 0: mu._f = the ode_init direction, Sigma._f = 0.
// One writer per element, plain vector stores, no atomics.
#pragma once
#include "rk_enums.hpp"
#include "kalman_small.hpp"
#include "philox.hpp"
#include "solve_args.hpp"
#include "solve_small_kernels.hpp"
#include "grid_kernels.hpp"
#include "dalton_kernels.hpp"
#include "dalton_grid_kernels.hpp"
#include "dual.hpp"
#include "tangent.hpp"
#include "dalton_grad_kernels.hpp"

namespace rk {

// Work item = (trajectory b, direction k), item = b K + k as in dalton_grid_jvp_kernel; a wave holds 64 items (there are no joint
// and marginal halves here).  A lane recomputes its trajectory's primal filter and carries one tangent.  A lane past B K runs on
// the last item only where grid_walk needs the whole wave (grid_walk_needs_helpers), and stores nothing.
template <class RHS, int P, int ITG>
__global__ void __launch_bounds__(64) fenrir_grid_jvp_fwd_kernel(SolveArgs a, GridArgs g, JvpDirs dir, double* __restrict__ dmean,
                                                                 double* __restrict__ dvar) {
    constexpr int D = RHS::D, NT = RHS::NTHETA;
    const long long n_items = (long long)a.B * dir.K;
    const long long lane_item = (long long)blockIdx.x * 64 + threadIdx.x;
    const bool live = lane_item < n_items;
    if (!(live || grid_walk_needs_helpers<RHS, P>(g))) return;
    const long long item_ll = live ? lane_item : n_items - 1;               // (a lane past B K reads an item that exists)
    const int item = (int)item_ll, b = (int)(item_ll / dir.K), k = (int)(item_ll % dir.K);
    const bool first = live && k == 0;                                      // the item that stores its trajectory's primal record
    const size_t BK = (size_t)n_items;
    double W[D][P], th[NT], dth[NT], mu[D][P], S[D][P][P], dmu[D][P], dS[D][P][P];
    {
        double Q0[D][P][P], R0[D][P][P];
        lane_load_model<RHS, P>(a, b, Q0, R0, W, th);                       // W and theta: the plan's own pair is not read
    }
    lane_load_init<D, P>(a, b, mu, S);
#pragma unroll
    for (int j = 0; j < NT; ++j) dth[j] = dir.dtheta ? ld(dir.dtheta, (size_t)k * NT + j, dir.dtheta_b, a.B, b) : 0.0;
#pragma unroll
    for (int blk = 0; blk < D; ++blk)
#pragma unroll
        for (int r = 0; r < P; ++r) {
            dmu[blk][r] = dir.dinit ? ld(dir.dinit, ((size_t)k * D + blk) * P + r, dir.dinit_b, a.B, b) : 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c) dS[blk][r][c] = 0.0;
        }
    if (live) store_moments_all<D, P>(dmean, dvar, BK, 0, item, dmu, dS);                      // time index 0
    if (first) store_moments_all<D, P>(a.mean, a.var, (size_t)a.B, 0, b, mu, S);

    const uint32_t traj = (uint32_t)(a.traj_offset + (uint64_t)b);
    // (always_inline: the walk calls the step from more than one loop, and an outlined step would keep the state in scratch)
    grid_walk<RHS, P>(a, g, b, live, [&](const double (&Q)[D][P][P], const double (&R)[D][P][P], double t, int n)
                                         __attribute__((always_inline)) {
        double mup[D][P], Sp[D][P][P], dmup[D][P], dSp[D][P][P];
#pragma unroll
        for (int blk = 0; blk < D; ++blk) {
            predict_block<P>(Q[blk], R[blk], mu[blk], S[blk], mup[blk], Sp[blk]);
            jvp_predict_block<P>(Q[blk], dmu[blk], dS[blk], dmup[blk], dSp[blk]);
        }
        double wgt[D][P], am[D], V[D], dwgt[D][P], dam[D], dV[D];
        interrogate_traj<RHS, P, ITG>(W, th, t, mup, Sp, a.seed, traj, (uint32_t)n, wgt, am, V);
        jvp_interrogate<RHS, P, ITG>(W, th, dth, t, mup, dmup, dSp, wgt, dwgt, dam, dV);
#pragma unroll
        for (int blk = 0; blk < D; ++blk) {
            double Wm[P], unused = 0.0;
#pragma unroll
            for (int j = 0; j < P; ++j) Wm[j] = W[blk][j] + wgt[blk][j];                      // solve.py:79
            jvp_update<P, ITG == RK_INTERROGATE_KRAMER>(Wm, dwgt[blk], am[blk], dam[blk], V[blk], dV[blk], mup[blk], Sp[blk],
                                                        dmup[blk], dSp[blk], dmu[blk], dS[blk], unused);
            update_block_m1<P>(Wm, am[blk], V[blk], mup[blk], Sp[blk], mu[blk], S[blk]);
            if (live) store_moments<P>(dmean, dvar, BK, D, n + 1, blk, item, dmu[blk], dS[blk]);
            if (first) store_moments<P>(a.mean, a.var, (size_t)a.B, D, n + 1, blk, b, mu[blk], S[blk]);
        }
    });
}

// The hyper form, a sibling of the kernel above on the same device functions, written out: as one
// `__device__ __forceinline__` body under `if constexpr (HYPER)` behind two one-line kernels the pair kept its registers and fp64
// instruction counts and ran 1.1 % (this kernel) and 2.3 % (the hyper one) slower than the parent's, whose three block medians
// lie within 0.05 % (profiles/grad_shared_times.txt).  The item's rates l.[D]
// of log sigma stay in registers, and Sigma.- = Q Sigma. Q^T + 2 l. R (jvp_predict_scale).  The forward pass has no observation:
// the rates of the observation variances are the backward kernel's alone, and hy.dlobs is not read here.
template <class RHS, int P, int ITG>
__global__ void __launch_bounds__(64) fenrir_grid_jvp_fwd_hyper_kernel(SolveArgs a, GridArgs g, JvpDirs dir, JvpHyper hy,
                                                                       double* __restrict__ dmean, double* __restrict__ dvar) {
    constexpr int D = RHS::D, NT = RHS::NTHETA;
    const long long n_items = (long long)a.B * dir.K;
    const long long lane_item = (long long)blockIdx.x * 64 + threadIdx.x;
    const bool live = lane_item < n_items;
    if (!(live || grid_walk_needs_helpers<RHS, P>(g))) return;
    const long long item_ll = live ? lane_item : n_items - 1;               // (a lane past B K reads an item that exists)
    const int item = (int)item_ll, b = (int)(item_ll / dir.K), k = (int)(item_ll % dir.K);
    const bool first = live && k == 0;                                      // the item that stores its trajectory's primal record
    const size_t BK = (size_t)n_items;
    double W[D][P], th[NT], dth[NT], mu[D][P], S[D][P][P], dmu[D][P], dS[D][P][P], dls[D];
    {
        double Q0[D][P][P], R0[D][P][P];
        lane_load_model<RHS, P>(a, b, Q0, R0, W, th);                       // W and theta: the plan's own pair is not read
    }
    lane_load_init<D, P>(a, b, mu, S);
#pragma unroll
    for (int j = 0; j < NT; ++j) dth[j] = dir.dtheta ? ld(dir.dtheta, (size_t)k * NT + j, dir.dtheta_b, a.B, b) : 0.0;
#pragma unroll
    for (int blk = 0; blk < D; ++blk) {
        dls[blk] = hyper_rate(hy.dlsig, hy.dlsig_b, D, k, blk, a.B, b);
#pragma unroll
        for (int r = 0; r < P; ++r) {
            dmu[blk][r] = dir.dinit ? ld(dir.dinit, ((size_t)k * D + blk) * P + r, dir.dinit_b, a.B, b) : 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c) dS[blk][r][c] = 0.0;
        }
    }
    if (live) store_moments_all<D, P>(dmean, dvar, BK, 0, item, dmu, dS);                      // time index 0
    if (first) store_moments_all<D, P>(a.mean, a.var, (size_t)a.B, 0, b, mu, S);

    const uint32_t traj = (uint32_t)(a.traj_offset + (uint64_t)b);
    // (always_inline: the walk calls the step from more than one loop, and an outlined step would keep the state in scratch)
    grid_walk<RHS, P>(a, g, b, live, [&](const double (&Q)[D][P][P], const double (&R)[D][P][P], double t, int n)
                                         __attribute__((always_inline)) {
        double mup[D][P], Sp[D][P][P], dmup[D][P], dSp[D][P][P];
#pragma unroll
        for (int blk = 0; blk < D; ++blk) {
            predict_block<P>(Q[blk], R[blk], mu[blk], S[blk], mup[blk], Sp[blk]);
            jvp_predict_block<P>(Q[blk], dmu[blk], dS[blk], dmup[blk], dSp[blk]);
            jvp_predict_scale<P>(R[blk], dls[blk], dSp[blk]);
        }
        double wgt[D][P], am[D], V[D], dwgt[D][P], dam[D], dV[D];
        interrogate_traj<RHS, P, ITG>(W, th, t, mup, Sp, a.seed, traj, (uint32_t)n, wgt, am, V);
        jvp_interrogate<RHS, P, ITG>(W, th, dth, t, mup, dmup, dSp, wgt, dwgt, dam, dV);
#pragma unroll
        for (int blk = 0; blk < D; ++blk) {
            double Wm[P], unused = 0.0;
#pragma unroll
            for (int j = 0; j < P; ++j) Wm[j] = W[blk][j] + wgt[blk][j];                      // solve.py:79
            jvp_update<P, ITG == RK_INTERROGATE_KRAMER>(Wm, dwgt[blk], am[blk], dam[blk], V[blk], dV[blk], mup[blk], Sp[blk],
                                                        dmup[blk], dSp[blk], dmu[blk], dS[blk], unused);
            update_block_m1<P>(Wm, am[blk], V[blk], mup[blk], Sp[blk], mu[blk], S[blk]);
            if (live) store_moments<P>(dmean, dvar, BK, D, n + 1, blk, item, dmu[blk], dS[blk]);
            if (first) store_moments<P>(a.mean, a.var, (size_t)a.B, D, n + 1, blk, b, mu[blk], S[blk]);
        }
    });
}

}  // namespace rk
