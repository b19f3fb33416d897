// solve_evidence_grid / solve_mv_dynamic_grid / solve_sim_dynamic_grid: the two calibration tools on the non-uniform grid of
// solve_mv_grid (an addition) -- the walk of a forward lane over the grid's per-step pairs, written
// once, and the two forward lane kernels built on it.  Shared by the ahead-of-time build (grid_calib.hip, built-in right-hand
// sides) and the hiprtc build for user-supplied right-hand sides (rhs_jit.hip, its grid-evidence and grid-dynamic kinds only).
// RTC-safe: no host code.
//
// Step n -> n + 1 takes (Q, R) = (q, r)[slot[n]] and interrogates at t[n+1] (grid_kernels.hpp).  The evidence step is
// evidence_kernel's and the dynamic step dynamic_fwd_kernel's, piece by piece and in their order, with that pair:
//   evidence:  predict_block, interrogate_traj, evidence_update_z;  quad_b += z^2 / s, logdet_b += log s (LogProd)
//   dynamic:   dynamic_propagate (mu- = Q mu, P = Q Sigma Q^T), interrogate_traj, c = max(z^2 / (W~ R W~^T), scale_min),
//              dynamic_add_noise (Sigma- = P + c R), rodeo's var_meas from this Sigma-, evidence_update_z, the sums, scale[n, b]
//              = c and the moments of node n + 1
// Outputs as evidence_kernel's (logdens (B); quad, logdet (n_block, B)) and dynamic_fwd_kernel's (scale (N, n_block, B); logdens).
#pragma once
#include "rk_enums.hpp"
#include "kalman_small.hpp"
#include "philox.hpp"
#include "solve_args.hpp"
#include "solve_small_kernels.hpp"
#include "evidence_kernels.hpp"
#include "dynamic_kernels.hpp"
#include "grid_kernels.hpp"

namespace rk {

// What a step hands back to the walk: per block, two values that its update produces last (an entry of the filtered variance,
// the running mantissa of logdet).  The walk makes the block that rotates the prefetched pair in -- and looks at the fetched
// slot -- depend on them.  A step that stores nothing (the evidence's) has no side effect, so without this the compiler merges
// that block into the one that issues the prefetch, IN FRONT of the step: every step then waits, vmcnt(0), for the loads it
// has just issued, looks at the slot right behind its load, and holds a third copy of the pair while it computes (at
// FitzHugh-Nagumo p = 4: 512 registers and 68 / 12 B of scratch under rodeo / kramer against 496 / 480 and none; DESIGN.md
// section 7 (18)).  Reading a value changes no arithmetic.
template <int D>
struct GridStepDone { double s[D], m[D]; };
template <int D>
__device__ __forceinline__ void grid_walk_behind(int& s_after, const GridStepDone<D>& done) {
#pragma unroll
    for (int blk = 0; blk < D; ++blk) asm volatile("" : : "v"(done.s[blk]), "v"(done.m[blk]));
    // (the fetched slot stays in a vector register until here, as in grid_fwd_kernel; volatile statements keep their order)
    asm volatile("" : "+v"(s_after));
}

// The walk of one forward lane over the steps of the grid: step(Q, R, t, n, live) -> GridStepDone<D> for n = 0 .. N-1 with the
// pair of step n (const double (&)[D][P][P], in registers or in LDS), the time t[n+1] and `live`, false for a lane past B that
// only helps to stage the pairs and must write nothing.  Where the pair lives follows grid_fwd_kernel's three regimes
// (grid_kernels.hpp):
//   (a) D P^2 <= 32: two register sets, the pair of step n + 1 fetched while step n computes and rotated in behind it;
//   (b) beyond, a shared pair: two LDS buffers staged one step ahead by the whole wave, one __syncthreads() per step;
//   (c) beyond, a pair with a batch axis: one LDS row of 2 D P^2 + 1 doubles per lane, filled at the top of the step.
// No step waits for a load that depends on another load: the time of step n + 1 is fetched one step ahead like its pair, the
// slot two, and a fetched slot is first looked at (clamped) one step after its load was issued.  The caller has returned for
// a lane past B in regime (a); in (c) the walk returns for it before the first step.  One wave per workgroup.
template <class RHS, int P, class Step>
__device__ __forceinline__ void grid_walk(const SolveArgs& a, const GridArgs& g, int b, bool live, Step&& step) {
    constexpr int D = RHS::D, E = D * P * P;
    double t = g.t[1];
    int s_next = a.N >= 2 ? g.slot[1] : 0;                   // slot of step n + 1 as the table has it: clamped where it is used
    if constexpr (grid_two_sets<RHS, P>()) {
        double Q[D][P][P], R[D][P][P];
#pragma unroll
        for (int blk = 0; blk < D; ++blk) grid_load_pair<P>(g, a.B, D, grid_slot(g, 0), blk, b, Q[blk], R[blk]);
        // the loads above are complete before the loop is entered (vmcnt(0); expcnt and lgkmcnt left alone): else the wait for
        // them lands in the loop body behind the prefetch just issued, where only vmcnt(0) covers them (grid_kernels.hpp)
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
            const GridStepDone<D> done = step(Q, R, t, n, true);
            if (more) {
                t = tn;
                grid_walk_behind<D>(s_after, done);
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
                (void)step(*reinterpret_cast<Mats*>(mine), *reinterpret_cast<Mats*>(mine + E), t, n, true);
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
                const GridStepDone<D> done = step(*reinterpret_cast<Mats*>(cur), *reinterpret_cast<Mats*>(cur + E), t, n, live);
                if (more) {
                    t = tn;
                    grid_walk_behind<D>(s_after, done);
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

// the lane of a forward kernel on the walk: false for a lane that has nothing to do (past B with the pairs in registers);
// a lane past B that stays reads a trajectory that exists
template <class RHS, int P>
__device__ __forceinline__ bool grid_walk_lane(const SolveArgs& a, int& b, bool& live) {
    const int lane_b = blockIdx.x * blockDim.x + threadIdx.x;
    live = lane_b < a.B;
    if (grid_two_sets<RHS, P>() && !live) return false;
    b = live ? lane_b : a.B - 1;
    return true;
}

// the evidence on the grid, one lane per trajectory: evidence_kernel's step and sums, nothing stored per step
template <class RHS, int P, int ITG>
__global__ void __launch_bounds__(64) grid_evidence_kernel(SolveArgs a, GridArgs g, double* __restrict__ logdens,
                                                           double* __restrict__ quad, double* __restrict__ logdet) {
    constexpr int D = RHS::D;
    static_assert(ITG != RK_INTERROGATE_CHKREBTII, "evidence_grid: interrogate_chkrebtii is not served (no scale law)");
    int b;
    bool live;
    if (!grid_walk_lane<RHS, P>(a, b, live)) return;
    const size_t B = (size_t)a.B;
    double W[D][P], th[RHS::NTHETA], mu[D][P], S[D][P][P], q[D] = {};
    LogProd l[D];
    {
        double Q0[D][P][P], R0[D][P][P];
        lane_load_model<RHS, P>(a, b, Q0, R0, W, th);                                        // W and theta: the plan's own pair is not read
    }
    lane_load_init<D, P>(a, b, mu, S);
    const uint32_t traj = (uint32_t)(a.traj_offset + (uint64_t)b);
    grid_walk<RHS, P>(a, g, b, live, [&](const double (&Q)[D][P][P], const double (&R)[D][P][P], double t, int n, bool) {
        double mup[D][P], Sp[D][P][P];
#pragma unroll
        for (int blk = 0; blk < D; ++blk) predict_block<P>(Q[blk], R[blk], mu[blk], S[blk], mup[blk], Sp[blk]);
        double wgt[D][P], am[D], V[D];
        interrogate_traj<RHS, P, ITG>(W, th, t, mup, Sp, a.seed, traj, (uint32_t)n, wgt, am, V);
#pragma unroll
        for (int blk = 0; blk < D; ++blk) {
            double Wm[P], z, s, rs;
#pragma unroll
            for (int j = 0; j < P; ++j) Wm[j] = W[blk][j] + wgt[blk][j];
            evidence_update_z<P>(Wm, am[blk], V[blk], mup[blk], Sp[blk], mu[blk], S[blk], z, s, rs);
            q[blk] = fma(z * z, rs, q[blk]);
            l[blk].mul(s);
        }
        GridStepDone<D> done;
#pragma unroll
        for (int blk = 0; blk < D; ++blk) done.s[blk] = S[blk][P - 1][P - 1], done.m[blk] = l[blk].m;
        return done;
    });
    if (!live) return;
    double tot = 0.0;
#pragma unroll
    for (int blk = 0; blk < D; ++blk) {
        const double lb = l[blk].log();
        quad[(size_t)blk * B + b] = q[blk];
        logdet[(size_t)blk * B + b] = lb;
        tot += q[blk] + lb;
    }
    logdens[b] = evidence_logdens(tot, D, a.N);
}

// the dynamic solver's forward pass on the grid, one lane per trajectory: dynamic_fwd_kernel's step, stores and sums
template <class RHS, int P, int ITG>
__global__ void __launch_bounds__(64) grid_dynamic_fwd_kernel(SolveArgs a, GridArgs g, double scale_min,
                                                              double* __restrict__ scale, double* __restrict__ logdens) {
    constexpr int D = RHS::D;
    static_assert(ITG != RK_INTERROGATE_CHKREBTII, "dynamic_grid: interrogate_chkrebtii is not served (its point is drawn from "
                                                   "the predicted variance, which here depends on the point)");
    int b;
    bool live;
    if (!grid_walk_lane<RHS, P>(a, b, live)) return;
    const size_t B = (size_t)a.B;
    double W[D][P], th[RHS::NTHETA], mu[D][P], S[D][P][P], q[D] = {};
    LogProd l[D];
    {
        double Q0[D][P][P], R0[D][P][P];
        lane_load_model<RHS, P>(a, b, Q0, R0, W, th);
    }
    lane_load_init<D, P>(a, b, mu, S);
    if (live) store_moments_all<D, P>(a.mean, a.var, B, 0, b, mu, S);                        // time index 0
    const uint32_t traj = (uint32_t)(a.traj_offset + (uint64_t)b);
    grid_walk<RHS, P>(a, g, b, live, [&](const double (&Q)[D][P][P], const double (&R)[D][P][P], double t, int n, bool on) {
        double mup[D][P], Sp[D][P][P];
#pragma unroll
        for (int blk = 0; blk < D; ++blk) dynamic_propagate<P>(Q[blk], mu[blk], S[blk], mup[blk], Sp[blk]);
        double wgt[D][P], am[D], V[D];
        // (Sp holds P here: of the three served interrogations only rodeo reads it, for a var_meas that is formed below instead)
        interrogate_traj<RHS, P, ITG>(W, th, t, mup, Sp, a.seed, traj, (uint32_t)n, wgt, am, V);
#pragma unroll
        for (int blk = 0; blk < D; ++blk) {
            double Wm[P], z, s, rs;
#pragma unroll
            for (int j = 0; j < P; ++j) Wm[j] = W[blk][j] + wgt[blk][j];                      // solve.py:79
            const double z0 = 0.0 - (dot<P>(Wm, mup[blk]) + am[blk]);
            double c = z0 * z0 / dynamic_quadform<P>(Wm, R[blk]);
            c = c < scale_min ? scale_min : c;                                                // (a NaN stays a NaN)
            dynamic_add_noise<P>(Sp[blk], c, R[blk], Sp[blk]);
            double Vb = 0.0;
            if constexpr (ITG == RK_INTERROGATE_RODEO) Vb = dynamic_quadform<P>(W[blk], Sp[blk]);   // interrogate.py:110-113
            evidence_update_z<P>(Wm, am[blk], Vb, mup[blk], Sp[blk], mu[blk], S[blk], z, s, rs);
            q[blk] = fma(z * z, rs, q[blk]);
            l[blk].mul(s);
            if (on) {
                *bm_item(scale, 1, B, D, n, blk, b) = c;
                store_moments<P>(a.mean, a.var, B, D, n + 1, blk, b, mu[blk], S[blk]);
            }
        }
        GridStepDone<D> done;
#pragma unroll
        for (int blk = 0; blk < D; ++blk) done.s[blk] = S[blk][P - 1][P - 1], done.m[blk] = l[blk].m;
        return done;
    });
    if (!live) return;
    double tot = 0.0;
#pragma unroll
    for (int blk = 0; blk < D; ++blk) tot += q[blk] + l[blk].log();
    logdens[b] = evidence_logdens(tot, D, a.N);
}

}  // namespace rk
