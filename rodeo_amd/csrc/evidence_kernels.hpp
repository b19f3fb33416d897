// solve_evidence: the solver's own marginal likelihood log p(Z_{1:N} = 0) (an addition), the
// lane kernels of both Kalman forms.  Shared by the ahead-of-time build (evidence.hip, built-in right-hand sides) and the
// hiprtc build for user-supplied right-hand sides (rhs_jit.hip, its evidence kinds only).  RTC-safe: no host code.
//
// The filter is the solver's forward filter (fwd_kernel / fwd_sqrt_kernel) with nothing stored: per block it accumulates
//   quad_b = sum_n z_{n,b}^2 / s_{n,b}      and      logdet_b = sum_n log s_{n,b},
// z the innovation 0 - (W~ mu- + a) and s its forecast variance, and leaves
//   logdens = -1/2 sum_b (quad_b + logdet_b) - d N log(2 pi) / 2,      the blocks summed in block order.
// The density is the plain Gaussian one: NO threshold on s (utils.py:60-78 drops |s| <= 1e-8; an absolute threshold would
// break the scale law quad -> quad / c, logdet -> logdet + N log c under R -> c R).  A zero, negative or non-finite s gives
// inf or NaN as the arithmetic produces it.
// Outputs: logdens (B); quad, logdet (n_block, B) batch-minor, element [blk * B + b].
#pragma once
#include "rk_enums.hpp"
#include "kalman_small.hpp"
#include "philox.hpp"
#include "solve_args.hpp"
#include "solve_small_kernels.hpp"
#include "sqrt_small.hpp"
#include "solve_sqrt_kernels.hpp"

namespace rk {

// -1/2 (tot) - d N log(2 pi) / 2 with tot = sum_b (quad_b + logdet_b): the one expression of every route (and of
// rodeo_amd/evidence.py's evidence_at, which returns the same double at c = 1)
__device__ __forceinline__ double evidence_logdens(double tot, int D, int N) {
    const double HALF_LOG_2PI = 0.5 * 1.83787706640934548356;
    return -0.5 * tot - (double)(D * N) * HALF_LOG_2PI;
}

// logdet_b = sum_n log s_n as the log of a running product: per step the mantissa of s is multiplied onto a mantissa kept in
// [0.5, 1) and the exponents are added (nine instructions where log() has about eighty-five, on a chain that one wave per SIMD
// walks alone); one log after the loop.  As with log(): a negative s gives NaN, a zero -inf, an infinite one inf, NaN stays.
struct LogProd {
    double m = 1.0;
    int e = 0;
    __device__ __forceinline__ void mul(double s) {
        s = s < 0.0 ? __builtin_nan("") : s;
        const double p = m * __builtin_amdgcn_frexp_mant(s);
        e += __builtin_amdgcn_frexp_exp(s) + __builtin_amdgcn_frexp_exp(p);
        m = __builtin_amdgcn_frexp_mant(p);
    }
    __device__ __forceinline__ double log() const { return fma((double)e, 0.693147180559945309417, ::log(m)); }
};

// z forecast and update of one block (standard.py:93-102 for n_bmeas = 1, x_meas = 0) that hands back the innovation and
// its forecast variance s with the reciprocal rs = 1 / s (one division for the gain and the caller's z^2 / s): update_z with
// that reciprocal multiplied onto the gain
template <int P>
__device__ __forceinline__ void evidence_update_z(const double (&Wm)[P], double am, double V, const double (&mup)[P],
                                                  const double (&Sp)[P][P], double (&mu)[P], double (&S)[P][P],
                                                  double& innov, double& s, double& rs) {
    rs = update_z<P, GAIN_RCP>(Wm, am, V, mup, Sp, mu, S, innov, s);
}

// standard form, one lane per trajectory (dalton_fwd_kernel's layout without the second filter)
template <class RHS, int P, int ITG>
__global__ void __launch_bounds__(64) evidence_kernel(SolveArgs a, double* __restrict__ logdens, double* __restrict__ quad,
                                                      double* __restrict__ logdet) {
    constexpr int D = RHS::D;
    static_assert(ITG != RK_INTERROGATE_CHKREBTII, "evidence: interrogate_chkrebtii is not served (no scale law)");
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const size_t B = (size_t)a.B;
    double Q[D][P][P], R[D][P][P], W[D][P], th[RHS::NTHETA], mu[D][P], S[D][P][P], q[D];
    LogProd l[D];
    lane_load_model<RHS, P>(a, b, Q, R, W, th);
#pragma unroll
    for (int blk = 0; blk < D; ++blk) {                                     // lane_load_init, written out
        q[blk] = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            mu[blk][i] = ld(a.x0, (size_t)blk * P + i, a.x0_b, a.B, b);
#pragma unroll
            for (int j = 0; j < P; ++j) S[blk][i][j] = 0.0;
        }
    }
    const uint32_t traj = (uint32_t)(a.traj_offset + (uint64_t)b);
    for (int n = 0; n < a.N; ++n) {
        double mup[D][P], Sp[D][P][P];
#pragma unroll
        for (int blk = 0; blk < D; ++blk) predict_block<P>(Q[blk], R[blk], mu[blk], S[blk], mup[blk], Sp[blk]);
        double wgt[D][P], am[D], V[D];
        interrogate_traj<RHS, P, ITG>(W, th, step_time(a, n), mup, Sp, a.seed, traj, (uint32_t)n, wgt, am, V);
#pragma unroll
        for (int blk = 0; blk < D; ++blk) {
            double Wm[P], z, s, rs;
#pragma unroll
            for (int j = 0; j < P; ++j) Wm[j] = W[blk][j] + wgt[blk][j];
            evidence_update_z<P>(Wm, am[blk], V[blk], mup[blk], Sp[blk], mu[blk], S[blk], z, s, rs);
            q[blk] = fma(z * z, rs, q[blk]);
            l[blk].mul(s);
        }
    }
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

// innovation and forecast variance of the square-root z update (square_root.py:88-99 for n_bmeas = 1, x_meas = 0; vm the
// 1 x 1 "factor" of var_meas): s is the square of the scalar forecast factor |add_sqrt(W L-, vm)| that sqrt_update_m1
// forms -- the same expressions in the same order, which the compiler merges with sqrt_update_m1's when both are inlined
template <int P>
__device__ __forceinline__ void evidence_sqrt_forecast(const double (&W)[P], double a, double vm, const double (&mup)[P],
                                                       const double (&Lp)[P][P], double& innov, double& s) {
    innov = 0.0 - (dot<P>(W, mup) + a);
    double s2 = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) {                                     // row_mat, written out
        double t = W[0] * Lp[0][j];
#pragma unroll
        for (int i = 1; i < P; ++i) t = fma(W[i], Lp[i][j], t);
        s2 = fma(t, t, s2);
    }
    s2 = fma(vm, vm, s2);
    const double sfac = fast_sqrt_pos(s2);
    s = sfac * sfac;
}

// square-root form: fwd_sqrt_kernel's lane layout -- one lane per (trajectory, block), the D blocks of a trajectory in D
// neighbouring lanes, idle lanes repeat a real unit and store nothing -- with the factor standing where the reference puts
// it (interrogate_rodeo hands W L- W^T to the update as the "factor" of var_meas).  Every valid lane stores its block's sums;
// the trajectory's first lane reads its blocks' sums in block order (sq_from_lane) and stores logdens.
template <class RHS, int P, int ITG>
__global__ void __launch_bounds__(64) evidence_sqrt_kernel(SolveArgs a, double* __restrict__ logdens,
                                                           double* __restrict__ quad, double* __restrict__ logdet) {
    constexpr int D = RHS::D, TPW_ = 64 / D;
    static_assert(D >= 1 && D <= 64, "square-root filter: at most 64 blocks");
    static_assert(ITG != RK_INTERROGATE_CHKREBTII, "evidence: interrogate_chkrebtii is not served (no scale law)");
    constexpr bool HOIST = P <= 5;                        // Q and R^{1/2} of the lane's block stay in registers
    const int lane = threadIdx.x, tl = lane / D, blk = lane - tl * D, base = lane - blk;
    const int b_raw = blockIdx.x * TPW_ + tl;
    const bool valid = tl < TPW_ && b_raw < a.B;
    const int b = b_raw < a.B ? b_raw : a.B - 1;
    const size_t B = (size_t)a.B;
    double W[P], th[RHS::NTHETA], mu[P], L[P][P], Qh[HOIST ? P : 1][HOIST ? P : 1], LRh[HOIST ? P : 1][HOIST ? P : 1];
#pragma unroll
    for (int k = 0; k < RHS::NTHETA; ++k) th[k] = a.theta ? ld(a.theta, k, a.theta_b, a.B, b) : 0.0;
    if constexpr (HOIST) load_block_consts<P>(a, blk, b, Qh, LRh);
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const size_t em = (size_t)blk * P + i;
        W[i] = ld(a.W, em, a.W_b, a.B, b);
        mu[i] = ld(a.x0, em, a.x0_b, a.B, b);
#pragma unroll
        for (int j = 0; j < P; ++j) L[i][j] = 0.0;
    }
    double q = 0.0;
    LogProd lp;
    for (int n = 0; n < a.N; ++n) {
        double mup[P], Lp[P][P];
        if constexpr (HOIST) {
            sqrt_predict<P>(Qh, LRh, mu, L, mup, Lp);                                    // square_root.py:56-57
        } else {
            double Q[P][P], LR[P][P];
            load_block_consts<P>(a, blk, b, Q, LR);
            sqrt_predict<P>(Q, LR, mu, L, mup, Lp);
        }
        const double t = step_time(a, n);
        double X[D][P];                                   // the whole trajectory's points, in every one of its lanes
#pragma unroll
        for (int bb = 0; bb < D; ++bb)
#pragma unroll
            for (int j = 0; j < P; ++j) X[bb][j] = D == 1 ? mup[j] : sq_from_lane(mup[j], base + bb);
        double f[D], am, vm[1], Wm[P];
        if constexpr (ITG == RK_INTERROGATE_KRAMER) {
            double J[D][P], Jo[P];
            RHS::template fjac<P>(X, t, th, f, J);
#pragma unroll
            for (int j = 0; j < P; ++j) {
                double col[D];
#pragma unroll
                for (int bb = 0; bb < D; ++bb) col[bb] = J[bb][j];
                Jo[j] = sq_pick<D>(col, blk);
            }
            am = -sq_pick<D>(f, blk) + dot<P>(Jo, mup);
            vm[0] = 0.0;
#pragma unroll
            for (int j = 0; j < P; ++j) Wm[j] = W[j] - Jo[j];                           // solve.py:79
        } else {
            RHS::template f<P>(X, t, th, f);
            am = -sq_pick<D>(f, blk);
            vm[0] = 0.0;
            if constexpr (ITG == RK_INTERROGATE_RODEO) {                                // interrogate.py:110-113 on the factor
                double WL[P];
#pragma unroll
                for (int j = 0; j < P; ++j) {                         // row_mat, written out
                    double s = W[0] * Lp[0][j];
#pragma unroll
                    for (int i = 1; i < P; ++i) s = fma(W[i], Lp[i][j], s);
                    WL[j] = s;
                }
                vm[0] = dot<P>(WL, W);
            }
#pragma unroll
            for (int j = 0; j < P; ++j) Wm[j] = W[j];
        }
        double z, s;
        evidence_sqrt_forecast<P>(Wm, am, vm[0], mup, Lp, z, s);
        q += z * z / s;
        lp.mul(s);
        sqrt_update_m1<P, 1>(Wm, am, vm, mup, Lp, mu, L);
    }
    const double l = lp.log();
    if (valid) {
        quad[(size_t)blk * B + b] = q;
        logdet[(size_t)blk * B + b] = l;
    }
    const double mine = q + l;
    double tot = 0.0;
#pragma unroll
    for (int bb = 0; bb < D; ++bb) tot += D == 1 ? mine : sq_from_lane(mine, base + bb);
    if (valid && blk == 0) logdens[b] = evidence_logdens(tot, D, a.N);
}

}  // namespace rk
