// MAGI log-density (src/rodeo/inference/magi.py:6-99), one lane per (trajectory, block): the Kalman filter of the prior
// X_n = Q X_{n-1} + N(0, R) that measures the first NA of the P components exactly (W = eye(NA, P), mean_meas = 0,
// var_meas = 0), from the known x_0 (var 0).  Per step: predict, forecast, the forecast's Gaussian log-density at x_n[:NA]
// (jax.scipy.stats.multivariate_normal.logpdf: Cholesky, no eigenvalue cut-off), update.  Host side: magi.hip.
#pragma once
#include "kalman_small.hpp"
#include "solve_args.hpp"
#include "sqrt_small.hpp"

namespace rk {

struct MagiArgs {
    int B, N, D;
    const double *x0, *xm, *Q, *R;      // x0 (D, P [,B]), xm (N, D, NA [,B]), Q / R (D, P, P [,B]), batch-minor
    int x0_b, xm_b, Q_b, R_b;
};

// x_meas steps in flight per lane: an HBM miss (~900 cycles) spans several filter steps at small P.
template <int NA>
constexpr int magi_prefetch() { return NA <= 2 ? 8 : (NA <= 5 ? 4 : 2); }

constexpr double MAGI_LOG_2PI = 1.83787706640934548356;

// standard.py:57-59, 333-335, 93-102 with W = eye(NA, P), var_meas = 0, and the logpdf of the forecast at x: returns the
// log-density, (mu, S) <- the filtered moments.  The gain is the LU solve of solve_var (utils.py:119), as in the solver.
template <int P, int NA>
__device__ __forceinline__ double magi_step_std(const double (&Q)[P][P], const double (&R)[P][P], const double (&x)[NA],
                                                double (&mu)[P], double (&S)[P][P]) {
    double mup[P], Sp[P][P];
    predict_block<P>(Q, R, mu, S, mup, Sp);
    double e[NA];                                                       // x - mean_fore; var_fore = Sp[:NA, :NA]
#pragma unroll
    for (int j = 0; j < NA; ++j) e[j] = x[j] - mup[j];
    // Cholesky of var_fore (lower triangle) and z = L^{-1} e: logpdf = -|z|^2 / 2 - sum log L_jj - NA log(2 pi) / 2
    double L[NA][NA], z[NA], det = 1.0, zz = 0.0;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        double dj = Sp[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) dj = fma(-L[j][k], L[j][k], dj);
        const double ljj = sqrt(dj);                                    // (NaN for an indefinite forecast, like the reference)
        const double rl = 1.0 / ljj;
        L[j][j] = ljj;
#pragma unroll
        for (int i = j + 1; i < NA; ++i) {
            double s = Sp[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = fma(-L[i][k], L[j][k], s);
            L[i][j] = s * rl;
        }
        double zj = e[j];
#pragma unroll
        for (int k = 0; k < j; ++k) zj = fma(-L[j][k], z[k], zj);
        z[j] = zj * rl;
        zz = fma(z[j], z[j], zz);
        det *= ljj;
    }
    // K^T = var_fore^{-1} (Sp W^T)^T: X[j][r] = Sp[r][j]
    double Vf[NA][NA], X[NA][P];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
#pragma unroll
        for (int l = 0; l < NA; ++l) Vf[j][l] = Sp[j][l];
#pragma unroll
        for (int r = 0; r < P; ++r) X[j][r] = Sp[r][j];
    }
    lu_solve<NA, P>(Vf, X);
#pragma unroll
    for (int r = 0; r < P; ++r) {
        double t = X[0][r] * e[0];
#pragma unroll
        for (int j = 1; j < NA; ++j) t = fma(X[j][r], e[j], t);
        mu[r] = mup[r] + t;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            double u = X[0][r] * Sp[0][c];                              // K (W Sp) = K Sp[:NA, :]
#pragma unroll
            for (int j = 1; j < NA; ++j) u = fma(X[j][r], Sp[j][c], u);
            S[r][c] = Sp[r][c] - u;
        }
    }
    return -0.5 * zz - log(det) - 0.5 * NA * MAGI_LOG_2PI;       // (one log per step: sum log L_jj = log prod L_jj)
}

// square_root.py:56-57 (predict), 342-344 (forecast), 88-99 (update) with W = eye(NA, P), var_meas = 0; L and LR are lower
// factors.  The forecast factor F = add_sqrt(W Lp, 0) has F F^T = var_fore: up to the signs of its columns (the QR's) it is
// the Cholesky factor that logpdf takes of the squared variance, so z = F^{-1} e and log |F_jj| give the same density.
template <int P, int NA>
__device__ __forceinline__ double magi_step_sqrt(const double (&Q)[P][P], const double (&LR)[P][P], const double (&x)[NA],
                                                 double (&mu)[P], double (&L)[P][P]) {
    double mup[P], Lp[P][P];
    sqrt_predict<P>(Q, LR, mu, L, mup, Lp);
    double WL[NA][P], zc[NA][1], F[NA][NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        zc[j][0] = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) WL[j][c] = Lp[j][c];
    }
    add_sqrt<NA, P, 1>(WL, zc, F);                                      // (a zero row adds nothing to the QR)
    double e[NA], z[NA][1], det = 1.0, zz = 0.0;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        e[j] = x[j] - mup[j];
        z[j][0] = e[j];
    }
    solve_lower<NA, 1>(F, z);
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        zz = fma(z[j][0], z[j][0], zz);
        det *= F[j][j];
    }
    // K^T = F^{-T} (F^{-1} W) Lp Lp^T; F^{-1} W is zero beyond column NA, so only its NA x NA part is formed
    double T1[NA][NA], T2[NA][P], K[NA][P];
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
        for (int l = 0; l < NA; ++l) T1[j][l] = j == l ? 1.0 : 0.0;
    solve_lower<NA, NA>(F, T1);
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
        for (int c = 0; c < P; ++c) {
            double s = T1[j][0] * WL[0][c];
#pragma unroll
            for (int l = 1; l < NA; ++l) s = fma(T1[j][l], WL[l][c], s);
            T2[j][c] = s;                                               // F^{-1} W Lp
        }
    mm_nt<NA, P, P>(T2, Lp, K);
    solve_upper_t<NA, P>(F, K);
    double A[P][P], zp[P][1];
#pragma unroll
    for (int r = 0; r < P; ++r) {
        double t = K[0][r] * e[0];
#pragma unroll
        for (int j = 1; j < NA; ++j) t = fma(K[j][r], e[j], t);
        mu[r] = mup[r] + t;
        zp[r][0] = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            double u = K[0][r] * WL[0][c];                              // (K W) Lp = K Lp[:NA, :]
#pragma unroll
            for (int j = 1; j < NA; ++j) u = fma(K[j][r], WL[j][c], u);
            A[r][c] = Lp[r][c] - u;
        }
    }
    add_sqrt<P, P, 1>(A, zp, L);                                        // add_sqrt(Lp - K W Lp, K var_meas = 0)
    return -0.5 * zz - log(fabs(det)) - 0.5 * NA * MAGI_LOG_2PI;
}

template <int P>
__device__ __forceinline__ void magi_load_prior(const MagiArgs& a, int blk, int b, double (&Q)[P][P], double (&R)[P][P]) {
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const size_t e = ((size_t)blk * P + i) * P + j;
            Q[i][j] = ld(a.Q, e, a.Q_b, a.B, b);
            R[i][j] = ld(a.R, e, a.R_b, a.B, b);
        }
}

// The sum over the N steps of one block's log-densities.  Q and R stay in registers up to P = 5 and are read again every
// step beyond (L2 hits), as in fwd_sqrt_kernel.  x_meas is loaded PF steps ahead of its use.
template <int P, int NA, bool SQRT>
__device__ __forceinline__ double magi_block(const MagiArgs& a, int blk, int b) {
    constexpr bool HOIST = P <= 5;
    constexpr int PF = magi_prefetch<NA>();
    const size_t B = (size_t)a.B, js = a.xm_b ? B : 1, ns = (size_t)a.D * NA * js;
    const double* xp = a.xm + (size_t)blk * NA * js + (a.xm_b ? (size_t)b : 0);
    double mu[P], S[P][P], Qh[HOIST ? P : 1][HOIST ? P : 1], Rh[HOIST ? P : 1][HOIST ? P : 1];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        mu[i] = ld(a.x0, (size_t)blk * P + i, a.x0_b, a.B, b);
#pragma unroll
        for (int j = 0; j < P; ++j) S[i][j] = 0.0;
    }
    if constexpr (HOIST) magi_load_prior<P>(a, blk, b, Qh, Rh);
    double xb[PF][NA];
#pragma unroll
    for (int k = 0; k < PF; ++k)
#pragma unroll
        for (int j = 0; j < NA; ++j) xb[k][j] = k < a.N ? xp[(size_t)k * ns + j * js] : 0.0;
    double acc = 0.0;
    for (int n0 = 0; n0 < a.N; n0 += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            if (n0 + k < a.N) {
                double x[NA];
#pragma unroll
                for (int j = 0; j < NA; ++j) x[j] = xb[k][j];
                const int nn = n0 + k + PF;
                if (nn < a.N) {
#pragma unroll
                    for (int j = 0; j < NA; ++j) xb[k][j] = xp[(size_t)nn * ns + j * js];
                }
                double lp;
                if constexpr (HOIST) {
                    lp = SQRT ? magi_step_sqrt<P, NA>(Qh, Rh, x, mu, S) : magi_step_std<P, NA>(Qh, Rh, x, mu, S);
                } else {
                    // the loop stores nothing, so the compiler would hoist these loads and hold both matrices across the
                    // loop (it spilled): an empty asm makes the base pointers new values every step
                    MagiArgs ap = a;
                    asm volatile("" : "+s"(ap.Q), "+s"(ap.R));
                    double Q[P][P], R[P][P];
                    magi_load_prior<P>(ap, blk, b, Q, R);
                    lp = SQRT ? magi_step_sqrt<P, NA>(Q, R, x, mu, S) : magi_step_std<P, NA>(Q, R, x, mu, S);
                }
                acc += lp;
            }
        }
    }
    return acc;
}

// grid (ceil(B / 64) D), block 64: one lane per (trajectory, block).  Workgroup g runs block g / ceil(B / 64) of the
// trajectories 64 (g mod ceil(B / 64)) + lane and writes that block's sum to part[blk * B + b]; with one block, part is
// logdens itself.
template <int P, int NA, bool SQRT>
__global__ void __launch_bounds__(64) magi_kernel(MagiArgs a, double* __restrict__ part) {
    const int nbx = (a.B + 63) >> 6;
    const int blk = blockIdx.x / nbx;
    const int b = (blockIdx.x - blk * nbx) * 64 + threadIdx.x;
    if (b < a.B) part[(size_t)blk * a.B + b] = magi_block<P, NA, SQRT>(a, blk, b);
}

// logdens[b] = the D block sums of trajectory b, added in block order: no atomics, the same bits on every run.
__global__ void __launch_bounds__(256) magi_sum_kernel(const double* __restrict__ part, int B, int D,
                                                       double* __restrict__ logdens) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) {
        double s = part[b];
        for (int k = 1; k < D; ++k) s += part[(size_t)k * B + b];
        logdens[b] = s;
    }
}

}  // namespace rk
