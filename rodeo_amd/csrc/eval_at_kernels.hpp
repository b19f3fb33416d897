// The solver's posterior at arbitrary times (rk_eval_at), one lane per (query, trajectory, block), no time loop.
// By the prior's Markov property the posterior at t in (t_n, t_{n+1}) needs the filtered moments at t_n, the smoothed ones
// at t_{n+1} and the prior's transitions over h1 = t - t_n and h2 = t_{n+1} - t:
//   (mu_t, Sigma_t) = predict(filt[n]; Q1, R1)                       standard.py:57-59
//   (mu', Sigma')   = predict((mu_t, Sigma_t); Q2, R2)
//   G = Sigma_t Q2^T Sigma'^{-1}                                     standard.py:175-176 (the LU solve of bwd_mv_kernel)
//   mu = mu_t + G (mu^s[n+1] - mu'),  Sigma = Sigma_t + G (Sigma^s[n+1] - Sigma') G^T       standard.py:213-216
// A query on a node copies that node's smoothed record.  Host side: eval_at.hip.
#pragma once
#include "../../include/rodeo_kalman.h"
#include "kalman_small.hpp"
#include "records.hpp"
#include "solve_args.hpp"

namespace rk {

struct EvalAtArgs {
    int B, N, D, T, n_quad;
    const double *fmean, *fvar;     // records of rk_solve_filter (fmean: batch-minor layout only)
    const double *smean, *svar;     // records of rk_solve_mv, same layout
    const int32_t* query;           // (T, 3): node n, on-node flag, slot of the (Q1, R1, Q2, R2) quadruple
    const double *trans, *noise;    // (n_quad, 2, D, P, P [,B]): (Q1, Q2) and (R1, R2), batch-minor when batched
    int trans_b, noise_b;
    double *mean_out, *var_out;     // (B, T, D, P) and (B, T, D, P, P): the reference's layout, batch first
};

// matrix `which` (0: over h1, 1: over h2) of quadruple `slot`
template <int P>
__device__ __forceinline__ void eval_at_prior(const EvalAtArgs& a, int slot, int which, int blk, int b, double (&Q)[P][P],
                                              double (&R)[P][P]) {
    const size_t base = (((size_t)slot * 2 + which) * a.D + blk) * P * P;
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) {
            Q[i][j] = ld(a.trans, base + i * P + j, a.trans_b, a.B, b);
            R[i][j] = ld(a.noise, base + i * P + j, a.noise_b, a.B, b);
        }
}

// grid (T ceil(B D / 64)), block 64: workgroup g serves query g / ceil(B D / 64), so the query's node, flag and slot are the
// same in every lane of a wave and the on-node branch does not diverge.  The indices are clamped to the buffers.
// LAYOUT: the filter's records; SLAYOUT: the smoother's -- the same but for RK_LAYOUT_TILE3_PACKED, which only rk_solve_mv writes.
// Smoothed p = 3 tile records are read with Sigma mirrored from its upper triangle (records.hpp) in both layouts.
template <int P, int LAYOUT, int SLAYOUT = LAYOUT>
__global__ void __launch_bounds__(64) eval_at_kernel(EvalAtArgs a) {
    constexpr bool SYM = LAYOUT == RK_LAYOUT_TILE3;
    const int nbx = (a.B * a.D + 63) >> 6;
    const int q = blockIdx.x / nbx;
    const int l = (blockIdx.x - q * nbx) * 64 + threadIdx.x;
    if (l >= a.B * a.D) return;
    int blk, b;
    record_lane<LAYOUT>(l, a.B, a.D, blk, b);
    const bool on = a.query[3 * q + 1] != 0;
    const int n = min(max(a.query[3 * q], 0), on ? a.N : a.N - 1);
    const int slot = min(max(a.query[3 * q + 2], 0), a.n_quad - 1);

    double mu[P], S[P][P];
    if (on) {
        load_moments<P, SLAYOUT, SYM>(a.smean, a.svar, a.B, a.D, n, blk, b, mu, S, a.N);
    } else {
        // Three stages, each with its own loads.  The scheduler would issue every load up front and hold 4 P^2 + 2 P (prior) +
        // 2 (P^2 + P) (records) doubles under the whole computation (P = 6 spilled): the barriers keep Q1, R1 and the filtered
        // moments dead before Q2 and R2 are loaded, and Q2, R2 dead before the smoothed record is.
        double mt[P], St[P][P];
        {
            double Q1[P][P], R1[P][P], mf[P], Sf[P][P];
            eval_at_prior<P>(a, slot, 0, blk, b, Q1, R1);
            load_moments<P, LAYOUT>(a.fmean, a.fvar, a.B, a.D, n, blk, b, mf, Sf);
            predict_block<P>(Q1, R1, mf, Sf, mt, St);
        }
        __builtin_amdgcn_sched_barrier(0);
        double mp[P], Sp[P][P], G[P][P];
        {
            double Q2[P][P], R2[P][P], Tm[P][P];
            eval_at_prior<P>(a, slot, 1, blk, b, Q2, R2);
            predict_block<P>(Q2, R2, mt, St, mp, Sp);
            smooth_gain<P>(Q2, St, Sp, Tm, G);
        }
        __builtin_amdgcn_sched_barrier(0);
        load_moments<P, SLAYOUT, SYM>(a.smean, a.svar, a.B, a.D, n + 1, blk, b, mu, S, a.N);
        smooth_mv_block<P>(G, mt, St, mp, Sp, mu, S);
    }
    double* mo = a.mean_out + ((((size_t)b * a.T + q) * a.D + blk) * P);
    double* vo = a.var_out + ((((size_t)b * a.T + q) * a.D + blk) * P * P);
#pragma unroll
    for (int i = 0; i < P; ++i) {
        mo[i] = mu[i];
#pragma unroll
        for (int j = 0; j < P; ++j) vo[i * P + j] = S[i][j];
    }
}

}  // namespace rk
