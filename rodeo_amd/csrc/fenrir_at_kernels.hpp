// fenrir_at: Fenrir's log-likelihood for observations whose times need not be nodes of the solver grid (DESIGN.md section 7
// (11)).  Fenrir's forward pass is free of data; the observations enter the backward Markov chain, so an observation inside a
// step means extra backward hops.  For the off-grid observation times t_n < tau_1 < .. < tau_k < t_n+1 with gaps h_0 .. h_k and
// (Q_j, R_j) the prior over h_j, the forward moments at the inner times are plain predictions from filt[n]:
//     s_0 = filt[n],   e_j = predict(s_j; Q_j, R_j),   s_j+1 = e_j   (j < k),       e_k = pred[n+1]  (Chapman-Kolmogorov)
// and hop j = k .. 0 of the backward chain is one smooth_cond map (standard.py:366-370) applied to the carry (m, M):
//     G_j = Sigma(s_j) Q_j^T Sigma(e_j)^-1 ;   m <- mu(s_j) + G_j (m - mu(e_j)) ;   M <- Sigma(s_j) + G_j (M - Sigma(e_j)) G_j^T
// Nothing of s_j, e_j, G_j depends on the carry: fenrir_at_hops_kernel evaluates them time-parallel before the chain runs, and
// the chain kernels (fenrir_bwd_at_kernel here, fenrir_bwd_at_tile3_kernel in solve_tile3.hip) read them and add no LU.
#pragma once
#include "../../include/rodeo_kalman.h"
#include "fenrir_kernels.hpp"
#include "records.hpp"
#include "fenrir_at_args.hpp"

namespace rk {

// prior pair `slot` of (q, r) (n, D, P, P [, B])
template <int P>
__device__ __forceinline__ void fenrir_at_pair(const double* q, const double* r, int slot, int D, int blk, int batched, int B, int b,
                                               double (&Q)[P][P], double (&R)[P][P]) {
    const size_t base = ((size_t)slot * D + blk) * P * P;
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) {
            Q[i][j] = ld(q, base + i * P + j, batched, B, b);
            R[i][j] = ld(r, base + i * P + j, batched, B, b);
        }
}

// One lane per (hop, trajectory, block), no time loop (the shape of eval_at_kernel).  grid (2 n_obs ceil(B D / 64)), block 64:
// workgroup g serves hop id g / ceil(B D / 64) = 2 i + which -- the hop in front of observation i (which = 0, record `pre slot`)
// or, for an interval's last observation, the hop behind it (which = 1, record n_pre + post slot) -- so the table row, the
// trip count of the chain and every branch are the same in all lanes of a wave.  Hop ids of on-node observations and of
// observations without a post slot have no record and leave at once.  The lane walks the interval's chain from filt[n]
// (read through load_moments in the plan's layout) up to its hop, serially: an interval with k observations costs its
// last hop k + 1 predicts, and nothing here or in the workspace (one record per pair) bounds k.  Indices are clamped to the
// buffers.
// LAYOUT = RK_LAYOUT_TILE3 (P = 3): a.var holds the filter's tile records, the record written is the tile form;
// LAYOUT = RK_LAYOUT_BATCH_MINOR: a.mean / a.var hold the batch-minor filtered moments, the record is the lane form.
template <int P, int LAYOUT>
__global__ void __launch_bounds__(64) fenrir_at_hops_kernel(SolveArgs a, FenrirAt f) {
    const int nbx = (a.B * a.D + 63) >> 6;
    const int q = blockIdx.x / nbx;
    const int l = (blockIdx.x - q * nbx) * 64 + threadIdx.x;
    if (l >= a.B * a.D) return;
    int blk, b;
    record_lane<LAYOUT>(l, a.B, a.D, blk, b);
    const int i = fenrir_at_clamp(q >> 1, f.n_obs), which = q & 1;
    const int32_t* row = f.tab + 4 * i;
    if (row[1] == 0 || (which && row[3] < 0)) return;                       // (wave-uniform)
    const int n = fenrir_at_clamp(row[0], a.N);
    int i0 = i;                                                               // first observation of the interval
    while (i0 > 0 && f.tab[4 * (i0 - 1) + 1] != 0 && f.tab[4 * (i0 - 1)] == row[0]) --i0;

    double ms[P], Ss[P][P];
    load_moments<P, LAYOUT>(a.mean, a.var, a.B, a.D, n, blk, b, ms, Ss);      // s_0 = filt[n]
    for (int m = i0; m < i + which; ++m) {                                    // s_j+1 = predict(s_j; Q_j, R_j)
        double Qm[P][P], Rm[P][P], mt[P], St[P][P];
        fenrir_at_pair<P>(f.pre_q, f.pre_r, fenrir_at_clamp(f.tab[4 * m + 2], f.n_pre), a.D, blk, f.prior_b, a.B, b, Qm, Rm);
        predict_block<P>(Qm, Rm, ms, Ss, mt, St);
#pragma unroll
        for (int r = 0; r < P; ++r) {
            ms[r] = mt[r];
#pragma unroll
            for (int c = 0; c < P; ++c) Ss[r][c] = St[r][c];
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    double me[P], Se[P][P], G[P][P];
    int rec;
    {
        double Qh[P][P], Rh[P][P], T[P][P];
        if (which) {
            rec = fenrir_at_clamp(row[3], f.n_post);
            fenrir_at_pair<P>(f.post_q, f.post_r, rec, a.D, blk, f.prior_b, a.B, b, Qh, Rh);
            rec += f.n_pre;
        } else {
            rec = fenrir_at_clamp(row[2], f.n_pre);
            fenrir_at_pair<P>(f.pre_q, f.pre_r, rec, a.D, blk, f.prior_b, a.B, b, Qh, Rh);
        }
        predict_block<P>(Qh, Rh, ms, Ss, me, Se);                             // e_j                      (standard.py:57-59)
        smooth_gain<P>(Qh, Ss, Se, T, G);                                     // G_j, the LU of bwd_mv_kernel (standard.py:175-176)
    }
    if constexpr (LAYOUT == RK_LAYOUT_TILE3) {
        static_assert(P == 3, "the tile records are the n_bstate = 3 hand-off items");
        // [M- | G~^T | M_f] augmented like tile3_gain_producers' items: row 3 = e_3, column 3 of G~^T = e_3
        double* o = f.hops + ((size_t)rec * a.B * a.D + (size_t)b * a.D + blk) * FENRIR_AT_TILE_REC;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                o[4 * r + c] = Se[r][c];
                o[16 + 4 * r + c] = G[c][r];
                o[32 + 4 * r + c] = Ss[r][c];
            }
            o[4 * r + 3] = me[r];
            o[16 + 4 * r + 3] = 0.0;
            o[32 + 4 * r + 3] = ms[r];
        }
#pragma unroll
        for (int w = 0; w < 3; ++w)
#pragma unroll
            for (int c = 0; c < 4; ++c) o[16 * w + 12 + c] = c == 3 ? 1.0 : 0.0;
    } else {
        constexpr FenrirAtLaneRec REC(P);
        const size_t B = (size_t)a.B;
        double* o = f.hops + ((size_t)rec * a.D + blk) * REC.width * B + b;
#pragma unroll
        for (int r = 0; r < P; ++r) {
            o[(size_t)(REC.s + r) * B] = ms[r];
            o[(size_t)(REC.e + r) * B] = me[r];
#pragma unroll
            for (int c = 0; c < P; ++c) {
                o[(size_t)(REC.s + P + r * P + c) * B] = Ss[r][c];
                o[(size_t)(REC.e + P + r * P + c) * B] = Se[r][c];
                o[(size_t)(REC.G + r * P + c) * B] = G[r][c];
            }
        }
    }
}

// fenrir_bwd_kernel<P, false, MO, false> (fenrir.hip) for observations anywhere: one lane per (block, trajectory) over the
// batch-minor filtered and predicted moments, with that kernel's Markov step (fenrir_markov_step, fenrir_kernels.hpp).  At an
// interval with off-grid observations it runs the hops from the batch-minor hop records -- G is read, not solved for -- with
// the conditioning (dalton_observe, at MO = 1 too) between them; the table index i is wave-uniform.
template <int P, int MO>
__global__ void __launch_bounds__(64) fenrir_bwd_at_kernel(SolveArgs a, FenrirAt f) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= a.B * a.D) return;
    const int blk = l / a.B, b = l - blk * a.B;
    const size_t B = (size_t)a.B;
    constexpr FenrirAtLaneRec REC(P);
    double Q[P][P];
    {
        double R[P][P];
        load_block_consts<P>(a, blk, b, Q, R);
    }
    DaltonObs o;
    o.obs = f.obs; o.obs_w = f.obs_w; o.obs_v = f.obs_v; o.obs_ind = nullptr; o.n_obs = f.n_obs;
    double bm[P], bS[P][P];
    load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, a.B, a.D, a.N, blk, b, bm, bS);   // terminal point (fenrir.py:186-188)
    double acc = 0.0;
    int i = f.n_obs - 1;
    auto observe = [&]() {
        dalton_observe<P, MO>(o, (size_t)i * a.D + blk, bm, bS, acc);
        --i;
    };
    // the carry through the hop of record `rec`: smooth_mv_block is the smooth_cond map applied to (m, M)
    auto hop = [&](int rec) {
        const double* h = f.hops + ((size_t)rec * a.D + blk) * REC.width * B + b;
        double msj[P], Ssj[P][P], mej[P], Sej[P][P], G[P][P];
#pragma unroll
        for (int r = 0; r < P; ++r) {
            msj[r] = h[(size_t)(REC.s + r) * B];
            mej[r] = h[(size_t)(REC.e + r) * B];
#pragma unroll
            for (int c = 0; c < P; ++c) {
                Ssj[r][c] = h[(size_t)(REC.s + P + r * P + c) * B];
                Sej[r][c] = h[(size_t)(REC.e + P + r * P + c) * B];
                G[r][c] = h[(size_t)(REC.G + r * P + c) * B];
            }
        }
        smooth_mv_block<P>(G, msj, Ssj, mej, Sej, bm, bS);
    };
    if (i >= 0 && f.tab[4 * i + 1] == 0 && f.tab[4 * i] >= a.N) observe();                 // fenrir.py:189-209
    for (int n = a.N - 1; n >= 0; --n) {
        if (i >= 0 && f.tab[4 * i + 1] != 0 && f.tab[4 * i] == n) {
            // ---- the interval (t_n, t_n+1) holds observations: hop k behind the last one, then condition / hop in turn ----
            hop(f.n_pre + fenrir_at_clamp(f.tab[4 * i + 3], f.n_post));
            do {
                const int pre = fenrir_at_clamp(f.tab[4 * i + 2], f.n_pre);
                observe();
                hop(pre);
            } while (i >= 0 && f.tab[4 * i + 1] != 0 && f.tab[4 * i] == n);
        } else {
            double mf[P], Sf[P][P], mp[P], Sp[P][P], G[P][P];
            load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, a.B, a.D, n, blk, b, mf, Sf);
            load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean_pred, a.var_pred, a.B, a.D, n + 1, blk, b, mp, Sp);   // solve.py:93-96
            fenrir_markov_step<P>(Q, mf, Sf, mp, Sp, bm, bS, G);
        }
        if (i >= 0 && f.tab[4 * i + 1] == 0 && f.tab[4 * i] == n) observe();   // fenrir.py:155-170
    }
    atomicAdd(&f.logdens[b], acc);
}

}  // namespace rk
