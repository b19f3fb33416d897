// Fenrir's backward filter on the lanes: the pieces that fenrir_bwd_kernel (fenrir.hip, observations on grid nodes) and
// fenrir_bwd_at_kernel (fenrir_at_kernels.hpp, observations anywhere) share.  The vector-observation update of both is
// dalton_observe (dalton_kernels.hpp).  Not part of the hiprtc program text (embed_sources.py).
#pragma once
#include "dalton_kernels.hpp"

namespace rk {

// The stored backward filter of fenrir's solve_mv (fenrir_bwd_kernel with STORE -> fenrir_smooth_kernel): per (time n, block) a
// batch-minor item [m_pred, S_pred | m_filt, S_filt | A] of n_bstate = p; element offsets of its fields and its doubles
struct FenrirItem {
    int pred, filt, A, width;
    constexpr explicit FenrirItem(int p) : pred(0), filt(p + p * p), A(2 * (p + p * p)), width(3 * p * p + 2 * p) {}
};

// One step of the backward Markov chain (smooth_cond, standard.py:366-370) as a Kalman prediction of the carry (bm, bS) from
// time n + 1 to n, given filt[n] = (mf, Sf) and pred[n + 1] = (mp, Sp); G is the step's weight A
template <int P>
__device__ __forceinline__ void fenrir_markov_step(const double (&Q)[P][P], const double (&mf)[P], const double (&Sf)[P][P],
                                                   const double (&mp)[P], const double (&Sp)[P][P], double (&bm)[P],
                                                   double (&bS)[P][P], double (&G)[P][P]) {
    double T[P][P];
    smooth_gain<P>(Q, Sf, Sp, T, G);                                    // A = G            (standard.py:175-176)
    double bb[P], Cc[P][P], GT[P][P];
    mm_nt<P, P, P>(G, T, GT);
#pragma unroll
    for (int r = 0; r < P; ++r) {
        bb[r] = mf[r] - dot<P>(G[r], mp);                               // b = mu_f - G mu-   (standard.py:368)
#pragma unroll
        for (int c = 0; c < P; ++c) Cc[r][c] = Sf[r][c] - GT[r][c];     // C = Sigma_f - G T^T (standard.py:369-370)
    }
    double nm[P], nS[P][P];
    predict_block<P>(G, Cc, bm, bS, nm, nS);                            // A m + 0, A S A^T + C (standard.py:57-59)
#pragma unroll
    for (int r = 0; r < P; ++r) {
        bm[r] = nm[r] + bb[r];
#pragma unroll
        for (int c = 0; c < P; ++c) bS[r][c] = nS[r][c];
    }
}

// fenrir_bwd_kernel's conditioning on a scalar observation of the block (row ib = i * D + blk): forecast (standard.py:333-335),
// log-density (utils.py:60-78) and update (standard.py:93-102) with K = Sigma D^T / w.  Not dalton_observe<P, 1>, which solves
// the 1 x 1 system by LU and rounds differently.
template <int P>
__device__ __forceinline__ void fenrir_observe_scalar(const DaltonObs& o, size_t ib, double (&m)[P], double (&S)[P][P], double& acc) {
    const double LOG_2PI = 1.83787706640934548356;
    double D[P], SD[P];
#pragma unroll
    for (int k = 0; k < P; ++k) D[k] = o.obs_w[ib * P + k];
    const double y = o.obs[ib], Om = o.obs_v[ib];
    const double mean_fore = dot<P>(D, m);
#pragma unroll
    for (int r = 0; r < P; ++r) SD[r] = dot<P>(S[r], D);                // Sigma D^T
    double DS[P];
#pragma unroll
    for (int c = 0; c < P; ++c) {
        double t = D[0] * S[0][c];
#pragma unroll
        for (int k = 1; k < P; ++k) t = fma(D[k], S[k][c], t);
        DS[c] = t;                                                      // D Sigma
    }
    const double w = dot<P>(DS, D) + Om;                                // var_fore
    const double z = y - mean_fore;
    if (fabs(w) > 1e-8) acc += -0.5 * (z * z / w + log(w)) - 0.5 * LOG_2PI;
#pragma unroll
    for (int r = 0; r < P; ++r) {
        const double K = SD[r] / w;                                     // solve_var with a 1 x 1 system
        m[r] = fma(K, z, m[r]);
#pragma unroll
        for (int c = 0; c < P; ++c) S[r][c] = fma(-K, DS[c], S[r][c]);
    }
}

}  // namespace rk
