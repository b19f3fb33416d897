// Per-block Kalman step maps on register-resident blocks (n_bmeas = 1), one (trajectory, block) per lane.
// Each function cites the reference lines it computes; NumPy mirrors: oracle/kalman_ops.py.
#pragma once
#include "linalg_small.hpp"

namespace rk {

// standard.py:57-59 with mean_state = 0 (solve.py:52):  mu- = Q mu ;  Sigma- = (Q Sigma) Q^T + R.
// Used by the forward kernel AND re-evaluated by the backward kernels (the predicted moments are not stored);
// it is written with explicit fma chains so both evaluations round identically.
template <int P>
__device__ __forceinline__ void predict_block(const double (&Q)[P][P], const double (&R)[P][P],
                                              const double (&mu)[P], const double (&S)[P][P],
                                              double (&mup)[P], double (&Sp)[P][P]) {
    mv<P, P>(Q, mu, mup);
    double A[P][P];
    mm<P, P, P>(Q, S, A);
    mm_nt<P, P, P>(A, Q, Sp);
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) Sp[i][j] = Sp[i][j] + R[i][j];
}

// standard.py:93-102 for n_bmeas = 1, x_meas = 0 (solve.py:51):
//   yhat = W mu- + a ; S = (W Sigma-) W^T + V ; K = Sigma- W^T / S ; mu = mu- + K (0 - yhat) ; Sigma = Sigma- - K (W Sigma-)
// The one body of the lane filters' scalar z updates; it hands back the innovation 0 - yhat and its forecast variance s.
// GAIN is how K = Sigma- W^T / s is divided, the only thing in which the filters differ: fast_rcp(s) multiplied (the solver's
// forward filter), one IEEE division per element (DALTON, whose log-density shares s), or the reciprocal 1.0 / s multiplied
// (solve_evidence and the dynamic solver, whose z^2 / s uses the same reciprocal).  Returns the reciprocal it multiplied with
// (0 under GAIN_DIVIDE, which has none).
enum GainRule { GAIN_FAST_RCP, GAIN_DIVIDE, GAIN_RCP };
template <int P, GainRule GAIN>
__device__ __forceinline__ double update_z(const double (&W)[P], double a, double V, const double (&mup)[P],
                                         const double (&Sp)[P][P], double (&mu)[P], double (&S)[P][P], double& innov,
                                         double& s) {
    const double yhat = dot<P>(W, mup) + a;
    double WS[P], SW[P];
    row_mat<P>(W, Sp, WS);
    s = dot<P>(WS, W) + V;                                                  // var_fore
    innov = 0.0 - yhat;
#pragma unroll
    for (int i = 0; i < P; ++i) SW[i] = dot<P>(Sp[i], W);
    double rs = 0.0;
    if constexpr (GAIN == GAIN_FAST_RCP) rs = fast_rcp(s);
    if constexpr (GAIN == GAIN_RCP) rs = 1.0 / s;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const double K = GAIN == GAIN_DIVIDE ? SW[i] / s : SW[i] * rs;
        mu[i] = fma(K, innov, mup[i]);
#pragma unroll
        for (int j = 0; j < P; ++j) S[i][j] = fma(-K, WS[j], Sp[i][j]);
    }
    return rs;
}

template <int P>
__device__ __forceinline__ void update_block_m1(const double (&W)[P], double a, double V,
                                                const double (&mup)[P], const double (&Sp)[P][P],
                                                double (&mu)[P], double (&S)[P][P]) {
    double innov, s;
    update_z<P, GAIN_FAST_RCP>(W, a, V, mup, Sp, mu, S, innov, s);
}

// standard.py:93-102 (LU) of one block on a vector observation y = D x + N(0, Om) held in registers, in two halves so that a
// caller can put the forecast's log-density between them (dalton_observe): observe_forecast gives the innovation z, D Sigma
// and the forecast variance Wf; observe_apply solves for the gain (Wf is destroyed) and updates (m, S).  A padded row (zero
// weight, unit variance, zero datum) is an exact no-op: its forecast row / column is a unit vector that the pivot search never
// picks for another column.
template <int P, int MO>
__device__ __forceinline__ void observe_forecast(const double (&D)[MO][P], const double (&y)[MO], const double (&Om)[MO][MO],
                                                 const double (&m)[P], const double (&S)[P][P], double (&z)[MO],
                                                 double (&DS)[MO][P], double (&Wf)[MO][MO]) {
#pragma unroll
    for (int j = 0; j < MO; ++j) {
        z[j] = y[j] - dot<P>(D[j], m);
        row_mat<P>(D[j], S, DS[j]);                                         // D Sigma
    }
#pragma unroll
    for (int j = 0; j < MO; ++j)
#pragma unroll
        for (int l = 0; l < MO; ++l) Wf[j][l] = dot<P>(DS[j], D[l]) + Om[j][l];    // var_fore
}
template <int P, int MO>
__device__ __forceinline__ void observe_apply(const double (&D)[MO][P], const double (&z)[MO], const double (&DS)[MO][P],
                                              double (&Wf)[MO][MO], double (&m)[P], double (&S)[P][P]) {
    double X[MO][P];
#pragma unroll
    for (int j = 0; j < MO; ++j)
#pragma unroll
        for (int r = 0; r < P; ++r) X[j][r] = dot<P>(S[r], D[j]);           // (Sigma D^T)^T
    lu_solve<MO, P>(Wf, X);                                                 // K^T
#pragma unroll
    for (int r = 0; r < P; ++r) {
        double t = X[0][r] * z[0];
#pragma unroll
        for (int j = 1; j < MO; ++j) t = fma(X[j][r], z[j], t);
        double dS[P];
#pragma unroll
        for (int c = 0; c < P; ++c) {
            double u = X[0][r] * DS[0][c];
#pragma unroll
            for (int j = 1; j < MO; ++j) u = fma(X[j][r], DS[j][c], u);
            dS[c] = u;
        }
        m[r] = m[r] + t;
#pragma unroll
        for (int c = 0; c < P; ++c) S[r][c] = S[r][c] - dS[c];
    }
}
// both halves: the update without a log-density
template <int P, int MO>
__device__ __forceinline__ void observe_update(const double (&D)[MO][P], const double (&y)[MO], const double (&Om)[MO][MO],
                                               double (&m)[P], double (&S)[P][P]) {
    double z[MO], DS[MO][P], Wf[MO][MO];
    observe_forecast<P, MO>(D, y, Om, m, S, z, DS, Wf);
    observe_apply<P, MO>(D, z, DS, Wf, m, S);
}

// standard.py:175-176:  T = Sigma_f Q^T ;  G = solve(Sigma-, T^T)^T  (LU with partial pivoting, utils.py:119)
template <int P>
__device__ __forceinline__ void smooth_gain(const double (&Q)[P][P], const double (&Sf)[P][P],
                                            const double (&Sp)[P][P], double (&T)[P][P], double (&G)[P][P]) {
    mm_nt<P, P, P>(Sf, Q, T);
    double A[P][P], X[P][P];
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) {
            A[i][j] = Sp[i][j];
            X[i][j] = T[j][i];
        }
    lu_solve<P, P>(A, X);
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) G[i][j] = X[j][i];
}

// standard.py:213-216:  mu_s = mu_f + G (mu_next - mu-) ;  Sigma_s = Sigma_f + (G (Sigma_next - Sigma-)) G^T
template <int P>
__device__ __forceinline__ void smooth_mv_block(const double (&G)[P][P], const double (&mf)[P],
                                                const double (&Sf)[P][P], const double (&mp)[P],
                                                const double (&Sp)[P][P], double (&ms)[P], double (&Ss)[P][P]) {
    double dm[P], D[P][P], GD[P][P], GDG[P][P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        dm[i] = ms[i] - mp[i];
#pragma unroll
        for (int j = 0; j < P; ++j) D[i][j] = Ss[i][j] - Sp[i][j];
    }
    double gm[P];
    mv<P, P>(G, dm, gm);
    mm<P, P, P>(G, D, GD);
    mm_nt<P, P, P>(GD, G, GDG);
#pragma unroll
    for (int i = 0; i < P; ++i) {
        ms[i] = mf[i] + gm[i];
#pragma unroll
        for (int j = 0; j < P; ++j) Ss[i][j] = Sf[i][j] + GDG[i][j];
    }
}

// standard.py:251-254:  mean_sim = mu_f + G (x_next - mu-) ;  var_sim = Sigma_f - G T^T
template <int P>
__device__ __forceinline__ void smooth_sim_block(const double (&G)[P][P], const double (&T)[P][P],
                                                 const double (&mf)[P], const double (&Sf)[P][P],
                                                 const double (&mp)[P], const double (&xn)[P],
                                                 double (&msim)[P], double (&Ssim)[P][P]) {
    double dm[P], gm[P], GT[P][P];
#pragma unroll
    for (int i = 0; i < P; ++i) dm[i] = xn[i] - mp[i];
    mv<P, P>(G, dm, gm);
    mm_nt<P, P, P>(G, T, GT);
#pragma unroll
    for (int i = 0; i < P; ++i) {
        msim[i] = mf[i] + gm[i];
#pragma unroll
        for (int j = 0; j < P; ++j) Ssim[i][j] = Sf[i][j] - GT[i][j];
    }
}

// x = mean + psd_factor(var) z
template <int P>
__device__ __forceinline__ void mvn_draw(const double (&mean)[P], const double (&var)[P][P],
                                         const double (&z)[P], double (&x)[P]) {
    double L[P][P];
    psd_factor<P>(var, L);
#pragma unroll
    for (int i = 0; i < P; ++i) {
        double s = mean[i];
#pragma unroll
        for (int k = 0; k <= i; ++k) s = fma(L[i][k], z[k], s);
        x[i] = s;
    }
}

// smooth_sim_block and mvn_draw in the parts that depend on the draw and the parts that do not, for a caller that takes
// several draws from one (G, T, filt) (sim_draws.hip): per step once smooth_sim_var and psd_factor, per draw smooth_sim_mean
// and mvn_apply.  The products, their fma chains and their order are those of the two functions above.
// var_sim = Sigma_f - G T^T
template <int P>
__device__ __forceinline__ void smooth_sim_var(const double (&G)[P][P], const double (&T)[P][P], const double (&Sf)[P][P],
                                               double (&Ssim)[P][P]) {
    double GT[P][P];
    mm_nt<P, P, P>(G, T, GT);
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) Ssim[i][j] = Sf[i][j] - GT[i][j];
}
// mean_sim = mu_f + G (x_next - mu-)
template <int P>
__device__ __forceinline__ void smooth_sim_mean(const double (&G)[P][P], const double (&mf)[P], const double (&mp)[P],
                                                const double (&xn)[P], double (&msim)[P]) {
    double dm[P], gm[P];
#pragma unroll
    for (int i = 0; i < P; ++i) dm[i] = xn[i] - mp[i];
    mv<P, P>(G, dm, gm);
#pragma unroll
    for (int i = 0; i < P; ++i) msim[i] = mf[i] + gm[i];
}
// x = mean + L z with L = psd_factor(var), lower triangular
template <int P>
__device__ __forceinline__ void mvn_apply(const double (&mean)[P], const double (&L)[P][P], const double (&z)[P],
                                          double (&x)[P]) {
#pragma unroll
    for (int i = 0; i < P; ++i) {
        double s = mean[i];
#pragma unroll
        for (int k = 0; k <= i; ++k) s = fma(L[i][k], z[k], s);
        x[i] = s;
    }
}

}  // namespace rk
