// DALTON for non-Gaussian observations (src/rodeo/inference/dalton.py:547-1039), lane-per-trajectory kernels.
//
//   daltonng_fwd_kernel   -- _solve_filter_nn (:550-698): the joint filter of (Z, Yhat), whose pseudo-observation is built on
//                            the fly from the gradient and the diagonal Hessian blocks of the user's log-likelihood at the
//                            predicted mean (Dual2, dual2.hpp), and -- with BOTH -- the filter on Z alone (_solve_filter_ode) in
//                            the other half of the wave.  Always a hiprtc build: OBS is user code (rodeo_amd.trace).
//   daltonng_gain_kernel  -- time-parallel half of _logx_yhat (:701-784) and _logx_z (:787-849): gains, predicted means,
//                            masked precisions and log-determinant constants of smooth_sim's conditionals.
//   daltonng_chain_kernel -- the sequential half: the mean recursion of smooth_mv and the quadratic forms.
//   daltonng_obs_kernel   -- logy_x (:921-923) on plain doubles and the final logy_x + logx_z - logx_yhat (hiprtc).
//
// What is built where the reference's text cannot be taken literally: with A_b the state components of
// block b that the log-likelihood reads, the observation of block b is yhat = mu-[A_b] + V g_A, V = (-H_AA)^{-1}, with the
// selector of A_b as its weight; -H_AA that is not positive definite (a non-concave point, a non-finite derivative) gives
// NaN moments from there on, never a fault.  yhat is conditioned on after z within a step, expanded at mu-.
// RTC-safe: no host code.
#pragma once
#include "rk_enums.hpp"
#include "kalman_small.hpp"
#include "philox.hpp"
#include "solve_args.hpp"
#include "solve_small_kernels.hpp"
#include "dual2.hpp"

namespace rk {

// observations of rk_daltonng_*: y (n_obs, D, NY), obs_ind (n_obs) strictly increasing, <= N
struct NgObs {
    const double* y;
    const int32_t* obs_ind;
    int n_obs;
};

// workspace of rk_daltonng_loglik (batch-minor throughout)
struct NgWs {
    double *jm, *jv;      // joint filter: filtered means (N+1, D, P, B) and variances (N+1, D, P, P, B)
    double *zm, *zv;      // filter on Z alone, same shapes
    double* rec;          // gain records (N-1, D, E, B), E = ng_rec_doubles(P)
    double* sm;           // smoothed means at the observations' grid indices (n_obs, D, P, B)
    double* part;         // per-block sums (2, D, B): logx_z, logx_yhat
};

__host__ __device__ constexpr int ng_rec_doubles(int p) { return 3 * p * p + 2 * p + 2; }

// (weight, datum, variance) of the pseudo-observation of blocks BLK .. D-1 at the predicted means mup (dalton.py:614-622):
// one evaluation of the log-likelihood per block with that block's active components seeded, the other blocks constants,
// which yields exactly the diagonal Hessian block the reference keeps.
template <class OBS, int P, int MO, int BLK>
__device__ __forceinline__ void ng_pseudo_obs(const double (&y)[OBS::D][OBS::NY], const double (&mup)[OBS::D][P], double ind,
                                              const double (&th)[OBS::NTHETA], double (&Dm)[OBS::D][MO][P],
                                              double (&yh)[OBS::D][MO], double (&Om)[OBS::D][MO][MO]) {
    if constexpr (BLK < OBS::D) {
        constexpr int K = OBS::NACT[BLK];
        static_assert(K <= MO && K <= 3, "active set larger than the observation size");
#pragma unroll
        for (int k = 0; k < MO; ++k) {                                      // padding
            yh[BLK][k] = 0.0;
#pragma unroll
            for (int j = 0; j < P; ++j) Dm[BLK][k][j] = 0.0;
#pragma unroll
            for (int l = 0; l < MO; ++l) Om[BLK][k][l] = k == l ? 1.0 : 0.0;
        }
        if constexpr (K > 0) {
            constexpr int J0 = OBS::ACT[BLK][0], J1 = OBS::ACT[BLK][1], J2 = OBS::ACT[BLK][2];
            static_assert(J0 >= 0 && J0 < P && J1 >= 0 && J1 < P && J2 >= 0 && J2 < P, "active component out of range");
            const int J[3] = {J0, J1, J2};
            Dual2<K> X[OBS::D][P];
#pragma unroll
            for (int bb = 0; bb < OBS::D; ++bb)
#pragma unroll
                for (int j = 0; j < P; ++j) X[bb][j] = Dual2<K>(mup[bb][j]);
#pragma unroll
            for (int k = 0; k < K; ++k) X[BLK][J[k]].g[k] = 1.0;
            const Dual2<K> l = OBS::template loglik<Dual2<K>>(y, X, ind, th);
            double A[K][K], V[K][K];                                        // A = -H_AA
#pragma unroll
            for (int r = 0; r < K; ++r)
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    A[r][c] = -l.hess(r, c);
                    V[r][c] = r == c ? 1.0 : 0.0;
                }
            bool pd = A[0][0] > 0.0;                                        // Sylvester; false for NaN
            if constexpr (K >= 2) pd = pd && (A[0][0] * A[1][1] - A[0][1] * A[0][1] > 0.0);
            if constexpr (K == 3)
                pd = pd && (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[1][2]) - A[0][1] * (A[0][1] * A[2][2] - A[1][2] * A[0][2]) +
                            A[0][2] * (A[0][1] * A[1][2] - A[1][1] * A[0][2]) > 0.0);
            if constexpr (K == 1) V[0][0] = 1.0 / A[0][0];
            else lu_solve<K, K>(A, V);
            const double bad = __builtin_nan("");
#pragma unroll
            for (int r = 0; r < K; ++r) {
                double s = mup[BLK][J[r]];
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    const double v = pd ? V[r][c] : bad;
                    Om[BLK][r][c] = v;
                    s = fma(v, l.g[c], s);
                }
                yh[BLK][r] = s;
#pragma unroll
                for (int j = 0; j < P; ++j) Dm[BLK][r][j] = j == J[r] ? 1.0 : 0.0;
            }
        }
        ng_pseudo_obs<OBS, P, MO, BLK + 1>(y, mup, ind, th, Dm, yh, Om);
    }
}

template <class OBS, int P, int MO, int BLK>
__device__ __forceinline__ void ng_observe_block(int blk, const double (&Dm)[OBS::D][MO][P], const double (&yh)[OBS::D][MO],
                                                 const double (&Om)[OBS::D][MO][MO], double (&m)[P], double (&S)[P][P]) {
    if constexpr (BLK < OBS::D) {
        if constexpr (OBS::NACT[BLK] > 0) {
            // (dalton_observe without the forecast log-density, which DALTON's non-Gaussian form does not use)
            if (blk == BLK) observe_update<P, MO>(Dm[BLK], yh[BLK], Om[BLK], m, S);
        }
        ng_observe_block<OBS, P, MO, BLK + 1>(blk, Dm, yh, Om, m, S);
    }
}

// BOTH = true (rk_daltonng_loglik): a wave holds 32 trajectories, lanes 0..31 run their joint filters and lanes 32..63 their
// filters on Z alone; the joint filter stores its filtered moments into a.mean / a.var, the other into zm / zv.
// BOTH = false (rk_daltonng_solve): one joint lane per trajectory.  Predicted moments are not stored (re-evaluated from
// filt[n], Q, R by whoever needs them).
template <class RHS, class OBS, int P, int ITG, int MO, bool BOTH>
__global__ void __launch_bounds__(64) daltonng_fwd_kernel(SolveArgs a, NgObs o, double* __restrict__ zm, double* __restrict__ zv) {
    constexpr int D = RHS::D;
    static_assert(OBS::D == D && OBS::P == P && OBS::NTHETA == RHS::NTHETA && OBS::MO == MO,
                  "the observation model was traced for another configuration");
    const int lane = threadIdx.x;
    const bool joint = !BOTH || lane < 32;
    const int b = BOTH ? blockIdx.x * 32 + (lane & 31) : blockIdx.x * 64 + lane;
    if (b >= a.B) return;
    const size_t B = (size_t)a.B;
    double* const mean = joint ? a.mean : zm;
    double* const var = joint ? a.var : zv;
    double Q[D][P][P], R[D][P][P], W[D][P], th[RHS::NTHETA], mu[D][P], S[D][P][P];
    lane_load_model<RHS, P>(a, b, Q, R, W, th);
    lane_load_init<D, P>(a, b, mu, S);
    store_moments_all<D, P>(mean, var, B, 0, b, mu, S);                     // time 0: (ode_init, 0) (dalton.py:689-693)
    // an observation at t_min does not enter the filter (dalton.py:671); it enters logy_x
    int i = (joint && o.n_obs > 0 && o.obs_ind[0] == 0) ? 1 : 0;

    const uint32_t traj = (uint32_t)(a.traj_offset + (uint64_t)b);
    for (int n = 0; n < a.N; ++n) {
        double mup[D][P], Sp[D][P][P];
#pragma unroll
        for (int blk = 0; blk < D; ++blk) predict_block<P>(Q[blk], R[blk], mu[blk], S[blk], mup[blk], Sp[blk]);
        double wgt[D][P], am[D], V[D];
        interrogate_traj<RHS, P, ITG>(W, th, step_time(a, n), mup, Sp, a.seed, traj, (uint32_t)n, wgt, am, V);
        const bool obs_here = joint && i < o.n_obs && o.obs_ind[i] == n + 1;
        double Dm[D][MO][P], yh[D][MO], Om[D][MO][MO];
        if (obs_here) {
            double y[D][OBS::NY];
#pragma unroll
            for (int blk = 0; blk < D; ++blk)
#pragma unroll
                for (int k = 0; k < OBS::NY; ++k) y[blk][k] = o.y[((size_t)i * D + blk) * OBS::NY + k];
            ng_pseudo_obs<OBS, P, MO, 0>(y, mup, (double)i, th, Dm, yh, Om);
        }
        const size_t mstride = (size_t)D * P * B, vstride = (size_t)D * P * P * B;
        double* mo = mean + (size_t)(n + 1) * mstride + b;
        double* vo = var + (size_t)(n + 1) * vstride + b;
#pragma unroll
        for (int blk = 0; blk < D; ++blk) {
            double Wm[P];
#pragma unroll
            for (int j = 0; j < P; ++j) Wm[j] = W[blk][j] + wgt[blk][j];
            update_block_m1<P>(Wm, am[blk], V[blk], mup[blk], Sp[blk], mu[blk], S[blk]);
            if (obs_here) ng_observe_block<OBS, P, MO, 0>(blk, Dm, yh, Om, mu[blk], S[blk]);
#pragma unroll
            for (int r = 0; r < P; ++r) {                                   // store_moments, written out
                const size_t em = (size_t)blk * P + r;
                mo[em * B] = mu[blk][r];
#pragma unroll
                for (int c = 0; c < P; ++c) vo[(em * P + c) * B] = S[blk][r][c];
            }
        }
        if (obs_here) ++i;
    }
}

// eigendecomposition of a conditional variance with the rule of utils.py:60-78 (|w| <= 1e-8 dropped): the constant
// sum_kept (-log w / 2 - log 2 pi / 2) and, if asked for, the masked precision A = V diag(1 / w) V^T
template <int P, bool PREC>
__device__ __forceinline__ double ng_masked(const double (&C)[P][P], double (&A)[P][P]) {
    const double LOG_2PI = 1.83787706640934548356;
    double Aw[P][P], w[P], V[P][P], iw[P];
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) Aw[i][j] = 0.5 * (C[i][j] + C[j][i]);
    sym_eig_jacobi<P>(Aw, w, V);
    double c = 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const bool keep = !(fabs(w[k]) <= 1e-8);                            // (NaN is kept and propagates)
        c += keep ? -0.5 * (::log(w[k]) + LOG_2PI) : 0.0;     // (::log: namespace rk's own log overloads are the duals')
        iw[k] = keep ? 1.0 / w[k] : 0.0;
    }
    if constexpr (PREC) {
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int j = 0; j < P; ++j) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < P; ++k) s = fma(V[i][k] * iw[k], V[j][k], s);
                A[i][j] = s;
            }
    }
    return c;
}

// one lane per (step n = 1 .. N-1, block, trajectory): record (n - 1, blk) =
//   [G_n (P*P) | mu-_{n+1} (P) | c_n | G^Z_n (P*P) | mu^Z-_{n+1} (P) | A^Z_n (P*P) | c^Z_n]
template <int P>
__global__ void __launch_bounds__(64) daltonng_gain_kernel(SolveArgs a, NgWs w) {
    constexpr int E = ng_rec_doubles(P);
    const size_t B = (size_t)a.B;
    const size_t l = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (l >= (size_t)(a.N - 1) * a.D * B) return;
    const int b = (int)(l % B), blk = (int)((l / B) % a.D), r = (int)(l / (B * a.D));
    double Q[P][P], R[P][P];
    load_block_consts<P>(a, blk, b, Q, R);
    double* rec = bm_item(w.rec, E, B, a.D, r, blk, b);
#pragma unroll
    for (int z = 0; z < 2; ++z) {
        double mf[P], Sf[P][P], mp[P], Sp[P][P], T[P][P], G[P][P], GT[P][P], A[P][P];
        load_moments_bm<P>(z ? w.zm : w.jm, z ? w.zv : w.jv, B, a.D, r + 1, blk, b, mf, Sf);
        predict_block<P>(Q, R, mf, Sf, mp, Sp);                             // pred[n+1] re-evaluated from filt[n]
        smooth_gain<P>(Q, Sf, Sp, T, G);
        mm_nt<P, P, P>(G, T, GT);
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int j = 0; j < P; ++j) GT[i][j] = Sf[i][j] - GT[i][j];     // var_sim (standard.py:254)
        const double c = z ? ng_masked<P, true>(GT, A) : ng_masked<P, false>(GT, A);
        double* o = rec + (size_t)(z ? P * P + P + 1 : 0) * B;
#pragma unroll
        for (int i = 0; i < P; ++i) {
#pragma unroll
            for (int j = 0; j < P; ++j) o[(size_t)(i * P + j) * B] = G[i][j];
            o[(size_t)(P * P + i) * B] = mp[i];
        }
        if (z) {
#pragma unroll
            for (int i = 0; i < P; ++i)
#pragma unroll
                for (int j = 0; j < P; ++j) o[(size_t)(P * P + P + i * P + j) * B] = A[i][j];
            o[(size_t)(2 * P * P + P) * B] = c;
        } else {
            o[(size_t)(P * P + P) * B] = c;
        }
    }
}

// one lane per (trajectory, block): the smoothed-mean recursion mu_s,n = mu_f,n + G_n (mu_s,n+1 - mu-_{n+1}) backwards from
// mu_f,N, the log-density of every smoothed mean under the Z filter's conditional, the constants of the joint filter's
// conditionals (their quadratic forms are dropped: the smoothed mean IS the conditional's mean, dalton.py:732-753), both
// terminal terms, and the smoothed means at the observations' grid indices.
template <int P>
__global__ void __launch_bounds__(64) daltonng_chain_kernel(SolveArgs a, NgWs w, NgObs o) {
    constexpr int E = ng_rec_doubles(P);
    const int l = blockIdx.x * 64 + threadIdx.x;
    if (l >= a.B * a.D) return;
    const int blk = l / a.B, b = l - blk * a.B;
    const size_t B = (size_t)a.B;
    double ms[P], Sf[P][P], mz[P], Sz[P][P], A[P][P];
    load_moments_bm<P>(w.jm, w.jv, B, a.D, a.N, blk, b, ms, Sf);
    load_moments_bm<P>(w.zm, w.zv, B, a.D, a.N, blk, b, mz, Sz);
    double acc_y = ng_masked<P, false>(Sf, A);                              // logpdf(mu_f,N; mu_f,N, Sigma_f,N)
    double acc_z = ng_masked<P, true>(Sz, A);                               // logpdf(mu_s,N; mu^Z_f,N, Sigma^Z_f,N)
    {
        double rr[P], Ar[P];
#pragma unroll
        for (int i = 0; i < P; ++i) rr[i] = ms[i] - mz[i];
        mv<P, P>(A, rr, Ar);
        acc_z += -0.5 * dot<P>(rr, Ar);
    }
    int i = o.n_obs - 1;
    auto keep = [&](int slot, const double (&m)[P]) {
        double* so = bm_item(w.sm, P, B, a.D, slot, blk, b);
#pragma unroll
        for (int e = 0; e < P; ++e) so[(size_t)e * B] = m[e];
    };
    if (i >= 0 && o.obs_ind[i] == a.N) { keep(i, ms); --i; }
    for (int n = a.N - 1; n >= 1; --n) {
        const double* rec = bm_item(w.rec, E, B, a.D, n - 1, blk, b);
        const double* mfp = bm_item(w.jm, P, B, a.D, n, blk, b);
        const double* mzp = bm_item(w.zm, P, B, a.D, n, blk, b);
        double G[P][P], GZ[P][P], d[P], dz[P], gm[P], gz[P], rr[P], Ar[P];
#pragma unroll
        for (int r = 0; r < P; ++r) {
#pragma unroll
            for (int c = 0; c < P; ++c) {
                G[r][c] = rec[(size_t)(r * P + c) * B];
                GZ[r][c] = rec[(size_t)(P * P + P + 1 + r * P + c) * B];
                A[r][c] = rec[(size_t)(2 * P * P + 2 * P + 1 + r * P + c) * B];
            }
            d[r] = ms[r] - rec[(size_t)(P * P + r) * B];
            dz[r] = ms[r] - rec[(size_t)(2 * P * P + P + 1 + r) * B];
        }
        mv<P, P>(G, d, gm);
        mv<P, P>(GZ, dz, gz);
#pragma unroll
        for (int r = 0; r < P; ++r) {
            ms[r] = mfp[(size_t)r * B] + gm[r];                             // standard.py:213
            rr[r] = ms[r] - (mzp[(size_t)r * B] + gz[r]);                   // standard.py:251
        }
        mv<P, P>(A, rr, Ar);
        acc_z += -0.5 * dot<P>(rr, Ar) + rec[(size_t)(3 * P * P + 2 * P + 1) * B];
        acc_y += rec[(size_t)(P * P + P) * B];
        if (i >= 0 && o.obs_ind[i] == n) { keep(i, ms); --i; }
    }
    if (i >= 0 && o.obs_ind[i] == 0) {
        double m0[P];
#pragma unroll
        for (int e = 0; e < P; ++e) m0[e] = ld(a.x0, (size_t)blk * P + e, a.x0_b, a.B, b);
        keep(i, m0);
    }
    w.part[(size_t)blk * B + b] = acc_z;
    w.part[((size_t)a.D + blk) * B + b] = acc_y;
}

// logy_x = sum_i loglik(y_i, smoothed mean at the grid index of observation i) on plain doubles, in the order of i, and
// the value logy_x + logx_z - logx_yhat (dalton.py:949) with the blocks summed in order: identical bits from call to call
template <class OBS>
__global__ void __launch_bounds__(64) daltonng_obs_kernel(int B_, int n_obs, const double* __restrict__ y,
                                                          const double* __restrict__ sm, const double* __restrict__ theta,
                                                          int theta_b, const double* __restrict__ part, double* __restrict__ out) {
    constexpr int D = OBS::D, P = OBS::P, NY = OBS::NY;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B_) return;
    const size_t B = (size_t)B_;
    double th[OBS::NTHETA];
#pragma unroll
    for (int k = 0; k < OBS::NTHETA; ++k) th[k] = theta ? ld(theta, k, theta_b, B_, b) : 0.0;
    double logy = 0.0;
    for (int i = 0; i < n_obs; ++i) {
        double X[D][P], yy[D][NY];
#pragma unroll
        for (int blk = 0; blk < D; ++blk) {
#pragma unroll
            for (int e = 0; e < P; ++e) X[blk][e] = sm[(((size_t)i * D + blk) * P + e) * B + b];
#pragma unroll
            for (int k = 0; k < NY; ++k) yy[blk][k] = y[((size_t)i * D + blk) * NY + k];
        }
        logy += OBS::template loglik<double>(yy, X, (double)i, th);
    }
    double lz = 0.0, ly = 0.0;
#pragma unroll
    for (int blk = 0; blk < D; ++blk) {
        lz += part[(size_t)blk * B + b];
        ly += part[((size_t)D + blk) * B + b];
    }
    out[b] = logy + lz - ly;
}

}  // namespace rk
