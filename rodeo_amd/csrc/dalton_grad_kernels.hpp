// dalton_grid_jvp / dalton_grid_grad / dalton_grad (an addition): directional derivatives of
// dalton_grid's log p(Y | Z) = joint - marginal with respect to the ODE parameters and the initial state, forward mode, one
// tangent direction per lane.  RTC-safe: no host code.
//
// The primal filter is dalton_grid_fwd_kernel's log-likelihood form (dalton_grid_kernels.hpp), helper for helper: grid_walk,
// predict_block, interrogate_traj, dalton_update_z, dalton_observe, and its observation schedule.  Next to (mu, Sigma) a lane
// carries (mu., Sigma.), the exact derivative of those formulas as they are computed (the update is one-sided and is
// differentiated as such):
//   predict        mu.- = Q mu. ;  Sigma.- = Q Sigma. Q^T                      (the pair does not depend on the parameters)
//   interrogation  x. = the tangent of the whole predicted mean, all blocks:
//       rodeo / schober   a. = -(df/dx x. + df/dtheta theta.) ;  V. = W Sigma.- W^T (rodeo), 0 (schober)
//       kramer            J. = d/de J(mu- + e x., theta + e theta.) ;  wgt. = -J. ;  a. = -f. + J. mu- + J mu.-
//   update         WS = W~ Sigma-, SW = Sigma- W~^T, s = WS W~ + V, innov = -(W~ mu- + a), K = SW / s, the product rule through
//                  all of them; the log-density term -1/2 (innov^2 / s + log s) has the derivative
//                  -innov innov. / s + 1/2 innov^2 s. / s^2 - 1/2 s. / s, and nothing where the value drops the term (|s| <= 1e-8)
//   y update       the same with the constant row D and the variance Omega (n_bobs = 1)
//   node 0         log N(y_0; D_0 x_0, Omega_0) differentiated in x_0; nothing is updated
// The marginal filter is the same recursion without y; dvalue = d(joint) - d(marginal).
//
// The hyper form (dalton_grid_jvp_hyper_kernel) adds two directions per block: l. = the rate of
// log sigma_b, under the scale law R_b ~ sigma_b^2 with Q free of it, and w. = the rate of a common log-scale of block b's
// observation variances:
//   predict        Sigma.- = Q Sigma. Q^T + 2 l. R     (the step's own R as it is loaded; the initial variance is not scaled)
//   y update       Omega. = w. Omega                    (node 0 included: -1/2 w. + 1/2 innov^2 w. / Omega)
// All three kernel pairs of the gradient family (this one, fenrir_grad_kernels.hpp's and fenrir_grad.hip's) stay written out, two
// kernels each on the same device functions.  As one `__device__
// __forceinline__` body under `if constexpr (HYPER)` behind two one-line kernels, 23 of this pair's 24 instances keep their
// registers, scratch 0 and fp64 instruction counts, and dalton_grid_jvp_hyper_kernel<Lorenz63, 3, rodeo>, which uses all 512
// registers, spills 12 B per lane: with by-value and with by-reference parameters, with and without __restrict__ on the body, and
// with the rates loaded in a loop of their own.  The Fenrir pairs kept their resources as one body and ran slower (DESIGN.md
// section 7 (26)).
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

namespace rk {

// Adapter: a struct with the scalar-generic `rhs_generic<T, TH, P>` alone (rodeo_amd.trace.trace_grad_source) -> a complete
// right-hand side: f and fjac through AutoJac (dual.hpp) on plain-double parameters, rhs_generic as it is.
template <class U>
struct GenericAsRhs {
    static constexpr int D = U::D, NTHETA = U::NTHETA, NDEP = U::NDEP;
    template <class T, int P>
    __device__ __forceinline__ static void rhs(const T (&X)[D][P], double t, const double (&th)[NTHETA], T (&out)[D]) {
        U::template rhs_generic<T, double, P>(X, t, th, out);
    }
};
template <class U>
struct AutoJacG : AutoJac<GenericAsRhs<U>> {
    template <class T, class TH, int P>
    __device__ __forceinline__ static void rhs_generic(const T (&X)[U::D][P], double t, const TH (&th)[U::NTHETA], T (&out)[U::D]) {
        U::template rhs_generic<T, TH, P>(X, t, th, out);
    }
};

// the K directions of rk_dalton_grid_jvp, batch-minor: dtheta (K, NTHETA[, B]), dinit (K, D, P[, B]); null: zero directions
struct JvpDirs {
    const double *dtheta, *dinit;
    int dtheta_b, dinit_b;
    int K;
};

// the hyper directions of rk_dalton_grid_jvp_hyper / rk_fenrir_grid_jvp_hyper, batch-minor like dtheta: dlog_sigma and dlog_obs_var
// (K, D[, B]); null: zero directions.  A struct of its own, for the hyper kernels only: JvpDirs travels by value into the others.
struct JvpHyper {
    const double *dlsig, *dlobs;
    int dlsig_b, dlobs_b;
};

// one rate of direction k, block blk, trajectory b, from dlsig or dlobs
__device__ __forceinline__ double hyper_rate(const double* v, int batched, int D, int k, int blk, int B, int b) {
    return v ? ld(v, (size_t)k * D + blk, batched, B, b) : 0.0;
}

// Sigma.- += 2 l. R: the prior scale's share of the predicted variance's tangent
template <int P>
__device__ __forceinline__ void jvp_predict_scale(const double (&R)[P][P], double dlsig, double (&dSp)[P][P]) {
    const double r2 = 2.0 * dlsig;
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) dSp[i][j] = fma(r2, R[i][j], dSp[i][j]);
}

// mu.- = Q mu. ;  Sigma.- = (Q Sigma.) Q^T
template <int P>
__device__ __forceinline__ void jvp_predict_block(const double (&Q)[P][P], const double (&dmu)[P], const double (&dS)[P][P],
                                                  double (&dmup)[P], double (&dSp)[P][P]) {
    mv<P, P>(Q, dmu, dmup);
    double A[P][P];
    mm<P, P, P>(Q, dS, A);
    mm_nt<P, P, P>(A, Q, dSp);
}

// The tangent of interrogate_traj's (wgt, a, V) along (x. = dmup, theta. = dth) at the predicted mean; `wgt` is the primal
// weight it returned (kramer: -J).
template <class RHS, int P, int ITG>
__device__ __forceinline__ void jvp_interrogate(const double (&W)[RHS::D][P], const double (&th)[RHS::NTHETA],
                                                const double (&dth)[RHS::NTHETA], double t, const double (&mup)[RHS::D][P],
                                                const double (&dmup)[RHS::D][P], const double (&dSp)[RHS::D][P][P],
                                                const double (&wgt)[RHS::D][P], double (&dwgt)[RHS::D][P], double (&da)[RHS::D],
                                                double (&dV)[RHS::D]) {
    constexpr int D = RHS::D, NT = RHS::NTHETA;
    static_assert(ITG == RK_INTERROGATE_RODEO || ITG == RK_INTERROGATE_SCHOBER || ITG == RK_INTERROGATE_KRAMER,
                  "the gradient kernels serve rodeo, schober and kramer");
    Tangent tht[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) tht[k] = Tangent(th[k], dth[k]);
    if constexpr (ITG == RK_INTERROGATE_KRAMER) {
        constexpr int ND = RHS::NDEP < P ? RHS::NDEP : P;                    // f reads the first NDEP entries of a block
#pragma unroll
        for (int blk = 0; blk < D; ++blk) {
            TJet<ND> X[D][P], out[D];
#pragma unroll
            for (int bb = 0; bb < D; ++bb)
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    X[bb][j] = TJet<ND>(Tangent(mup[bb][j], dmup[bb][j]));
                    if (bb == blk && j < ND) X[bb][j].d[j] = Tangent(1.0);
                }
            RHS::template rhs_generic<TJet<ND>, Tangent, P>(X, t, tht, out);
            double acc = -out[blk].v.d;                                      // -f.
#pragma unroll
            for (int j = 0; j < P; ++j) {
                if (j < ND) {
                    const double dJ = out[blk].d[j].d;
                    dwgt[blk][j] = -dJ;
                    acc = fma(dJ, mup[blk][j], acc);                        // + J. mu-
                    acc = fma(-wgt[blk][j], dmup[blk][j], acc);             // + J mu.-   (J = -wgt)
                } else {
                    dwgt[blk][j] = 0.0;
                }
            }
            da[blk] = acc;
            dV[blk] = 0.0;
        }
    } else {
        Tangent X[D][P], out[D];
#pragma unroll
        for (int bb = 0; bb < D; ++bb)
#pragma unroll
            for (int j = 0; j < P; ++j) X[bb][j] = Tangent(mup[bb][j], dmup[bb][j]);
        RHS::template rhs_generic<Tangent, Tangent, P>(X, t, tht, out);
#pragma unroll
        for (int blk = 0; blk < D; ++blk) {
            da[blk] = -out[blk].d;
#pragma unroll
            for (int j = 0; j < P; ++j) dwgt[blk][j] = 0.0;
            if constexpr (ITG == RK_INTERROGATE_SCHOBER) {
                dV[blk] = 0.0;
            } else {
                double WS[P];
                row_mat<P>(W[blk], dSp[blk], WS);
                dV[blk] = dot<P>(WS, W[blk]);
            }
        }
    }
}

// The tangent of update_z<P, GAIN_DIVIDE> and of the log-density term it shares its forecast variance with: the measurement
// 0 = W x + a + N(0, V) with tangents (dW, da, dV), at the predicted (mp, Sp) with tangents (dmp, dSp).  DW = false: dW is zero
// and not read.  The primal quantities are recomputed by update_z's own expressions.
template <int P, bool DW>
__device__ __forceinline__ void jvp_update(const double (&W)[P], const double (&dW)[P], double a, double da, double V, double dV,
                                           const double (&mp)[P], const double (&Sp)[P][P], const double (&dmp)[P],
                                           const double (&dSp)[P][P], double (&dm)[P], double (&dS)[P][P], double& dacc) {
    double WS[P], SW[P], dWS[P], dSW[P];
    row_mat<P>(W, Sp, WS);
    const double s = dot<P>(WS, W) + V;
    const double innov = 0.0 - (dot<P>(W, mp) + a);
    row_mat<P>(W, dSp, dWS);
    double ds = dot<P>(dWS, W) + dV;
    double dinnov = -(dot<P>(W, dmp) + da);
#pragma unroll
    for (int i = 0; i < P; ++i) {
        SW[i] = dot<P>(Sp[i], W);
        dSW[i] = dot<P>(dSp[i], W);
    }
    if constexpr (DW) {
        double t1[P];
        row_mat<P>(dW, Sp, t1);
#pragma unroll
        for (int j = 0; j < P; ++j) dWS[j] += t1[j];
        ds += dot<P>(t1, W) + dot<P>(WS, dW);
        dinnov -= dot<P>(dW, mp);
#pragma unroll
        for (int i = 0; i < P; ++i) dSW[i] += dot<P>(Sp[i], dW);
    }
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const double K = SW[i] / s;
        const double dK = (dSW[i] - K * ds) / s;
        dm[i] = dmp[i] + dK * innov + K * dinnov;
#pragma unroll
        for (int j = 0; j < P; ++j) dS[i][j] = dSp[i][j] - dK * WS[j] - K * dWS[j];
    }
    if (fabs(s) > 1e-8) dacc += -innov * dinnov / s + 0.5 * innov * innov * ds / (s * s) - 0.5 * ds / s;
}

// the tangent of dalton_observe<P, 1> on observation row ib, in place on (dm, dS); called BEFORE the primal update of (m, S)
template <int P>
__device__ __forceinline__ void jvp_observe(const DaltonObs& o, size_t ib, const double (&m)[P], const double (&S)[P][P],
                                            double (&dm)[P], double (&dS)[P][P], double& dacc) {
    double Drow[P], dm2[P], dS2[P][P];
#pragma unroll
    for (int k = 0; k < P; ++k) Drow[k] = o.obs_w[ib * P + k];
    jvp_update<P, false>(Drow, Drow, -o.obs[ib], 0.0, o.obs_v[ib], 0.0, m, S, dm, dS, dm2, dS2, dacc);
#pragma unroll
    for (int i = 0; i < P; ++i) {
        dm[i] = dm2[i];
#pragma unroll
        for (int j = 0; j < P; ++j) dS[i][j] = dS2[i][j];
    }
}

// The same where the variance has the tangent Omega. = rate Omega (the hyper kernels).  Its own few lines: with jvp_observe written
// as the rate-0 case of this one, the compiler orders that function's loads differently, and dalton_grid_jvp_kernel's code with them.
template <int P>
__device__ __forceinline__ void jvp_observe_rate(const DaltonObs& o, size_t ib, double rate, const double (&m)[P],
                                                 const double (&S)[P][P], double (&dm)[P], double (&dS)[P][P], double& dacc) {
    double Drow[P], dm2[P], dS2[P][P];
#pragma unroll
    for (int k = 0; k < P; ++k) Drow[k] = o.obs_w[ib * P + k];
    const double V = o.obs_v[ib];
    jvp_update<P, false>(Drow, Drow, -o.obs[ib], 0.0, V, rate * V, m, S, dm, dS, dm2, dS2, dacc);
#pragma unroll
    for (int i = 0; i < P; ++i) {
        dm[i] = dm2[i];
#pragma unroll
        for (int j = 0; j < P; ++j) dS[i][j] = dS2[i][j];
    }
}

// Work item = (trajectory b, direction k), B K items; a wave holds 32: lanes 0..31 run the items' joint filters, lanes 32..63
// their marginal filters (dalton_grid_fwd_kernel's halves).  A lane recomputes its trajectory's primal filter and carries one
// tangent.  dvalue[b K + k] = d(joint) - d(marginal) and, from the k = 0 item, value[b] = joint - marginal leave through one
// cross-lane read each: one writer per element, no atomics.  A lane past B K runs on the last item only where grid_walk needs
// the whole wave, and stores nothing.  n_bobs = 1.
template <class RHS, int P, int ITG>
__global__ void __launch_bounds__(64) dalton_grid_jvp_kernel(SolveArgs a, DaltonObs o, GridArgs g, JvpDirs dir,
                                                             double* __restrict__ value, double* __restrict__ dvalue) {
    constexpr int D = RHS::D, NT = RHS::NTHETA;
    const int lane = threadIdx.x;
    const bool joint = lane < 32;
    const long long n_items = (long long)a.B * dir.K;
    const long long lane_item = (long long)blockIdx.x * 32 + (lane & 31);
    const bool live = lane_item < n_items;
    const long long item = live ? lane_item : n_items - 1;                  // (a lane past B K reads an item that exists)
    const int b = (int)(item / dir.K), k = (int)(item % dir.K);
    double acc = 0.0, dacc = 0.0;
    if (live || grid_walk_needs_helpers<RHS, P>(g)) {
        double W[D][P], th[NT], dth[NT], mu[D][P], S[D][P][P], dmu[D][P], dS[D][P][P];
        {
            double Q0[D][P][P], R0[D][P][P];
            lane_load_model<RHS, P>(a, b, Q0, R0, W, th);                   // W and theta: the plan's own pair is not read
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
        // an observation on node 0 adds log p(y_0 | x_0) to the joint density and does not update x_0 (dalton_grid_fwd_kernel)
        int i = 0;
        if (o.n_obs > 0 && o.obs_ind[0] == 0) {
            if (joint) {
#pragma unroll
                for (int blk = 0; blk < D; ++blk) {
                    double m0[P], S0[P][P], dm0[P], dS0[P][P];
#pragma unroll
                    for (int r = 0; r < P; ++r) {
                        m0[r] = mu[blk][r];
                        dm0[r] = dmu[blk][r];
#pragma unroll
                        for (int c = 0; c < P; ++c) S0[r][c] = dS0[r][c] = 0.0;
                    }
                    jvp_observe<P>(o, (size_t)blk, m0, S0, dm0, dS0, dacc);
                    dalton_observe<P, 1>(o, (size_t)blk, m0, S0, acc);
                }
            }
            i = 1;
        }
        int obs_node = i < o.n_obs ? o.obs_ind[i] : -1;                     // node of observation i; -1: none left

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
            const bool obs_here = obs_node == n + 1;                        // (the same in every lane of the wave)
#pragma unroll
            for (int blk = 0; blk < D; ++blk) {
                double Wm[P];
#pragma unroll
                for (int j = 0; j < P; ++j) Wm[j] = W[blk][j] + wgt[blk][j];
                jvp_update<P, ITG == RK_INTERROGATE_KRAMER>(Wm, dwgt[blk], am[blk], dam[blk], V[blk], dV[blk], mup[blk], Sp[blk],
                                                            dmup[blk], dSp[blk], dmu[blk], dS[blk], dacc);
                dalton_update_z<P>(Wm, am[blk], V[blk], mup[blk], Sp[blk], mu[blk], S[blk], acc);
                if (obs_here && joint) {
                    jvp_observe<P>(o, (size_t)i * D + blk, mu[blk], S[blk], dmu[blk], dS[blk], dacc);
                    dalton_observe<P, 1>(o, (size_t)i * D + blk, mu[blk], S[blk], acc);
                }
            }
            if (obs_here) {
                ++i;
                obs_node = i < o.n_obs ? o.obs_ind[i] : -1;
                asm volatile("" : "+v"(obs_node));                          // (dalton_grid_fwd_kernel: waited for on the rare path)
            }
        });
    }
    const double marg = __shfl_down(acc, 32, 64), dmarg = __shfl_down(dacc, 32, 64);     // lane l < 32 reads lane l + 32
    if (joint && live) {
        dvalue[lane_item] = dacc - dmarg;
        if (k == 0) value[b] = acc - marg;
    }
}

// The hyper form: dalton_grid_jvp_kernel's items, lanes, walk and exits, with the rates l.[D] of log sigma and w.[D] of the
// observation variances' log-scale of the item's direction in registers (2 D doubles): jvp_predict_scale after every
// jvp_predict_block, in both filters, and jvp_observe_rate where that kernel has jvp_observe.
template <class RHS, int P, int ITG>
__global__ void __launch_bounds__(64) dalton_grid_jvp_hyper_kernel(SolveArgs a, DaltonObs o, GridArgs g, JvpDirs dir, JvpHyper hy,
                                                                   double* __restrict__ value, double* __restrict__ dvalue) {
    constexpr int D = RHS::D, NT = RHS::NTHETA;
    const int lane = threadIdx.x;
    const bool joint = lane < 32;
    const long long n_items = (long long)a.B * dir.K;
    const long long lane_item = (long long)blockIdx.x * 32 + (lane & 31);
    const bool live = lane_item < n_items;
    const long long item = live ? lane_item : n_items - 1;                  // (a lane past B K reads an item that exists)
    const int b = (int)(item / dir.K), k = (int)(item % dir.K);
    double acc = 0.0, dacc = 0.0;
    if (live || grid_walk_needs_helpers<RHS, P>(g)) {
        double W[D][P], th[NT], dth[NT], mu[D][P], S[D][P][P], dmu[D][P], dS[D][P][P], dls[D], dlo[D];
        {
            double Q0[D][P][P], R0[D][P][P];
            lane_load_model<RHS, P>(a, b, Q0, R0, W, th);                   // W and theta: the plan's own pair is not read
        }
        lane_load_init<D, P>(a, b, mu, S);
#pragma unroll
        for (int j = 0; j < NT; ++j) dth[j] = dir.dtheta ? ld(dir.dtheta, (size_t)k * NT + j, dir.dtheta_b, a.B, b) : 0.0;
#pragma unroll
        for (int blk = 0; blk < D; ++blk) {
            dls[blk] = hyper_rate(hy.dlsig, hy.dlsig_b, D, k, blk, a.B, b);
            dlo[blk] = hyper_rate(hy.dlobs, hy.dlobs_b, D, k, blk, a.B, b);
#pragma unroll
            for (int r = 0; r < P; ++r) {
                dmu[blk][r] = dir.dinit ? ld(dir.dinit, ((size_t)k * D + blk) * P + r, dir.dinit_b, a.B, b) : 0.0;
#pragma unroll
                for (int c = 0; c < P; ++c) dS[blk][r][c] = 0.0;
            }
        }
        // node 0: log p(y_0 | x_0) with Omega. = w. Omega; nothing is updated
        int i = 0;
        if (o.n_obs > 0 && o.obs_ind[0] == 0) {
            if (joint) {
#pragma unroll
                for (int blk = 0; blk < D; ++blk) {
                    double m0[P], S0[P][P], dm0[P], dS0[P][P];
#pragma unroll
                    for (int r = 0; r < P; ++r) {
                        m0[r] = mu[blk][r];
                        dm0[r] = dmu[blk][r];
#pragma unroll
                        for (int c = 0; c < P; ++c) S0[r][c] = dS0[r][c] = 0.0;
                    }
                    jvp_observe_rate<P>(o, (size_t)blk, dlo[blk], m0, S0, dm0, dS0, dacc);
                    dalton_observe<P, 1>(o, (size_t)blk, m0, S0, acc);
                }
            }
            i = 1;
        }
        int obs_node = i < o.n_obs ? o.obs_ind[i] : -1;                     // node of observation i; -1: none left

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
            const bool obs_here = obs_node == n + 1;                        // (the same in every lane of the wave)
#pragma unroll
            for (int blk = 0; blk < D; ++blk) {
                double Wm[P];
#pragma unroll
                for (int j = 0; j < P; ++j) Wm[j] = W[blk][j] + wgt[blk][j];
                jvp_update<P, ITG == RK_INTERROGATE_KRAMER>(Wm, dwgt[blk], am[blk], dam[blk], V[blk], dV[blk], mup[blk], Sp[blk],
                                                            dmup[blk], dSp[blk], dmu[blk], dS[blk], dacc);
                dalton_update_z<P>(Wm, am[blk], V[blk], mup[blk], Sp[blk], mu[blk], S[blk], acc);
                if (obs_here && joint) {
                    jvp_observe_rate<P>(o, (size_t)i * D + blk, dlo[blk], mu[blk], S[blk], dmu[blk], dS[blk], dacc);
                    dalton_observe<P, 1>(o, (size_t)i * D + blk, mu[blk], S[blk], acc);
                }
            }
            if (obs_here) {
                ++i;
                obs_node = i < o.n_obs ? o.obs_ind[i] : -1;
                asm volatile("" : "+v"(obs_node));                          // (dalton_grid_jvp_kernel: waited for on the rare path)
            }
        });
    }
    const double marg = __shfl_down(acc, 32, 64), dmarg = __shfl_down(dacc, 32, 64);     // lane l < 32 reads lane l + 32
    if (joint && live) {
        dvalue[lane_item] = dacc - dmarg;
        if (k == 0) value[b] = acc - marg;
    }
}

}  // namespace rk
