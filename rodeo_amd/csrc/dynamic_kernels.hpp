// solve_mv_dynamic / solve_sim_dynamic: the solver with a per-step calibrated prior scale (an addition; DESIGN.md section 7
// (13)), the forward lane kernel and the pieces it shares with the backward kernels of dynamic.hip.  Shared by the
// ahead-of-time build (dynamic.hip, built-in right-hand sides) and the hiprtc build for user-supplied right-hand sides
// (rhs_jit.hip, its dynamic kind only).  RTC-safe: no host code.
//
// Step n -> n + 1 of block b, from the filtered (mu, Sigma):
//   mu- = Q mu,  P = Q Sigma Q^T                              (no R yet)
//   W~ = W + wgt_meas, a = mean_meas: the interrogation at mu- (schober and kramer need no variance; rodeo's comes below)
//   z = 0 - (W~ mu- + a),  r = W~ R W~^T,  c = max(z^2 / r, scale_min)
//   Sigma- = P + c R;  var_meas V = W Sigma- W^T under rodeo, 0 under schober and kramer
//   s = W~ Sigma- W~^T + V and the usual update;  scale[n, b] = c, quad_b += z^2 / s, logdet_b += log s
// The backward kernels re-evaluate Sigma-_{n+1} = Q Sigma_f[n] Q^T + scale[n] R with the two functions below, the forward
// kernel's own expressions.  A step with z = 0 exactly and scale_min = 0 has c = 0, hence s = 0: inf / NaN as the arithmetic
// produces them, like solve_evidence's s.
// Outputs next to the batch-minor moments: scale (N, n_block, B), element [(n * n_block + blk) * B + b]; logdens (B).
#pragma once
#include "rk_enums.hpp"
#include "kalman_small.hpp"
#include "philox.hpp"
#include "solve_args.hpp"
#include "solve_small_kernels.hpp"
#include "evidence_kernels.hpp"

namespace rk {

// standard.py:57-59 without the noise term:  mu- = Q mu ;  P = (Q Sigma) Q^T   (predict_block's products, in its order)
template <int P>
__device__ __forceinline__ void dynamic_propagate(const double (&Q)[P][P], const double (&mu)[P], const double (&S)[P][P],
                                                  double (&mup)[P], double (&Pp)[P][P]) {
    mv<P, P>(Q, mu, mup);
    double A[P][P];
    mm<P, P, P>(Q, S, A);
    mm_nt<P, P, P>(A, Q, Pp);
}

// Sigma- = P + c R
template <int P>
__device__ __forceinline__ void dynamic_add_noise(const double (&Pp)[P][P], double c, const double (&R)[P][P],
                                                  double (&Sp)[P][P]) {
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) Sp[i][j] = fma(c, R[i][j], Pp[i][j]);
}

// w M w^T of a row vector
template <int P>
__device__ __forceinline__ double dynamic_quadform(const double (&w)[P], const double (&M)[P][P]) {
    double wM[P];
    row_mat<P>(w, M, wM);
    return dot<P>(wM, w);
}

// forward pass, one lane per trajectory (fwd_kernel's layout and stores; evidence_kernel's sums)
template <class RHS, int P, int ITG>
__global__ void __launch_bounds__(64) dynamic_fwd_kernel(SolveArgs a, double scale_min, double* __restrict__ scale,
                                                         double* __restrict__ logdens) {
    constexpr int D = RHS::D;
    static_assert(ITG != RK_INTERROGATE_CHKREBTII, "dynamic: interrogate_chkrebtii is not served (its point is drawn from the "
                                                   "predicted variance, which here depends on the point)");
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const size_t B = (size_t)a.B;
    double Q[D][P][P], R[D][P][P], W[D][P], th[RHS::NTHETA], mu[D][P], S[D][P][P], q[D] = {};
    LogProd l[D];
    lane_load_model<RHS, P>(a, b, Q, R, W, th);
    lane_load_init<D, P>(a, b, mu, S);
    store_moments_all<D, P>(a.mean, a.var, B, 0, b, mu, S);                                   // time index 0
    const uint32_t traj = (uint32_t)(a.traj_offset + (uint64_t)b);
    for (int n = 0; n < a.N; ++n) {
        double mup[D][P], Sp[D][P][P];
#pragma unroll
        for (int blk = 0; blk < D; ++blk) dynamic_propagate<P>(Q[blk], mu[blk], S[blk], mup[blk], Sp[blk]);
        double wgt[D][P], am[D], V[D];
        // (Sp holds P here: of the three served interrogations only rodeo reads it, for a var_meas that is formed below instead)
        interrogate_traj<RHS, P, ITG>(W, th, step_time(a, n), mup, Sp, a.seed, traj, (uint32_t)n, wgt, am, V);
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
            *bm_item(scale, 1, B, D, n, blk, b) = c;
            store_moments<P>(a.mean, a.var, B, D, n + 1, blk, b, mu[blk], S[blk]);
        }
    }
    double tot = 0.0;
#pragma unroll
    for (int blk = 0; blk < D; ++blk) tot += q[blk] + l[blk].log();
    logdens[b] = evidence_logdens(tot, D, a.N);
}

}  // namespace rk
