// DALTON for Gaussian observations (src/rodeo/inference/dalton.py:39-545), lane-per-trajectory forward filters.
// Shared by the ahead-of-time build (dalton.hip, built-in right-hand sides) and by the hiprtc build for user-supplied
// right-hand sides (rhs_jit.hip, its DALTON kinds only).  RTC-safe: no host code.
//
// The joint filter of (Z, Y) is fwd_kernel's filter (solve_small_kernels.hpp) whose z update also accumulates the forecast
// log-density, and which conditions on y_i = D_i X + N(0, Omega_i) at the grid index of observation i.  The reference stacks
// [W~; D_i] into one measurement (dalton.py:136-149); here y is conditioned on after z (sequential conditioning): the same
// log-density and update up to rounding, unless a forecast variance lies within utils.py:60-78's 1e-8 threshold
// (DESIGN.md section 7).  The marginal filter of Z is the same recursion without observations.
#pragma once
#include "rk_enums.hpp"
#include "kalman_small.hpp"
#include "philox.hpp"
#include "solve_args.hpp"
#include "solve_small_kernels.hpp"

namespace rk {

// observations of rk_dalton_*: obs (n_obs, D, MO), obs_w (n_obs, D, MO, P), obs_v (n_obs, D, MO, MO), obs_ind (n_obs)
struct DaltonObs {
    const double *obs, *obs_w, *obs_v;
    const int32_t* obs_ind;
    int n_obs;
};

// forecast, log-density (utils.py:60-78: eigenvalues with |w| <= 1e-8 dropped) and update (standard.py:93-102, LU) of one
// block with observation row ib = i * D + blk; fenrir_bwd_kernel's observe() (solve_small.hip) as a function
template <int P, int MO>
__device__ __forceinline__ void dalton_observe(const DaltonObs& o, size_t ib, double (&m)[P], double (&S)[P][P], double& acc) {
    const double LOG_2PI = 1.83787706640934548356;
    double D[MO][P], y[MO], Om[MO][MO], Wf[MO][MO], DS[MO][P], z[MO];
#pragma unroll
    for (int j = 0; j < MO; ++j) {
        y[j] = o.obs[ib * MO + j];
#pragma unroll
        for (int k = 0; k < P; ++k) D[j][k] = o.obs_w[(ib * MO + j) * P + k];
#pragma unroll
        for (int l = 0; l < MO; ++l) Om[j][l] = o.obs_v[(ib * MO + j) * MO + l];
    }
    observe_forecast<P, MO>(D, y, Om, m, S, z, DS, Wf);
    if constexpr (MO == 1) {
        if (fabs(Wf[0][0]) > 1e-8) acc += -0.5 * (z[0] * z[0] / Wf[0][0] + log(Wf[0][0])) - 0.5 * LOG_2PI;
    } else {
        double Aw[MO][MO], w[MO], V[MO][MO];
#pragma unroll
        for (int j = 0; j < MO; ++j)
#pragma unroll
            for (int l = 0; l < MO; ++l) Aw[j][l] = 0.5 * (Wf[j][l] + Wf[l][j]);
        sym_eig_jacobi<MO>(Aw, w, V);
#pragma unroll
        for (int k = 0; k < MO; ++k) {
            double zk = 0.0;
#pragma unroll
            for (int j = 0; j < MO; ++j) zk = fma(V[j][k], z[j], zk);
            if (fabs(w[k]) > 1e-8) acc += -0.5 * (zk * zk / w[k] + log(w[k])) - 0.5 * LOG_2PI;
        }
    }
    observe_apply<P, MO>(D, z, DS, Wf, m, S);
}

// z forecast, log-density and update of one block (x_meas = 0, n_bmeas = 1): update_z with a division per gain element,
// whose forecast variance the log-density shares
template <int P>
__device__ __forceinline__ void dalton_update_z(const double (&Wm)[P], double am, double V, const double (&mup)[P],
                                                const double (&Sp)[P][P], double (&mu)[P], double (&S)[P][P], double& acc) {
    const double LOG_2PI = 1.83787706640934548356;
    double innov, s;
    update_z<P, GAIN_DIVIDE>(Wm, am, V, mup, Sp, mu, S, innov, s);
    if (fabs(s) > 1e-8) acc += -0.5 * (innov * innov / s + log(s)) - 0.5 * LOG_2PI;
}

// the end of the two-filters-per-wave kernels: lane l < 32 holds trajectory b's joint sum, lane l + 32 its marginal one
__device__ __forceinline__ void store_joint_minus_marginal(double acc, int lane, int b, int B, double* logdens) {
    const double marg = __shfl_down(acc, 32, 64);                         // lane l < 32 reads lane l + 32
    if (lane < 32 && b < B) logdens[b] = acc - marg;
}

// STORE = false (log-likelihood): a wave holds 32 trajectories, lanes 0..31 run their joint filters and lanes 32..63 their
// marginal filters; logdens[b] = joint - marginal leaves through one cross-lane read, nothing else is stored.
// STORE = true (rk_dalton_solve): one lane per trajectory runs the joint filter (dalton.py:242-371) and writes the
// batch-minor filtered moments (+ the predicted ones when a.mean_pred is set) that bwd_mv_kernel / bwd_sim_kernel read.
template <class RHS, int P, int ITG, int MO, bool STORE>
__global__ void __launch_bounds__(64) dalton_fwd_kernel(SolveArgs a, DaltonObs o, double* __restrict__ logdens) {
    constexpr int D = RHS::D;
    const int lane = threadIdx.x;
    const bool joint = STORE || lane < 32;
    const int b = STORE ? blockIdx.x * 64 + lane : blockIdx.x * 32 + (lane & 31);
    double acc = 0.0;
    if (b < a.B) {
        const size_t B = (size_t)a.B;
        double Q[D][P][P], R[D][P][P], W[D][P], th[RHS::NTHETA], mu[D][P], S[D][P][P];
        lane_load_model<RHS, P>(a, b, Q, R, W, th);
        lane_load_init<D, P>(a, b, mu, S);
        if constexpr (STORE) {                                              // time 0: (ode_init, 0) (dalton.py:362-370)
            store_moments_all<D, P>(a.mean, a.var, B, 0, b, mu, S);
            if (a.mean_pred) store_moments_all<D, P>(a.mean_pred, a.var_pred, B, 0, b, mu, S);
        }
        // an observation at t_min contributes log p(y_0 | x_0) to the joint density and does not update x_0 (dalton.py:206-215)
        int i = 0;
        if (joint && o.n_obs > 0 && o.obs_ind[0] == 0) {
            if constexpr (!STORE) {
#pragma unroll
                for (int blk = 0; blk < D; ++blk) {
                    double m0[P], S0[P][P];
#pragma unroll
                    for (int r = 0; r < P; ++r) {
                        m0[r] = mu[blk][r];
#pragma unroll
                        for (int c = 0; c < P; ++c) S0[r][c] = 0.0;
                    }
                    dalton_observe<P, MO>(o, (size_t)blk, m0, S0, acc);
                }
            }
            i = 1;
        }

        const uint32_t traj = (uint32_t)(a.traj_offset + (uint64_t)b);
        for (int n = 0; n < a.N; ++n) {
            double mup[D][P], Sp[D][P][P];
#pragma unroll
            for (int blk = 0; blk < D; ++blk) predict_block<P>(Q[blk], R[blk], mu[blk], S[blk], mup[blk], Sp[blk]);
            double wgt[D][P], am[D], V[D];
            interrogate_traj<RHS, P, ITG>(W, th, step_time(a, n), mup, Sp, a.seed, traj, (uint32_t)n, wgt, am, V);
            const bool obs_here = joint && i < o.n_obs && o.obs_ind[i] == n + 1;
#pragma unroll
            for (int blk = 0; blk < D; ++blk) {
                double Wm[P];
#pragma unroll
                for (int j = 0; j < P; ++j) Wm[j] = W[blk][j] + wgt[blk][j];
                dalton_update_z<P>(Wm, am[blk], V[blk], mup[blk], Sp[blk], mu[blk], S[blk], acc);
                if (obs_here) dalton_observe<P, MO>(o, (size_t)i * D + blk, mu[blk], S[blk], acc);
            }
            if (obs_here) ++i;
            if constexpr (STORE) {
                store_moments_all<D, P>(a.mean, a.var, B, n + 1, b, mu, S);
                if (a.mean_pred) store_moments_all<D, P>(a.mean_pred, a.var_pred, B, n + 1, b, mup, Sp);
            }
        }
    }
    if constexpr (!STORE) store_joint_minus_marginal(acc, lane, b, a.B, logdens);
}

}  // namespace rk
