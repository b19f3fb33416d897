// dalton_at: DALTON's log-likelihood for Gaussian observations whose times need not be nodes of the solver grid
// (DESIGN.md section 7 (10)), lane-per-trajectory form.  The sibling of dalton_fwd_kernel<.., STORE = false>
// (dalton_kernels.hpp, left untouched).  Shared by the ahead-of-time build (dalton_at.hip) and the hiprtc build of user
// right-hand sides (rhs_jit.hip, JIT_DALTON_AT only).  RTC-safe: no host code.
//
// An observation at t in (t_n, t_n+1) splits the prediction of step n: predict over t - (previous event) with the prior of
// that gap (a "pre" pair), condition on y (dalton_observe, as at a node), and after the interval's last observation predict
// up to t_n+1 with the "post" pair; the interrogation and the z update at node n + 1 follow as always.  The marginal filter
// takes the same split predictions without the conditioning, so both densities see the same prediction arithmetic.  An
// observation on a node is handled as in dalton_fwd_kernel (z first, y second).
#pragma once
#include "dalton_kernels.hpp"

namespace rk {

// Sub-step priors and the observation table of rk_dalton_loglik_at.  pre_* (n_pre, D, P, P [, B]): the prior over the gap in
// front of each off-grid observation; post_* (n_post, D, P, P [, B]): the prior from an interval's last observation to its
// right node; batch-minor where prior_b.  tab (n_obs, 4): node, off-grid flag, pre slot, post slot of the interval's last
// observation or -1.  With the flag clear the observation sits on grid node `node`; with it set it lies in (t_node, t_node+1).
struct DaltonAt {
    const double *pre_q, *pre_r, *post_q, *post_r;
    const int32_t* tab;
    int n_pre, n_post, prior_b;
};

__device__ __forceinline__ int dalton_at_slot(int slot, int n) { return slot < 0 ? 0 : (slot >= n ? n - 1 : slot); }

// One block's predict (standard.py:57-59) over sub-step `slot`, in place, with the matrices streamed from memory: each
// element is loaded where it is used, so this rare branch holds no second prior in registers next to the step's own (with
// load_block_consts + predict_block the n_bstate = 6 instances took 2.3 to 2.5 KB of scratch per lane).  The loads are
// volatile so that the compiler neither hoists nor keeps the 2 P^2 values; DESIGN.md section 7 (10) lists what each instance
// uses and what would replace this.  Every element is accumulated in predict_block's order (mv / mm / mm_nt: k ascending, a
// product, then fused multiply-adds).
template <int P>
__device__ __forceinline__ void predict_block_stream(const double* q, const double* r, int slot, int nblk, int blk, int batched,
                                                     int B, int b, double (&mu)[P], double (&S)[P][P]) {
    const size_t stride = batched ? (size_t)B : 1, off = batched ? (size_t)b : 0;
    const volatile double* const Q = q + ((size_t)slot * nblk + blk) * P * P * stride + off;
    const volatile double* const R = r + ((size_t)slot * nblk + blk) * P * P * stride + off;
    double mup[P], A[P][P];
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int k = 0; k < P; ++k) {
            const double e = Q[(size_t)(i * P + k) * stride];
            mup[i] = k == 0 ? e * mu[0] : fma(e, mu[k], mup[i]);
#pragma unroll
            for (int j = 0; j < P; ++j) A[i][j] = k == 0 ? e * S[0][j] : fma(e, S[k][j], A[i][j]);
        }
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
        for (int k = 0; k < P; ++k) {
            const double e = Q[(size_t)(j * P + k) * stride];
#pragma unroll
            for (int i = 0; i < P; ++i) S[i][j] = k == 0 ? A[i][0] * e : fma(A[i][k], e, S[i][j]);
        }
#pragma unroll
    for (int i = 0; i < P; ++i) {
        mu[i] = mup[i];
#pragma unroll
        for (int j = 0; j < P; ++j) S[i][j] = S[i][j] + R[(size_t)(i * P + j) * stride];
    }
}

// A wave holds 32 trajectories: lanes 0..31 run their joint filters, lanes 32..63 their marginal filters, and
// logdens[b] = joint - marginal leaves through one cross-lane read (dalton_fwd_kernel's log-likelihood form).  The table
// is walked by every lane alike (the index i is wave-uniform); only the conditioning is the joint half's.
template <class RHS, int P, int ITG, int MO>
__global__ void __launch_bounds__(64) dalton_fwd_at_kernel(SolveArgs a, DaltonObs o, DaltonAt s, double* __restrict__ logdens) {
    constexpr int D = RHS::D;
    const int lane = threadIdx.x;
    const bool joint = lane < 32;
    const int b = blockIdx.x * 32 + (lane & 31);
    double acc = 0.0;
    if (b < a.B) {
        double Q[D][P][P], R[D][P][P], W[D][P], th[RHS::NTHETA], mu[D][P], S[D][P][P];
        lane_load_model<RHS, P>(a, b, Q, R, W, th);
        lane_load_init<D, P>(a, b, mu, S);
        // an observation at t_min contributes log p(y_0 | x_0) to the joint density and does not update x_0 (dalton.py:206-215)
        int i = 0;
        if (o.n_obs > 0 && s.tab[0] == 0 && s.tab[1] == 0) {
            if (joint) {
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
            if (i < o.n_obs && s.tab[4 * i + 1] != 0 && s.tab[4 * i] == n) {
                // ---- the interval (t_n, t_n+1) holds observations: predict to each, condition, predict to t_n+1 ----
                int post = -1;
                do {
                    const int slot = dalton_at_slot(s.tab[4 * i + 2], s.n_pre);
#pragma unroll
                    for (int blk = 0; blk < D; ++blk) {
                        predict_block_stream<P>(s.pre_q, s.pre_r, slot, D, blk, s.prior_b, a.B, b, mu[blk], S[blk]);
                        if (joint) dalton_observe<P, MO>(o, (size_t)i * D + blk, mu[blk], S[blk], acc);
                    }
                    post = s.tab[4 * i + 3];
                    ++i;
                } while (post < 0 && i < o.n_obs && s.tab[4 * i + 1] != 0 && s.tab[4 * i] == n);
                post = dalton_at_slot(post, s.n_post);
#pragma unroll
                for (int blk = 0; blk < D; ++blk) {
                    predict_block_stream<P>(s.post_q, s.post_r, post, D, blk, s.prior_b, a.B, b, mu[blk], S[blk]);
#pragma unroll
                    for (int r = 0; r < P; ++r) {
                        mup[blk][r] = mu[blk][r];
#pragma unroll
                        for (int c = 0; c < P; ++c) Sp[blk][r][c] = S[blk][r][c];
                    }
                }
            } else {
#pragma unroll
                for (int blk = 0; blk < D; ++blk) predict_block<P>(Q[blk], R[blk], mu[blk], S[blk], mup[blk], Sp[blk]);
            }
            double wgt[D][P], am[D], V[D];
            interrogate_traj<RHS, P, ITG>(W, th, step_time(a, n), mup, Sp, a.seed, traj, (uint32_t)n, wgt, am, V);
            const bool node_here = i < o.n_obs && s.tab[4 * i + 1] == 0 && s.tab[4 * i] == n + 1;
            const bool obs_here = joint && node_here;
#pragma unroll
            for (int blk = 0; blk < D; ++blk) {
                double Wm[P];
#pragma unroll
                for (int j = 0; j < P; ++j) Wm[j] = W[blk][j] + wgt[blk][j];
                dalton_update_z<P>(Wm, am[blk], V[blk], mup[blk], Sp[blk], mu[blk], S[blk], acc);
                if (obs_here) dalton_observe<P, MO>(o, (size_t)i * D + blk, mu[blk], S[blk], acc);
            }
            if (node_here) ++i;
        }
    }
    store_joint_minus_marginal(acc, lane, b, a.B, logdens);
}

}  // namespace rk
