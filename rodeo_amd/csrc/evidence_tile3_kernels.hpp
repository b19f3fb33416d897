// solve_evidence on the p = 3 MFMA tiles (standard form, n_block 1..4): log p(Z_{1:N} = 0) with its per-block parts (an
// addition; DESIGN.md section 7 (12), evidence_kernels.hpp for the quantities and the no-threshold rule).  Shared by the
// ahead-of-time build (evidence.hip) and the hiprtc build of user right-hand sides (rhs_jit.hip, its evidence tile kind
// only).  RTC-safe: no host code.
//
// The step is dalton_fwd_tile3_kernel's, i.e. the generic step of fwd_tile3_kernel (solve_tile3_kernels.hpp, left
// untouched): one filter instance per trajectory, no observation path, no records -- the time loop stores nothing.  The
// forecast mean yhat = W~ mu- + a and the forecast variance S that the update forms anyway feed two accumulators,
// yhat^2 / S and log S, both the same in the 16 lanes of a tile.  The step has ONE division, 1 / S, for the gain and for
// yhat^2 / S, and no log: log S is accumulated as a running product (LogProd, evidence_kernels.hpp) with one log after the
// loop -- two divisions and a log() are 106 of the 120 VALU instructions of the plain form's step, on a chain that one
// wave per SIMD walks alone (1.27 ms against 0.40 ms for fwd_tile3_kernel on the headline shape).  After the loop lane
// (0, 0) of each tile stores its block's quad and logdet; a trajectory's blocks are tiles of one wave, summed there in block
// order, and one lane stores logdens[b].  No atomics, no memset: every output element has exactly one writer.
#pragma once
#include "solve_tile3_kernels.hpp"
#include "evidence_kernels.hpp"

namespace rk {

template <class RHS, int ITG>
__global__ void __launch_bounds__(64) evidence_tile3_kernel(SolveArgs a, double* __restrict__ logdens,
                                                            double* __restrict__ quad, double* __restrict__ logdet) {
    constexpr int D = RHS::D, P = 3, TPW = Tpw<D>::value;
    static_assert(D >= 1 && D <= 4, "evidence tile route: n_block in 1..4");
    static_assert(RHS::NDEP == 1, "tile path: right-hand sides that depend on X[b][0] only");
    static_assert(ITG != RK_INTERROGATE_CHKREBTII, "evidence: interrogate_chkrebtii is not served (no scale law)");
    const int n_tiles = a.B * D;
    const int lane = threadIdx.x;
    const TileCoord tc = tile_coord<D, TPW>(blockIdx.x, lane, n_tiles);
    const int r = tc.r, c = tc.c, blk = tc.blk, b = tc.b;
    const bool in3 = r < 3 && c < 3;

    // per-lane constants in D layout (fwd_tile3_kernel)
    const double Qt = in3 ? ld(a.Q, ((size_t)blk * P + c) * P + r, a.Q_b, a.B, b) : ((r == 3 && c == 3) ? 1.0 : 0.0);
    const double Qt0 = in3 ? Qt : 0.0;
    const double Rt = in3 ? ld(a.R, ((size_t)blk * P + r) * P + c, a.R_b, a.B, b) : 0.0;
    const double RtT = in3 ? ld(a.R, ((size_t)blk * P + c) * P + r, a.R_b, a.B, b) : 0.0;
    const double Wr = r < 3 ? ld(a.W, (size_t)blk * P + r, a.W_b, a.B, b) : 0.0;
    const double Y0 = r < 3 ? ld(a.Q, ((size_t)blk * P + 0) * P + r, a.Q_b, a.B, b) : 0.0;
    const double E0 = r == 0 ? 1.0 : 0.0;
    const double e3r = r == 3 ? 1.0 : 0.0;
    double th[RHS::NTHETA];
#pragma unroll
    for (int k = 0; k < RHS::NTHETA; ++k) th[k] = a.theta ? ld(a.theta, k, a.theta_b, a.B, b) : 0.0;
    double c3 = 0.0, c2 = 0.0, c1 = 0.0, co = 0.0, c0 = Wr;
    if constexpr (rhs_has_tile_form<RHS>::value && D == 2) {
        double tk[6];
        RHS::tile_consts(blk, th, tk);
        const bool jac = ITG == RK_INTERROGATE_KRAMER;
        const double k4 = jac ? tk[4] : 0.0, k5 = jac ? tk[5] : 0.0;
        if (r == 3) { c3 = k5 - tk[1]; c1 = k4 - tk[0]; co = -tk[2]; c0 = -tk[3]; }
        if (r == 0) { c2 = -k5; c0 = Wr - k4; }
    }
    double l0 = 0.0, l1 = 0.0, l2 = 0.0, l3 = 0.0, l4 = 0.0, XwL = 0.0;
    if constexpr (rhs_has_tile3_form<RHS>::value && D == 3) {
        double kk[5];
        RHS::tile3_consts(blk, th, kk);
        const bool jac = ITG == RK_INTERROGATE_KRAMER;
        l0 = jac ? 0.0 : -kk[0]; l1 = -kk[1]; l2 = -kk[2]; l3 = -kk[3]; l4 = -kk[4];
        XwL = fma(jac ? -kk[0] : 0.0, E0, Wr);
    }

    // M_0 = [0 | ode_init ; 0 1]
    const double x0r = r < 3 ? ld(a.x0, (size_t)blk * P + r, a.x0_b, a.B, b) : 0.0;
    double M = r < 3 ? (c == 3 ? x0r : 0.0) : (c == 3 ? 1.0 : 0.0);

    double accq = 0.0;
    LogProd lp;
    for (int n = 0; n < a.N; ++n) {
        // ---- predict (standard.py:57-59) ----
        const double U = MF(M, Qt, 0.0);
        const double v_own = quad_bcast3(MF(Y0, M, 0.0));         // mu-_0: the point the ODE is evaluated at
        const double Mp = MF(U, Qt, Rt);
        const double MpT = MF(Qt0, U, RtT);
        // ---- interrogation on the predicted moments ----
        const double t = a.t_min + (a.t_max - a.t_min) * (double)(n + 1) / (double)a.N;
        double Xw;                                                // rows W~_0, W~_1, W~_2, a
        if constexpr (rhs_has_tile_form<RHS>::value && D == 2) {
            const double v_oth = pair_other_quad_uniform(v_own);
            Xw = fma(fma(fma(c3, v_own, c2), v_own, c1), v_own, fma(co, v_oth, c0));
        } else if constexpr (rhs_has_tile3_form<RHS>::value && D == 3) {
            const double n1 = from_next_tile(v_own), p1 = from_prev_tile(v_own), p2 = dpp64<0x128>(v_own);
            const double a_meas = fma(l4, p2 * p1, fma(l3, p1 * n1, fma(l2, p1, fma(l1, n1, l0 * v_own))));
            Xw = fma(a_meas, e3r, XwL);
        } else {
            constexpr int PX = 1;
            double X[D][PX];
            double vals[D];
            gather_blocks<D>(v_own, vals);
#pragma unroll
            for (int bb = 0; bb < D; ++bb) X[bb][0] = vals[bb];
            double fb, J0;
            if constexpr (ITG == RK_INTERROGATE_KRAMER && rhs_has_fjac0<RHS>::value) {
                RHS::template fjac0_block<PX>(X, t, th, blk, fb, J0);
            } else if constexpr (ITG != RK_INTERROGATE_KRAMER && rhs_has_f_block<RHS>::value) {
                fb = RHS::template f_block<PX>(X, t, th, blk);
                J0 = 0.0;
            } else {
                double f[D], J[D][PX];
                if constexpr (ITG == RK_INTERROGATE_KRAMER) {
                    RHS::template fjac<PX>(X, t, th, f, J);
                } else {
                    RHS::template f<PX>(X, t, th, f);
#pragma unroll
                    for (int bb = 0; bb < D; ++bb) J[bb][0] = 0.0;
                }
                double J0s[D];
#pragma unroll
                for (int bb = 0; bb < D; ++bb) J0s[bb] = J[bb][0];
                fb = pick_block<D>(f, blk); J0 = pick_block<D>(J0s, blk);
            }
            const double a_meas = fma(J0, v_own, -fb);
            Xw = fma(-J0, E0, fma(a_meas, e3r, Wr));
        }
        // ---- z: forecast, the two sums and the update (standard.py:93-102) ----
        const double WS = MF(Xw, Mp, 0.0);                        // [W~ Sigma- | W~ mu- + a]
        const double Z0 = MF(MpT, Xw, 0.0);                       // Sigma- W~^T
        double S = MF(Z0, Xw, 0.0);                               // W~ Sigma- W~^T
        if constexpr (ITG == RK_INTERROGATE_RODEO) S = S + S;     // + var_meas = W Sigma- W^T (interrogate.py:110-113)
        const double yhat = quad_bcast3(WS);                      // forecast mean; x_meas = 0
        const double rS = 1.0 / S;                                // the step's one division: the gain and yhat^2 / S
        accq = fma(yhat * yhat, rS, accq);
        lp.mul(S);                                                // log S, as a product (evidence_kernels.hpp)
        M = fma(-(Z0 * rS), WS, Mp);
    }
    const double accl = lp.log();
    const size_t B = (size_t)a.B;
    if (tc.valid && r == 0 && c == 0) {
        quad[(size_t)blk * B + b] = accq;
        logdet[(size_t)blk * B + b] = accl;
    }
    // the trajectory's blocks are the tiles g0 .. g0 + D - 1 of this wave; lane 4 g of tile g holds its block's sums
    const int g0 = tc.g - blk;
    const double mine = accq + accl;
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) tot += __shfl(mine, ((g0 + k) & 3) << 2, 64);
    if (tc.valid && r == 0 && c == 0 && blk == 0) logdens[b] = evidence_logdens(tot, D, a.N);
}

}  // namespace rk
