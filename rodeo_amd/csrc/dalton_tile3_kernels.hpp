// DALTON for Gaussian observations (src/rodeo/inference/dalton.py:39-545) on the p = 3 MFMA tiles, n_block 1..4, one
// observation per block.  Shared by the ahead-of-time build (dalton.hip) and the hiprtc build of user right-hand sides
// (rhs_jit.hip, its DALTON tile kinds only).  RTC-safe: no host code.
//
// The step is the generic step of fwd_tile3_kernel (solve_tile3_kernels.hpp, left untouched: its schedule is tuned to the
// instruction) with two additions: the z forecast log-density, from the forecast variance S and the forecast mean
// W~ mu- + a that the update forms anyway; and, at the grid index of an observation, the tile update with the measurement
// row [D_i | -y_i] and the variance Omega_i of fenrir_bwd_tile3_kernel's observe() (solve_tile3.hip) and its log-density
// (sequential conditioning, dalton_kernels.hpp).  Steps with an observation are rare; that path is not tuned.
//
// STORE = false (rk_dalton_loglik): filter instance k of 2B runs trajectory k / 2, the joint filter for even k and the
// marginal one for odd k, so a trajectory's joint and marginal tiles are neighbours and share the wave whenever
// 2 n_block <= 4.  The instance's block values are summed in the wave in a fixed order and leave through one atomic add
// each onto the zeroed logdens[b]: two addends onto zero, so the value does not depend on their order.
// STORE = true (rk_dalton_solve): the joint filter of each trajectory writes RK_LAYOUT_TILE3 records in exactly
// fwd_tile3_kernel's format; bwd_mv_tile3_kernel / bwd_sim_tile3_kernel run on them unchanged (they re-evaluate the
// predictions from the filtered moments with the same prior, which is what this filter predicted).
#pragma once
#include "solve_tile3_kernels.hpp"
#include "dalton_kernels.hpp"

namespace rk {

template <class RHS, int ITG, bool STORE>
__global__ void __launch_bounds__(64) dalton_fwd_tile3_kernel(SolveArgs a, DaltonObs o, double* __restrict__ out) {
    constexpr int D = RHS::D, P = 3, TPW = Tpw<D>::value;
    static_assert(D >= 1 && D <= 4, "DALTON tile route: n_block in 1..4");
    static_assert(RHS::NDEP == 1, "tile path: right-hand sides that depend on X[b][0] only");
    static_assert(ITG != RK_INTERROGATE_CHKREBTII, "DALTON: interrogate_chkrebtii is not supported");
    const double LOG_2PI = 1.83787706640934548356;
    const int n_tiles = (STORE ? a.B : 2 * a.B) * D;
    const int lane = threadIdx.x;
    const TileCoord tc = tile_coord<D, TPW>(blockIdx.x, lane, n_tiles);
    const int r = tc.r, c = tc.c, blk = tc.blk, inst = tc.b;
    const int b = STORE ? inst : inst >> 1;
    const bool joint = STORE || (inst & 1) == 0;
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
    const double I4 = r == c ? 1.0 : 0.0;
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
    const bool st = STORE && tc.valid && r < 3;
    double* const rec = out + (size_t)tc.tau * TILE_DOUBLES + r * 4 + c;
    const size_t tstride = (size_t)n_tiles * TILE_DOUBLES;

    double acc = 0.0;
    int i = 0;
    if (o.n_obs > 0 && o.obs_ind[0] == 0) {
        // an observation at t_min: log N(y_0; D_0 x_0, Omega_0) with utils.py:60-78's rule, in the joint density only; x_0 is
        // not updated (dalton.py:206-215).  Lane (0, 0) of a tile carries its block's value.
        if (!STORE && joint) {
            double mean = 0.0;
#pragma unroll
            for (int k = 0; k < P; ++k) mean = fma(o.obs_w[(size_t)blk * P + k], ld(a.x0, (size_t)blk * P + k, a.x0_b, a.B, b), mean);
            const double w = o.obs_v[blk], z = o.obs[blk] - mean;
            if (fabs(w) > 1e-8) acc += -0.5 * (z * z / w + log(w)) - 0.5 * LOG_2PI;
        }
        i = 1;
    }
    int next = i < o.n_obs ? o.obs_ind[i] : -1;                  // grid index of the next observation (the same in every lane)

    for (int n = 0; n < a.N; ++n) {
        if (st) rec[(size_t)n * tstride] = M;                     // the state of time n
        // ---- predict (standard.py:57-59) ----
        const double U = MF(M, Qt, 0.0);
        const double v_own = quad_bcast3(MF(Y0, M, 0.0));         // mu-_0: the point the ODE is evaluated at
        const double Mp = MF(U, Qt, Rt);
        const double MpT = MF(Qt0, U, RtT);
        // ---- interrogation on this filter's own predicted moments (dalton.py:112-134) ----
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
        // ---- z: forecast, log-density and update (standard.py:93-102, utils.py:60-78) ----
        const double WS = MF(Xw, Mp, 0.0);                        // [W~ Sigma- | W~ mu- + a]
        const double Z0 = MF(MpT, Xw, 0.0);                       // Sigma- W~^T
        double S = MF(Z0, Xw, 0.0);                               // W~ Sigma- W~^T
        if constexpr (ITG == RK_INTERROGATE_RODEO) S = S + S;     // + var_meas = W Sigma- W^T (interrogate.py:110-113)
        if constexpr (!STORE) {
            const double yhat = quad_bcast3(WS);                  // forecast mean; x_meas = 0
            if (fabs(S) > 1e-8) acc += -0.5 * (yhat * yhat / S + log(S)) - 0.5 * LOG_2PI;
        }
        M = fma(-(Z0 / S), WS, Mp);
        // ---- y given z at an observation's grid index (joint filter only; dalton.py:136-149) ----
        if (next == n + 1) {
            const size_t ib = (size_t)i * D + blk;
            const double xw = r < 3 ? o.obs_w[ib * P + r] : -o.obs[ib];
            double MT = MF(M, I4, 0.0);                           // M^T (one MFMA with the identity), row 3 zeroed
            MT = r == 3 ? 0.0 : MT;
            const double WSo = MF(xw, M, 0.0);                    // [D Sigma | D mu - y]
            const double Zo = MF(MT, xw, 0.0);                    // Sigma D^T
            const double w = MF(Zo, xw, 0.0) + o.obs_v[ib];       // var_fore
            const double z = -quad_bcast3(WSo);                   // y - D mu
            const double lp = fabs(w) > 1e-8 ? -0.5 * (z * z / w + log(w)) - 0.5 * LOG_2PI : 0.0;
            const double Mo = fma(-(Zo / w), WSo, M);
            acc += joint ? lp : 0.0;
            M = joint ? Mo : M;
            ++i;
            next = i < o.n_obs ? o.obs_ind[i] : -1;
        }
    }
    if (st) rec[(size_t)a.N * tstride] = M;                       // time N
    if constexpr (!STORE) {
        // the instance's blocks are the tiles g0 .. g0 + D - 1 of this wave; lane 4 g of tile g holds its block's sum
        const int g0 = tc.g - blk;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) s += __shfl(acc, ((g0 + k) & 3) << 2, 64);
        if (tc.valid && r == 0 && c == 0 && blk == 0) atomicAdd(&out[b], joint ? s : -s);
    }
}

}  // namespace rk
