// dalton_at on the p = 3 MFMA tiles (n_block 1..4, one observation per block, log-likelihood form only): the sibling of
// dalton_fwd_tile3_kernel<.., STORE = false> (dalton_tile3_kernels.hpp, left untouched).  Shared by the ahead-of-time build
// (dalton_at.hip) and the hiprtc build of user right-hand sides (rhs_jit.hip, JIT_DALTON_AT_TILE3 only).  RTC-safe.
//
// The time loop runs from event to event: the steps that hold no observation are an inner loop whose body is
// dalton_fwd_tile3_kernel's generic step, and the step with an event is that step with ONE wave-uniform branch at its head:
// when the interval (t_n, t_n+1) holds observations, each is reached by a predict over the gap in front of it (its "pre"
// pair, loaded in the D layout of Qt / Rt), conditioned on with the tile update of the node case, and the remaining predict
// to t_n+1 (the "post" pair) gives Mp, MpT and the evaluation point v_own from the sub-step's own row 0 in place of Y0.
// Filter instance k of 2 B runs trajectory k / 2, the joint filter for even k and the marginal one for odd k; the marginal
// filter takes the same split predictions and skips the conditioning (M = joint ? Mo : M).  The per-trajectory reduction is
// the two-addend atomic onto the zeroed logdens[b].
#pragma once
#include "dalton_tile3_kernels.hpp"
#include "dalton_at_kernels.hpp"

namespace rk {

template <class RHS, int ITG>
__global__ void __launch_bounds__(64) dalton_fwd_at_tile3_kernel(SolveArgs a, DaltonObs o, DaltonAt s, double* __restrict__ out) {
    constexpr int D = RHS::D, P = 3, TPW = Tpw<D>::value;
    static_assert(D >= 1 && D <= 4, "DALTON tile route: n_block in 1..4");
    static_assert(RHS::NDEP == 1, "tile path: right-hand sides that depend on X[b][0] only");
    static_assert(ITG != RK_INTERROGATE_CHKREBTII, "DALTON: interrogate_chkrebtii is not supported");
    const double LOG_2PI = 1.83787706640934548356;
    const int n_tiles = 2 * a.B * D;
    const int lane = threadIdx.x;
    const TileCoord tc = tile_coord<D, TPW>(blockIdx.x, lane, n_tiles);
    const int r = tc.r, c = tc.c, blk = tc.blk, inst = tc.b;
    const int b = inst >> 1;
    const bool joint = (inst & 1) == 0;
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

    double acc = 0.0;
    int i = 0;
    if (o.n_obs > 0 && s.tab[0] == 0 && s.tab[1] == 0) {
        // an observation at t_min: log N(y_0; D_0 x_0, Omega_0) with utils.py:60-78's rule, in the joint density only; x_0 is
        // not updated (dalton.py:206-215).  Lane (0, 0) of a tile carries its block's value.
        if (joint) {
            double mean = 0.0;
#pragma unroll
            for (int k = 0; k < P; ++k) mean = fma(o.obs_w[(size_t)blk * P + k], ld(a.x0, (size_t)blk * P + k, a.x0_b, a.B, b), mean);
            const double w = o.obs_v[blk], z = o.obs[blk] - mean;
            if (fabs(w) > 1e-8) acc += -0.5 * (z * z / w + log(w)) - 0.5 * LOG_2PI;
        }
        i = 1;
    }
    // the next observation (the same in every lane): `next` is its grid index when it sits on a node, `noff` the index of its
    // interval's left node when it does not; the other one is -1
    int next = -1, noff = -1;
    if (i < o.n_obs) {
        const int node = s.tab[4 * i], off = s.tab[4 * i + 1];
        next = off ? -1 : node;
        noff = off ? node : -1;
    }

    // The interrogation, the z forecast log-density and the z update of node n + 1 from the predicted tiles (the generic
    // step of dalton_fwd_tile3_kernel from its interrogation on): shared by the two places a step is taken below.
    auto z_step = [&](int n, double v_own, double Mp, double MpT) {
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
        const double yhat = quad_bcast3(WS);                      // forecast mean; x_meas = 0
        if (fabs(S) > 1e-8) acc += -0.5 * (yhat * yhat / S + log(S)) - 0.5 * LOG_2PI;
        M = fma(-(Z0 / S), WS, Mp);
    };

    // The time loop runs from event to event.  The steps in front of the next event -- an interval that holds observations,
    // or a node with one -- are an inner loop whose body is dalton_fwd_tile3_kernel's generic step and nothing else; the step
    // with the event is taken once, outside it.
    int n = 0;
    while (n < a.N) {
        int stop = noff >= 0 ? noff : (next >= 1 ? next - 1 : a.N);          // the step that holds the next event
        stop = stop < n ? n : (stop > a.N ? a.N : stop);
        for (; n < stop; ++n) {
            // ---- predict (standard.py:57-59) ----
            const double U = MF(M, Qt, 0.0);
            const double v_own = quad_bcast3(MF(Y0, M, 0.0));         // mu-_0: the point the ODE is evaluated at
            const double Mp = MF(U, Qt, Rt);
            const double MpT = MF(Qt0, U, RtT);
            z_step(n, v_own, Mp, MpT);
        }
        if (n >= a.N) break;
        double U, v_own, Mp, MpT;
        if (noff == n) {
            // ---- the interval (t_n, t_n+1) holds observations: predict to each, condition, predict on to t_n+1 ----
            int post = -1;
            do {
                const int slot = dalton_at_slot(s.tab[4 * i + 2], s.n_pre);
                const size_t e = ((size_t)slot * D + blk) * P * P;
                const double Q1 = in3 ? ld(s.pre_q, e + c * P + r, s.prior_b, a.B, b) : ((r == 3 && c == 3) ? 1.0 : 0.0);
                const double R1 = in3 ? ld(s.pre_r, e + r * P + c, s.prior_b, a.B, b) : 0.0;
                const double U1 = MF(M, Q1, 0.0);
                M = MF(U1, Q1, R1);                               // the state predicted to the observation's own time
                const size_t ib = (size_t)i * D + blk;
                const double xw = r < 3 ? o.obs_w[ib * P + r] : -o.obs[ib];
                double MT = MF(M, I4, 0.0);                       // M^T (one MFMA with the identity), row 3 zeroed
                MT = r == 3 ? 0.0 : MT;
                const double WSo = MF(xw, M, 0.0);                // [D Sigma | D mu - y]
                const double Zo = MF(MT, xw, 0.0);                // Sigma D^T
                const double w = MF(Zo, xw, 0.0) + o.obs_v[ib];   // var_fore
                const double z = -quad_bcast3(WSo);               // y - D mu
                const double lp = fabs(w) > 1e-8 ? -0.5 * (z * z / w + log(w)) - 0.5 * LOG_2PI : 0.0;
                const double Mo = fma(-(Zo / w), WSo, M);
                acc += joint ? lp : 0.0;
                M = joint ? Mo : M;
                post = s.tab[4 * i + 3];
                ++i;
            } while (post < 0 && i < o.n_obs && s.tab[4 * i + 1] != 0 && s.tab[4 * i] == n);
            next = noff = -1;
            if (i < o.n_obs) {
                const int node = s.tab[4 * i], off = s.tab[4 * i + 1];
                next = off ? -1 : node;
                noff = off ? node : -1;
            }
            post = dalton_at_slot(post, s.n_post);
            const size_t e = ((size_t)post * D + blk) * P * P;
            const double Q2 = in3 ? ld(s.post_q, e + c * P + r, s.prior_b, a.B, b) : ((r == 3 && c == 3) ? 1.0 : 0.0);
            const double Q20 = in3 ? Q2 : 0.0;
            const double R2 = in3 ? ld(s.post_r, e + r * P + c, s.prior_b, a.B, b) : 0.0;
            const double R2T = in3 ? ld(s.post_r, e + c * P + r, s.prior_b, a.B, b) : 0.0;
            const double Y2 = r < 3 ? ld(s.post_q, e + r, s.prior_b, a.B, b) : 0.0;       // the sub-step's row 0
            U = MF(M, Q2, 0.0);
            v_own = quad_bcast3(MF(Y2, M, 0.0));
            Mp = MF(U, Q2, R2);
            MpT = MF(Q20, U, R2T);
        } else {
            U = MF(M, Qt, 0.0);
            v_own = quad_bcast3(MF(Y0, M, 0.0));
            Mp = MF(U, Qt, Rt);
            MpT = MF(Qt0, U, RtT);
        }
        z_step(n, v_own, Mp, MpT);
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
            next = noff = -1;
            if (i < o.n_obs) {
                const int node = s.tab[4 * i], off = s.tab[4 * i + 1];
                next = off ? -1 : node;
                noff = off ? node : -1;
            }
        }
        ++n;
    }
    // the instance's blocks are the tiles g0 .. g0 + D - 1 of this wave; lane 4 g of tile g holds its block's sum
    const int g0 = tc.g - blk;
    double s_sum = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) s_sum += __shfl(acc, ((g0 + k) & 3) << 2, 64);
    if (tc.valid && r == 0 && c == 0 && blk == 0) atomicAdd(&out[b], joint ? s_sum : -s_sum);
}

}  // namespace rk
