// solve_sim_draws (an addition): host side of rk_solve_sim_draws and its backward kernel -- many
// sample paths per trajectory from ONE forward filter.  Route: rk_solve_filter's lanes on batch-minor records (called, not
// copied), then bwd_sim_draws_kernel, one lane per (draw chunk, block, trajectory): bwd_sim_kernel of solve_small.hip with the
// work that no draw changes -- the record's load, predict_block, smooth_gain, Sigma_f - G T^T and its psd_factor -- done once
// per step for the 1, 2 or SIM_DRAWS_CHUNK draws the lane carries, and with a store only at the nodes of `keep`.
// THE SEED LAW: draw s is rk_solve_sim's path under the seed cfg->seed + s (mod 2^64) -- Philox is keyed with
// (seed + s, trajectory, step, block, PURPOSE_SMOOTH), bwd_sim_kernel's key.  Standard form, n_bstate 2..6, any n_block,
// interrogate rodeo / schober / kramer.  Nothing but out->mean_state / var_state (the filtered moments) and x_draws is
// written; there is no workspace.
#include <string>
#include "common.hpp"
#include "kalman_small.hpp"
#include "philox.hpp"
#include "rhs.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "records.hpp"

namespace rk {

// (SIM_DRAWS_CHUNK, the most draws a lane carries, and sim_draws_chunk, the rule that picks 1, 2 or that per call, are in
// solve_paths.hpp: grid_draws.hip shares them)
constexpr int SIM_DRAWS_PMIN = 2, SIM_DRAWS_PMAX = 6;

// Mirrors lane_backward.hpp (BwdLane, bwd_walk under StaticPrior, store_path, load_path_init), written out: through them <3, 1>
// ran 0.9 % slower, with the walk alone written out <3, 4> 0.35 % ("One walk for the lane backward passes")
// x_draws (n_draws, K, D, P, B): element i of (draw s, kept row k, block blk, trajectory b) at (((s K + k) D + blk) P + i) B + b
template <int P, int C>
__global__ void __launch_bounds__(64) bwd_sim_draws_kernel(SolveArgs a, int n_draws, const int32_t* __restrict__ keep, int n_keep,
                                                           double* __restrict__ xd) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= a.B * a.D) return;
    const int blk = l / a.B, b = l - blk * a.B;
    const int s0 = blockIdx.y * C;                                          // the chunk's first draw; draw s0 + c exists below n_draws
    const size_t B = (size_t)a.B;
    const uint32_t traj = (uint32_t)(a.traj_offset + (uint64_t)b);
    const int K = keep ? n_keep : a.N + 1;
    double Q[P][P], R[P][P];
    load_block_consts<P>(a, blk, b, Q, R);

    // the kept rows, walked from the end as the chain walks the nodes down: row kp is the next one to store (without `keep`
    // row kp is node kp).  kp stays in 0 .. K - 1 whatever `keep` holds, so no store leaves x_draws.
    int kp = K - 1;
    auto kept = [&](int n) { return !keep || (kp >= 0 && keep[kp] == n); };
    auto store_x = [&](int c, const double (&x)[P]) {
        double* xo = xd + (((size_t)(s0 + c) * K + kp) * a.D + blk) * P * B + b;     // (bm_item with a 64-bit row index)
#pragma unroll
        for (int i = 0; i < P; ++i) xo[(size_t)i * B] = x[i];
    };

    double mf[P], Sf[P][P], xn[C][P], L[P][P];
    // terminal draws x_N ~ N(filt[N]) (solve.py:182-186): one factor, C applications
    load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, a.N, blk, b, mf, Sf);
    psd_factor<P>(Sf, L);
    {
        const bool st = kept(a.N);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (s0 + c < n_draws) {
                double z[P];
                normals<P>(a.seed + (uint64_t)(s0 + c), traj, (uint32_t)a.N, (uint32_t)blk, PURPOSE_SMOOTH, z);
                mvn_apply<P>(mf, L, z, xn[c]);
                if (st) store_x(c, xn[c]);
            }
        }
        if (st) --kp;
    }
    if (a.N >= 2) load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, a.N - 1, blk, b, mf, Sf);
    for (int n = a.N - 1; n >= 1; --n) {
        // software prefetch of the next (earlier) filtered state while this step computes
        double mfn[P], Sfn[P][P];
        if (n >= 2) load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, n - 1, blk, b, mfn, Sfn);
        double mp[P], G[P][P];
        {
            double Sp[P][P], T[P][P], Ssim[P][P];
            predict_block<P>(Q, R, mf, Sf, mp, Sp);      // pred[n+1] re-evaluated from filt[n]
            smooth_gain<P>(Q, Sf, Sp, T, G);
            smooth_sim_var<P>(G, T, Sf, Ssim);
            psd_factor<P>(Ssim, L);
        }
        const bool st = kept(n);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (s0 + c < n_draws) {
                double msim[P], z[P];
                smooth_sim_mean<P>(G, mf, mp, xn[c], msim);
                normals<P>(a.seed + (uint64_t)(s0 + c), traj, (uint32_t)n, (uint32_t)blk, PURPOSE_SMOOTH, z);
                mvn_apply<P>(msim, L, z, xn[c]);
                if (st) store_x(c, xn[c]);
            }
        }
        if (st) --kp;
        if (n >= 2) {
#pragma unroll
            for (int i = 0; i < P; ++i) {
                mf[i] = mfn[i];
#pragma unroll
                for (int j = 0; j < P; ++j) Sf[i][j] = Sfn[i][j];
            }
        }
    }
    // x[0] = ode_init exactly (solve.py:196-204)
    if (kept(0)) {
        double x0[P];
#pragma unroll
        for (int i = 0; i < P; ++i) x0[i] = a.mean[((size_t)blk * P + i) * B + b];
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (s0 + c < n_draws) store_x(c, x0);
    }
}

// ---- dispatch ---------------------------------------------------------------------------------------------------
// Is this configuration served?  Decided on the configuration alone: RK_OK, RK_ERR_INVALID (sizes, the layout flag) or
// RK_ERR_UNSUPPORTED.
static int sim_draws_check(const rk_solve_cfg* c) {
    RK_REQUIRE(c->n_traj >= 1 && c->n_steps >= 1 && c->n_block >= 1 && c->n_bstate >= 1 && c->n_bmeas >= 1, RK_ERR_INVALID,
               "sim_draws: non-positive dimension (n_traj=%d n_steps=%d n_block=%d n_bstate=%d n_bmeas=%d)", c->n_traj,
               c->n_steps, c->n_block, c->n_bstate, c->n_bmeas);
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD || c->kalman_type == RK_KALMAN_SQRT, RK_ERR_UNSUPPORTED,
               "sim_draws: unknown kalman_type %d", c->kalman_type);
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD, RK_ERR_UNSUPPORTED, "sim_draws: kalman_type square-root is not built");
    RK_REQUIRE(c->interrogate != RK_INTERROGATE_CHKREBTII, RK_ERR_UNSUPPORTED,
               "sim_draws: interrogate_chkrebtii is not served (its forward pass depends on the key, so the draws cannot share "
               "one filter)");
    RK_REQUIRE(c->interrogate >= RK_INTERROGATE_RODEO && c->interrogate <= RK_INTERROGATE_KRAMER, RK_ERR_UNSUPPORTED,
               "sim_draws: interrogate id %d is not supported (rodeo, schober, kramer)", c->interrogate);
    RK_REQUIRE(c->n_bmeas == 1, RK_ERR_UNSUPPORTED, "sim_draws: n_bmeas = 1 only (the dense / indep_init form is not served), "
               "got %d", c->n_bmeas);
    RK_REQUIRE(c->n_bstate >= SIM_DRAWS_PMIN && c->n_bstate <= SIM_DRAWS_PMAX, RK_ERR_UNSUPPORTED,
               "sim_draws: n_bstate in %d..%d, got %d", SIM_DRAWS_PMIN, SIM_DRAWS_PMAX, c->n_bstate);
    if (is_user_rhs(c->rhs_id)) {
        const int rc = user_rhs_check(c);
        if (rc) {
            const std::string why = rk_last_error();
            set_error("sim_draws: %s", why.c_str());
            return rc;
        }
    } else {
        RK_REQUIRE(with_builtin_rhs(c->rhs_id, [](auto) {}), RK_ERR_UNSUPPORTED, "sim_draws: unknown rhs_id %d", c->rhs_id);
        RK_REQUIRE(builtin_has_n_block(c->rhs_id, c->n_block), RK_ERR_UNSUPPORTED,
                   "sim_draws: rhs %d needs another n_block than %d", c->rhs_id, c->n_block);
    }
    RK_REQUIRE(c->flags & RK_FLAG_BATCH_MINOR, RK_ERR_INVALID,
               "sim_draws: the backward kernel reads batch-minor filtered records (set RK_FLAG_BATCH_MINOR)");
    return RK_OK;
}

template <int C>
static int launch_sim_draws(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, int n_draws, const int32_t* keep, int n_keep,
                            double* x_draws) {
    LaunchGeom g = bwd_lane_geom(a.B, a.D);
    g.grid.y = div_up(n_draws, C);
    LaunchTimer t(h, "bwd_sim_draws_kernel");
    const bool ok = dispatch_int<SIM_DRAWS_PMIN, SIM_DRAWS_PMAX>(c->n_bstate, [&](auto P) {
        hipLaunchKernelGGL((bwd_sim_draws_kernel<P, C>), g.grid, g.block, 0, h->stream, a, n_draws, keep, n_keep, x_draws);
    });
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "sim_draws: no backward kernel for n_bstate %d", c->n_bstate);
    t.stop();
    RK_HIP(hipGetLastError());
    return RK_OK;
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_solve_sim_draws(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, int32_t n_draws,
                       const int32_t* keep, int32_t n_keep, double* x_draws) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_solve_sim_draws: null cfg");
    int rc = sim_draws_check(c);                                    // (the configuration alone, before anything else is looked at)
    if (rc) return rc;
    // (65535 chunks: the grid's second dimension)
    RK_REQUIRE(n_draws >= 1 && n_draws <= 65535, RK_ERR_INVALID, "sim_draws: n_draws must be in 1..65535, got %d", n_draws);
    RK_REQUIRE(!keep || (n_keep >= 1 && n_keep <= c->n_steps + 1), RK_ERR_INVALID,
               "sim_draws: n_keep must be in 1..n_steps + 1 = %d, got %d", c->n_steps + 1, n_keep);
    RK_REQUIRE(h && in && out && x_draws, RK_ERR_INVALID, "rk_solve_sim_draws: null argument");
    RK_REQUIRE(out->mean_state && out->var_state, RK_ERR_INVALID,
               "rk_solve_sim_draws: out->mean_state / var_state must not be NULL");
    rc = rk_solve_filter(h, c, in, out);                            // the forward pass of a batch-minor plan, built-in or hiprtc
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, out, a);
    switch (sim_draws_chunk(h, c, n_draws)) {
        case 1: return launch_sim_draws<1>(h, c, a, n_draws, keep, n_keep, x_draws);
        case 2: return launch_sim_draws<2>(h, c, a, n_draws, keep, n_keep, x_draws);
        default: return launch_sim_draws<SIM_DRAWS_CHUNK>(h, c, a, n_draws, keep, n_keep, x_draws);
    }
}

int rk_sim_draws_chunk(void) { return SIM_DRAWS_CHUNK; }

}  // extern "C"
