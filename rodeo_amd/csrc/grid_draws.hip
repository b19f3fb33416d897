// solve_sim_draws_grid / dalton.solve_sim_draws_grid (an addition): host side of
// rk_solve_sim_draws_grid and rk_dalton_grid_sim_draws and their backward kernel -- many sample paths per trajectory from ONE
// forward filter on a non-uniform grid shared by the batch.  Route: grid.hip's forward launch (grid_fwd_kernel) or dalton_grid.hip's
// store form (dalton_grid_fwd_kernel<store>), called, not copied, on batch-minor records; then grid_bwd_sim_draws_kernel, one lane
// per (draw chunk, block, trajectory): bwd_sim_draws_kernel of sim_draws.hip with the prior pair of step n (grid_kernels.hpp:
// grid_load_pair / grid_slot) in place of the lane's loop-invariant Q, R -- in the prediction and in the smoothing gain.
// THE SEED LAW: draw s is rk_solve_grid's (rk_dalton_grid_solve's) RK_MODE_SIM path under the seed cfg->seed + s (mod 2^64) --
// Philox is keyed with (seed + s, trajectory, step, block, PURPOSE_SMOOTH), grid_bwd_sim_kernel's key.  Standard form, n_bstate
// 2..6 (2..5 with three or more blocks), interrogate rodeo / schober / kramer.  Nothing but out->mean_state / var_state (the
// filtered moments) and x_draws is written; there is no workspace.  The pieces of the configuration check, the grid's staging
// and the test of the output pointers are grid_entry.hpp's.
#include "common.hpp"
#include "kalman_small.hpp"
#include "philox.hpp"
#include "rhs.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "grid_entry.hpp"
#include "records.hpp"
#include "grid_kernels.hpp"
#include "dalton_kernels.hpp"

namespace rk {

constexpr int GRID_DRAWS_PMIN = 2, GRID_DRAWS_PMAX = 6;
constexpr int GRID_DRAWS_PMAX_THREE_BLOCKS = 5;

// The walk is written out, as in sim_draws.hip and for its reason (through lane_backward.hpp's BwdLane / bwd_walk the one-draw
// sibling ran 0.9 % slower): bwd_walk's step is a callback per node, and here the per-step work (once) and the per-draw work (C
// times) sit in one body next to the kept-row cursor, which a callback would have to capture.  What bwd_walk does under
// SlotPrior is mirrored: the pair of step n - 1 is fetched next to filt[n - 1], one step ahead of its use, and rotated in
// behind the step.
// x_draws (n_draws, K, D, P, B): element i of (draw s, kept row k, block blk, trajectory b) at (((s K + k) D + blk) P + i) B + b
template <int P, int C>
__global__ void __launch_bounds__(64) grid_bwd_sim_draws_kernel(SolveArgs a, GridArgs g, int n_draws,
                                                                const int32_t* __restrict__ keep, int n_keep,
                                                                double* __restrict__ xd) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= a.B * a.D) return;
    const int blk = l / a.B, b = l - blk * a.B;
    const int s0 = blockIdx.y * C;                                          // the chunk's first draw; draw s0 + c exists below n_draws
    const size_t B = (size_t)a.B;
    const uint32_t traj = (uint32_t)(a.traj_offset + (uint64_t)b);
    const int K = keep ? n_keep : a.N + 1;

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
    double Q[P][P], R[P][P];                                                // the pair of step n -> n + 1 (none is read for N = 1)
    if (a.N >= 2) {
        load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, a.N - 1, blk, b, mf, Sf);
        grid_load_pair<P>(g, a.B, a.D, grid_slot(g, a.N - 1), blk, b, Q, R);
    }
    for (int n = a.N - 1; n >= 1; --n) {
        // software prefetch of the next (earlier) filtered state and its step's pair while this step computes
        double mfn[P], Sfn[P][P], Qn[P][P], Rn[P][P];
        if (n >= 2) {
            load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, n - 1, blk, b, mfn, Sfn);
            grid_load_pair<P>(g, a.B, a.D, grid_slot(g, n - 1), blk, b, Qn, Rn);
        }
        double mp[P], G[P][P];
        {
            double Sp[P][P], T[P][P], Ssim[P][P];
            predict_block<P>(Q, R, mf, Sf, mp, Sp);      // pred[n+1] re-evaluated from filt[n] and the pair of step n
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
                for (int j = 0; j < P; ++j) {
                    Sf[i][j] = Sfn[i][j];
                    Q[i][j] = Qn[i][j];
                    R[i][j] = Rn[i][j];
                }
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
// Every (P, C) instance ships: the rule is check_code_objects.py's, at most 2048 B of scratch per lane, and the nearest, (6, 4),
// takes 1884 B (profiles/grid_draws_code_objects.txt has every instance next to bwd_sim_draws_kernel<P, C> and
// grid_bwd_sim_kernel<P>).  Should one cross it, the dispatch below is where its chunk is capped: the
// draws do not depend on the chunk, so a cap is not visible.

// Is this configuration served?  Decided on the configuration (and, for DALTON, n_bobs; < 0: the plain form) alone: RK_OK,
// RK_ERR_INVALID (sizes, the layout flag) or RK_ERR_UNSUPPORTED.  grid_check's / dalton_grid_check's limits (grid.hip,
// dalton_grid.hip) joined with sim_draws_check's (sim_draws.hip), on grid_entry.hpp's pieces.
static int grid_draws_check(const rk_solve_cfg* c, int n_bobs) {
    const bool dalton = n_bobs >= 0;
    int rc = grid_sizes_check("grid_draws", c);
    if (rc) return rc;
    rc = grid_served_check({"grid_draws", "the backward kernel reads batch-minor filtered records", RK_INTERROGATE_KRAMER,
                            "its forward pass depends on the key, so the draws cannot share one filter", GRID_DRAWS_PMIN,
                            GRID_DRAWS_PMAX, GRID_DRAWS_PMAX_THREE_BLOCKS}, c);
    if (rc) return rc;
    RK_REQUIRE(!dalton || (n_bobs >= 1 && n_bobs <= 3), RK_ERR_UNSUPPORTED, "grid_draws: n_bobs in 1..3, got %d", n_bobs);
    rc = grid_rhs_check("grid_draws", c, dalton ? "dalton_grid" : "grid");  // (the forward pass is theirs: their rule, our name)
    if (rc) return rc;
    RK_REQUIRE(!dalton || !dalton_grid_left_out(c, n_bobs, true), RK_ERR_UNSUPPORTED,
               "grid_draws: the store form of dalton_grid's filter for rhs %d at n_bstate %d with n_bobs %d is left out", c->rhs_id,
               c->n_bstate, n_bobs);
    return RK_OK;
}

// n_draws and n_keep, the second thing both entries look at
static int grid_draws_counts(const rk_solve_cfg* c, int n_draws, const int32_t* keep, int n_keep) {
    // (65535 chunks: the grid's second dimension)
    RK_REQUIRE(n_draws >= 1 && n_draws <= 65535, RK_ERR_INVALID, "grid_draws: n_draws must be in 1..65535, got %d", n_draws);
    RK_REQUIRE(!keep || (n_keep >= 1 && n_keep <= c->n_steps + 1), RK_ERR_INVALID,
               "grid_draws: n_keep must be in 1..n_steps + 1 = %d, got %d", c->n_steps + 1, n_keep);
    return RK_OK;
}

template <int C>
static int launch_grid_draws_chunk(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& ga, int n_draws,
                                   const int32_t* keep, int n_keep, double* x_draws) {
    LaunchGeom g = bwd_lane_geom(a.B, a.D);
    g.grid.y = div_up(n_draws, C);
    LaunchTimer t(h, "grid_bwd_sim_draws_kernel");
    const bool ok = dispatch_int<GRID_DRAWS_PMIN, GRID_DRAWS_PMAX>(c->n_bstate, [&](auto P) {
        hipLaunchKernelGGL((grid_bwd_sim_draws_kernel<P, C>), g.grid, g.block, 0, h->stream, a, ga, n_draws, keep, n_keep, x_draws);
    });
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "grid_draws: no backward kernel for n_bstate %d", c->n_bstate);
    t.stop();
    RK_HIP(hipGetLastError());
    return RK_OK;
}

static int launch_grid_draws(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& ga, int n_draws,
                             const int32_t* keep, int n_keep, double* x_draws) {
    switch (sim_draws_chunk(h, c, n_draws)) {
        case 1: return launch_grid_draws_chunk<1>(h, c, a, ga, n_draws, keep, n_keep, x_draws);
        case 2: return launch_grid_draws_chunk<2>(h, c, a, ga, n_draws, keep, n_keep, x_draws);
        default: return launch_grid_draws_chunk<SIM_DRAWS_CHUNK>(h, c, a, ga, n_draws, keep, n_keep, x_draws);
    }
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_solve_sim_draws_grid(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out,
                            const rk_grid_in* g, int32_t n_draws, const int32_t* keep, int32_t n_keep, double* x_draws) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_solve_sim_draws_grid: null cfg");
    int rc = grid_draws_check(c, -1);                               // (the configuration alone, before anything else is looked at)
    if (rc) return rc;
    rc = grid_draws_counts(c, n_draws, keep, n_keep);
    if (rc) return rc;
    RK_REQUIRE(h && out && g && x_draws, RK_ERR_INVALID, "rk_solve_sim_draws_grid: null argument");
    GridArgs ga;
    rc = grid_args("rk_solve_sim_draws_grid", g, ga);
    if (rc) return rc;
    rc = check_cfg(c, in);
    if (rc) return rc;
    rc = grid_out_check("rk_solve_sim_draws_grid", out, RK_MODE_MV);    // (the draws go to x_draws)
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, out, a);
    rc = launch_grid_forward(h, c, a, ga);                          // grid.hip's forward pass, built-in or hiprtc
    if (rc) return rc;
    return launch_grid_draws(h, c, a, ga, n_draws, keep, n_keep, x_draws);
}

int rk_dalton_grid_sim_draws(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out,
                             const double* obs, const double* obs_weight, const double* obs_var, const int32_t* obs_ind,
                             int32_t n_obs, int32_t n_bobs, const rk_grid_in* g, int32_t n_draws, const int32_t* keep,
                             int32_t n_keep, double* x_draws) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_dalton_grid_sim_draws: null cfg");
    RK_REQUIRE(n_bobs >= 0, RK_ERR_UNSUPPORTED, "grid_draws: n_bobs in 1..3, got %d", n_bobs);
    int rc = grid_draws_check(c, n_bobs);
    if (rc) return rc;
    rc = grid_draws_counts(c, n_draws, keep, n_keep);
    if (rc) return rc;
    RK_REQUIRE(h && out && g && x_draws, RK_ERR_INVALID, "rk_dalton_grid_sim_draws: null argument");
    DaltonObs o;
    GridArgs ga;
    rc = dalton_grid_inputs("rk_dalton_grid_sim_draws", c, in, obs, obs_weight, obs_var, obs_ind, n_obs, g, o, ga);
    if (rc) return rc;
    rc = grid_out_check("rk_dalton_grid_sim_draws", out, RK_MODE_MV);
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, out, a);
    rc = dalton_grid_store_forward(h, c, a, o, ga, n_bobs);         // dalton_grid.hip's joint filter, its store form
    if (rc) return rc;
    return launch_grid_draws(h, c, a, ga, n_draws, keep, n_keep, x_draws);
}

}  // extern "C"
