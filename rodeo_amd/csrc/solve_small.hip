// The lane-per-trajectory solver in the covariance form and the solver's C entries.  Kernels (n_bmeas = 1; forward n_bstate <= 6,
// backward <= 9): the fused time loops of
//   src/rodeo/solve.py:31-122   _solve_filter   -> fwd_kernel      (solve_small_kernels.hpp, also built at run time)
//   src/rodeo/solve.py:257-301  solve_mv        -> bwd_mv_kernel   (in place over the filtered moments)
//   src/rodeo/solve.py:162-204  solve_sim       -> bwd_sim_kernel
// and gauss_logpost_kernel, the Gaussian observation log-posterior of a sampled path.  Host side: the argument block and
// checks every path shares (make_args, check_cfg, begin_solve), and rk_solve_filter / _mv / _sim, rk_solve_layout / _sizes /
// _workspace_bytes, rk_solve_sim_logpost, rk_interrogate_batched, rk_gauss_obs_logpost, which route a configuration to its
// path (solve_paths.hpp).  Fenrir is in fenrir.hip.
// The whole N-step recursion of a trajectory runs inside ONE kernel launch; the state lives in VGPRs and only the
// filtered / smoothed moments touch HBM, in the batch-minor layout of include/rodeo_kalman.h (512 B per wave per
// element row).  Predicted moments are re-evaluated from the filtered ones in the backward pass instead of being
// stored (they are a pure function of filt[n], Q, R: standard.py:57-59): bwd_walk of lane_backward.hpp under StaticPrior.
#include "common.hpp"
#include "kalman_small.hpp"
#include "philox.hpp"
#include "rhs.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "solve_small_kernels.hpp"
#include "tile3_pack.hpp"
#include "lane_backward.hpp"

namespace rk {

// ---- backward passes: one lane per (block, trajectory) -----------------------------------------------------------
template <int P>
__global__ void __launch_bounds__(64) bwd_mv_kernel(SolveArgs a) {
    BwdLane<P> ln;
    if (ln.init(a)) bwd_smooth_lane<P>(a, ln, StaticPrior<P>{});
}

template <int P>
__global__ void __launch_bounds__(64) bwd_sim_kernel(SolveArgs a) {
    BwdLane<P> ln;
    if (ln.init(a)) bwd_sample_lane<P>(a, ln, StaticPrior<P>{});
}

// ---- Gaussian observation log-posterior reduction (docs/examples/parameter.md:188-210) ---------------------------
// One wave per trajectory: the n_obs x n_block observation terms are spread over the 64 lanes (a fixed stride-64 assignment
// and a fixed xor tree, so the value does not depend on the launch), where one lane per trajectory walked its 82 strided
// loads one after the other on 16 waves in all (C4: 36 us of a 306 us evaluation; now 6).
// (`packed`: RK_LAYOUT_TILE3_PACKED -- the mean of a packed record is its slot 6, tile3_pack.hpp)
__global__ void __launch_bounds__(64) gauss_logpost_kernel(int B, int n_steps, int D, int P, int tile, int tile_off, bool packed, const double* x,
                                                           const double* obs, const int32_t* obs_ind, int n_obs, double noise_sd,
                                                           const double* upars, int n_prior, double prior_sd, double* out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const double LOG_SQRT_2PI = 0.91893853320467274178;
    const double lsd = log(noise_sd);
    double acc = 0.0;
    for (int e = lane; e < n_obs * D; e += 64) {
        const int k = e / D, blk = e - k * D;
        int ni = obs_ind[k];
        ni = ni < 0 ? 0 : (ni > n_steps ? n_steps : ni);     // never index outside the (N+1)-long path
        const size_t n = (size_t)ni;
        const long long n_tiles = (long long)B * D, tau = (long long)b * D + blk;
        const double xv = packed && tile3_pack_record(n_steps, n_tiles, ni, tau)
                              ? x[tile3_pack_index(n_tiles, ni, tau, tile3_pack_slot(0, 3))]
                              : tile ? x[((n * B + b) * D + blk) * tile + tile_off]      // mu_0 inside the tile
                                     : x[((n * D + blk) * P + 0) * (size_t)B + b];
        const double zz = (obs[e] - xv) / noise_sd;
        acc += -0.5 * zz * zz - lsd - LOG_SQRT_2PI;           // scipy.stats.norm.logpdf
    }
    if (upars) {
        const double lps = log(prior_sd);
        for (int k = lane; k < n_prior; k += 64) {
            const double zz = upars[(size_t)k * B + b] / prior_sd;
            acc += -0.5 * zz * zz - lps - LOG_SQRT_2PI;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if (lane == 0) out[b] = acc;
}

// ---- dispatch ---------------------------------------------------------------------------------------------------
int make_args(const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, SolveArgs& a) {
    a.B = c->n_traj; a.N = c->n_steps; a.D = c->n_block;
    a.t_min = c->t_min; a.t_max = c->t_max; a.seed = c->seed; a.traj_offset = c->traj_offset;
    a.W = in->ode_weight; a.W_b = in->ode_weight_batched;
    a.x0 = in->ode_init; a.x0_b = in->ode_init_batched;
    a.Q = in->prior_weight; a.Q_b = in->prior_weight_batched;
    a.R = in->prior_var; a.R_b = in->prior_var_batched;
    a.theta = in->theta; a.theta_b = in->theta_batched;
    a.mean = out ? out->mean_state : nullptr; a.var = out ? out->var_state : nullptr;
    a.mean_pred = out ? out->mean_pred : nullptr; a.var_pred = out ? out->var_pred : nullptr;
    a.x = out ? out->x_state : nullptr;
    return RK_OK;
}

int check_cfg(const rk_solve_cfg* c, const rk_solve_in* in) {
    RK_REQUIRE(c && in, RK_ERR_INVALID, "null cfg / in");
    RK_REQUIRE(c->n_traj >= 1 && c->n_steps >= 1 && c->n_block >= 1 && c->n_bstate >= 1 && c->n_bmeas >= 1,
               RK_ERR_INVALID, "non-positive dimension (n_traj=%d n_steps=%d n_block=%d n_bstate=%d n_bmeas=%d)",
               c->n_traj, c->n_steps, c->n_block, c->n_bstate, c->n_bmeas);
    RK_REQUIRE(in->ode_weight && in->ode_init && in->prior_weight && in->prior_var, RK_ERR_INVALID,
               "ode_weight / ode_init / prior_weight / prior_var must not be NULL");
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD || c->kalman_type == RK_KALMAN_SQRT, RK_ERR_UNSUPPORTED,
               "unknown kalman_type %d", c->kalman_type);
    RK_REQUIRE(c->interrogate >= 0 && c->interrogate <= 3, RK_ERR_UNSUPPORTED, "unknown interrogate id %d",
               c->interrogate);
    return RK_OK;
}

template <class RHS>
static int launch_fwd_rhs(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a) {
    RK_REQUIRE(c->n_block == RHS::D && c->n_bmeas == 1, RK_ERR_UNSUPPORTED,
               "rhs %d needs n_block=%d, n_bmeas=1 (got %d, %d)", c->rhs_id, RHS::D, c->n_block, c->n_bmeas);
    const int rc = check_n_theta<RHS>(c, a);
    if (rc) return rc;
    const bool sp = (c->flags & RK_FLAG_STORE_PRED) != 0;
    const LaunchGeom g = fwd_lane_geom(a.B);
    bool itg_ok = false;
    const bool p_ok = dispatch_int<2, 6>(c->n_bstate, [&](auto P) {
        itg_ok = dispatch_int<RK_INTERROGATE_RODEO, RK_INTERROGATE_CHKREBTII>(c->interrogate, [&](auto I) {
            LaunchTimer t(h, "fwd_kernel");
            if (sp) hipLaunchKernelGGL((fwd_kernel<RHS, P, I, true>), g.grid, g.block, 0, h->stream, a);
            else hipLaunchKernelGGL((fwd_kernel<RHS, P, I, false>), g.grid, g.block, 0, h->stream, a);
            t.stop();
        });
    });
    RK_REQUIRE(p_ok, RK_ERR_UNSUPPORTED, "lane-per-trajectory path supports n_bstate in [2, 6] (the blocked tile path 4 .. 8 without "
               "RK_FLAG_STORE_PRED / RK_FLAG_BATCH_MINOR), got %d", c->n_bstate);
    RK_REQUIRE(itg_ok, RK_ERR_UNSUPPORTED, "unknown interrogate id %d", c->interrogate);
    RK_HIP(hipGetLastError());
    return RK_OK;
}

static int small_forward(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a) {
    if (is_user_rhs(c->rhs_id)) return user_forward(h, c, a);
    int rc = RK_ERR_UNSUPPORTED;
    if (!with_builtin_rhs(c->rhs_id, [&](auto rhs) { rc = launch_fwd_rhs<decltype(rhs)>(h, c, a); }))
        set_error("unknown rhs_id %d for the small-block path", c->rhs_id);
    return rc;
}

template <bool SIM>
static int small_backward(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a) {
    const LaunchGeom g = bwd_lane_geom(a.B, a.D);
    LaunchTimer t(h, SIM ? "bwd_sim_kernel" : "bwd_mv_kernel");
    const bool ok = dispatch_int<2, 9>(c->n_bstate, [&](auto P) {
        if (SIM) hipLaunchKernelGGL((bwd_sim_kernel<P>), g.grid, g.block, 0, h->stream, a);
        else hipLaunchKernelGGL((bwd_mv_kernel<P>), g.grid, g.block, 0, h->stream, a);
    });
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "small-block path supports n_bstate in [2, 9] for the backward pass, got %d", c->n_bstate);
    t.stop();
    RK_HIP(hipGetLastError());
    return RK_OK;
}

// the lane-per-trajectory smoothing (RK_MODE_MV) or sampling (RK_MODE_SIM) pass over batch-minor filtered moments
int small_backward_pass(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, int mode) {
    return mode == RK_MODE_SIM ? small_backward<true>(h, c, a) : small_backward<false>(h, c, a);
}

template <class RHS>
static int launch_itg_rhs(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, double t, int step,
                          const double* mp, const double* vp, double* wm, double* mm_, double* vm) {
    RK_REQUIRE(c->n_block == RHS::D && c->n_bmeas == 1, RK_ERR_UNSUPPORTED,
               "rhs %d needs n_block=%d, n_bmeas=1 (got %d, %d)", c->rhs_id, RHS::D, c->n_block, c->n_bmeas);
    const LaunchGeom g = fwd_lane_geom(a.B);
    const int sqrt_mode = c->kalman_type == RK_KALMAN_SQRT ? 1 : 0;      // only interrogate_chkrebtii reads it
    const bool ok = dispatch_int<2, 6>(c->n_bstate, [&](auto P) {
        dispatch_int<RK_INTERROGATE_RODEO, RK_INTERROGATE_CHKREBTII>(c->interrogate, [&](auto I) {
            hipLaunchKernelGGL((interrogate_kernel<RHS, P, I>), g.grid, g.block, 0, h->stream, a, t, step, mp, vp, wm, mm_, vm, sqrt_mode);
        });
    });
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "rk_interrogate_batched supports n_bstate in [2, 6], got %d", c->n_bstate);
    RK_HIP(hipGetLastError());
    return RK_OK;
}

int begin_solve(rk_handle h) {
    RK_HIP(hipSetDevice(h->device));
    if (!h->profile_keep) { h->prof.clear(); h->event_used = 0; }
    return RK_OK;
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_solve_layout(const rk_solve_cfg* c, int32_t mode, int32_t* layout) {
    RK_REQUIRE(c && layout, RK_ERR_INVALID, "rk_solve_layout: null argument");
    RK_REQUIRE(mode >= RK_MODE_FILTER && mode <= RK_MODE_SIM, RK_ERR_INVALID, "rk_solve_layout: bad mode %d", mode);
    *layout = path_layout(solve_path(c, mode), c, mode);
    return RK_OK;
}

int rk_tile3_packed_waves(int32_t n_steps, int32_t n_tiles) { return tile3_pack_waves(n_steps, n_tiles); }

int rk_solve_workspace_bytes(const rk_solve_cfg* c, int32_t mode, size_t* bytes) {
    RK_REQUIRE(c && bytes, RK_ERR_INVALID, "rk_solve_workspace_bytes: null argument");
    switch (solve_path(c, mode)) {
        case SolvePath::Dense: *bytes = dense_ws_bytes(c, mode); break;
        case SolvePath::Sqrt: *bytes = sqrt_ws_doubles(c, mode) * sizeof(double); break;     // optional (solve_sqrt.hip)
        case SolvePath::TileN: *bytes = tilen_ws_doubles(c, mode) * sizeof(double); break;
        default: *bytes = 0;
    }
    return RK_OK;
}

int rk_solve_sizes(const rk_solve_cfg* c, int32_t layout, size_t* mean_bytes, size_t* var_bytes) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_solve_sizes: null cfg");
    const size_t m = (size_t)(c->n_steps + 1) * c->n_block * c->n_bstate * (size_t)c->n_traj * sizeof(double);
    if (layout == RK_LAYOUT_TILE3 || layout == RK_LAYOUT_TILE3_PACKED) {            // one size: the packed records lie in place
        RK_REQUIRE(c->n_bstate == 3, RK_ERR_INVALID, "RK_LAYOUT_TILE3 needs n_bstate = 3");
        if (mean_bytes) *mean_bytes = 0;
        if (var_bytes) {
            const size_t n_tiles = (size_t)c->n_block * (size_t)c->n_traj;
            *var_bytes = ((size_t)(c->n_steps + 1) * n_tiles * 12 + ((n_tiles + 7) / 8) * 128) * sizeof(double);
        }
        return RK_OK;
    }
    if (layout == RK_LAYOUT_TILE4) {
        RK_REQUIRE(c->n_bstate == 4, RK_ERR_INVALID, "RK_LAYOUT_TILE4 needs n_bstate = 4");
        if (mean_bytes) *mean_bytes = 0;
        if (var_bytes) *var_bytes = tile4_doubles(c) * sizeof(double);
        return RK_OK;
    }
    if (layout == RK_LAYOUT_TILEP) {
        RK_REQUIRE(c->n_bstate >= 4 && c->n_bstate <= 8, RK_ERR_INVALID, "RK_LAYOUT_TILEP needs n_bstate in 4..8");
        if (mean_bytes) *mean_bytes = 0;
        if (var_bytes) *var_bytes = tilen_tile_doubles(c) * sizeof(double);
        return RK_OK;
    }
    RK_REQUIRE(layout == RK_LAYOUT_BATCH_MINOR || layout == RK_LAYOUT_TRAJ_MAJOR, RK_ERR_INVALID, "unknown layout %d", layout);
    if (mean_bytes) *mean_bytes = m;
    if (var_bytes) *var_bytes = m * c->n_bstate;
    return RK_OK;
}

static int solve_common(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out,
                        int mode /*0 filter, 1 mv, 2 sim*/) {
    RK_REQUIRE(h, RK_ERR_INVALID, "null handle");
    int rc = check_cfg(c, in);
    if (rc) return rc;
    const SolvePath path = solve_path(c, mode);
    const bool tile = path == SolvePath::Tile3 || path == SolvePath::Tile4 || path == SolvePath::TileN;
    RK_REQUIRE(out && out->var_state && (tile || out->mean_state), RK_ERR_INVALID,
               "out->mean_state / var_state must not be NULL");
    if (path == SolvePath::Dense) {
        rc = dense_check(c, in, mode);
        if (rc) return rc;
        rc = begin_solve(h);
        if (rc) return rc;
        return dense_solve(h, c, in, out, mode);
    }
    RK_REQUIRE(!(c->flags & RK_FLAG_STORE_PRED) || (out->mean_pred && out->var_pred), RK_ERR_INVALID,
               "RK_FLAG_STORE_PRED needs out->mean_pred / var_pred");
    RK_REQUIRE(mode != 2 || out->x_state, RK_ERR_INVALID, "rk_solve_sim needs out->x_state");
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, out, a);
    switch (path) {
        case SolvePath::Sqrt: return sqrt_solve(h, c, a, mode, (double*)out->workspace, out->workspace_bytes);
        case SolvePath::Tile4: return tile4_solve(h, c, a, out->var_state, mode);
        case SolvePath::Tile3: return tile3_solve(h, c, a, out->var_state, mode);
        case SolvePath::TileN: return tilen_solve(h, c, a, out->var_state, (double*)out->workspace, out->workspace_bytes, mode);
        default: break;
    }
    rc = small_forward(h, c, a);
    if (rc) return rc;
    if (mode == 1) rc = small_backward<false>(h, c, a);
    if (mode == 2) rc = small_backward<true>(h, c, a);
    return rc;
}

int rk_solve_filter(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out) {
    return solve_common(h, c, in, out, 0);
}
int rk_solve_mv(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out) {
    return solve_common(h, c, in, out, 1);
}
int rk_solve_sim(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out) {
    return solve_common(h, c, in, out, 2);
}

int rk_gauss_obs_logpost(rk_handle h, int32_t n_traj, int32_t n_steps, int32_t n_block, int32_t n_bstate,
                         int32_t layout, const double* x_state, const double* obs, const int32_t* obs_ind,
                         int32_t n_obs, double noise_sd, const double* upars, int32_t n_prior, double prior_sd,
                         double* logpost);

int rk_solve_sim_logpost(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out,
                         const double* obs, const int32_t* obs_ind, int32_t n_obs, double noise_sd,
                         const double* upars, int32_t n_prior, double prior_sd, double* logpost) {
    RK_REQUIRE(h, RK_ERR_INVALID, "null handle");
    RK_REQUIRE(logpost && n_obs >= 0 && (n_obs == 0 || (obs && obs_ind)), RK_ERR_INVALID,
               "rk_solve_sim_logpost: null obs / obs_ind / logpost");      // (no observation: prior only, obs / obs_ind are not read)
    RK_REQUIRE(!upars || n_prior >= 0, RK_ERR_INVALID, "rk_solve_sim_logpost: n_prior < 0");
    int rc = check_cfg(c, in);
    if (rc) return rc;
    // (tile3_sim_logpost_supported first: it implies the tile3 route, so solve_path stops there)
    if (tile3_sim_logpost_supported(c, n_obs) && solve_path(c, RK_MODE_SIM) == SolvePath::Tile3) {
        // the sampler's consumer wave reduces the log-posterior itself; out->x_state may be NULL (no path is stored)
        RK_REQUIRE(out && out->var_state, RK_ERR_INVALID, "out->var_state must not be NULL");
        rc = begin_solve(h);
        if (rc) return rc;
        SolveArgs a;
        make_args(c, in, out, a);
        return tile3_solve_sim_logpost(h, c, a, out->var_state, obs, obs_ind, n_obs, noise_sd, upars, n_prior, prior_sd, logpost);
    }
    // any other configuration: the sampler, then the reduction kernel on its path (one call, no host work in between)
    RK_REQUIRE(out && out->x_state, RK_ERR_INVALID, "rk_solve_sim_logpost: this configuration needs out->x_state");
    rc = solve_common(h, c, in, out, 2);
    if (rc) return rc;
    const bool keep = h->profile_keep;
    h->profile_keep = true;                            // (keep the sampler's kernel times next to the reduction's)
    rc = rk_gauss_obs_logpost(h, c->n_traj, c->n_steps, c->n_block, c->n_bstate, RK_LAYOUT_BATCH_MINOR, out->x_state, obs,
                              obs_ind, n_obs, noise_sd, upars, n_prior, prior_sd, logpost);
    h->profile_keep = keep;
    return rc;
}

int rk_interrogate_batched(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, double t, int32_t step,
                           const double* mean_state_pred, const double* var_state_pred, double* wgt_meas,
                           double* mean_meas, double* var_meas) {
    RK_REQUIRE(h, RK_ERR_INVALID, "null handle");
    RK_REQUIRE(c && in && in->ode_weight, RK_ERR_INVALID, "rk_interrogate_batched: null cfg / in / ode_weight");
    RK_REQUIRE(mean_state_pred && var_state_pred && wgt_meas && mean_meas && var_meas, RK_ERR_INVALID,
               "rk_interrogate_batched: null array");
    RK_REQUIRE(c->n_traj >= 1, RK_ERR_INVALID, "rk_interrogate_batched: n_traj must be positive");
    RK_HIP(hipSetDevice(h->device));
    SolveArgs a;
    make_args(c, in, nullptr, a);
    if (is_user_rhs(c->rhs_id))
        return user_interrogate(h, c, a, t, step, mean_state_pred, var_state_pred, wgt_meas, mean_meas, var_meas);
    int rc = RK_ERR_UNSUPPORTED;
    if (!with_builtin_rhs(c->rhs_id, [&](auto rhs) {
            rc = launch_itg_rhs<decltype(rhs)>(h, c, a, t, step, mean_state_pred, var_state_pred, wgt_meas, mean_meas, var_meas);
        }))
        set_error("unknown rhs_id %d", c->rhs_id);
    return rc;
}

int rk_gauss_obs_logpost(rk_handle h, int32_t n_traj, int32_t n_steps, int32_t n_block, int32_t n_bstate,
                         int32_t layout, const double* x_state, const double* obs, const int32_t* obs_ind,
                         int32_t n_obs, double noise_sd, const double* upars, int32_t n_prior, double prior_sd,
                         double* logpost) {
    RK_REQUIRE(h && x_state && logpost && (n_obs <= 0 || (obs && obs_ind)), RK_ERR_INVALID, "rk_gauss_obs_logpost: null argument");
    const bool tile3 = layout == RK_LAYOUT_TILE3 || layout == RK_LAYOUT_TILE3_PACKED;
    RK_REQUIRE(layout == RK_LAYOUT_BATCH_MINOR || (tile3 && n_bstate == 3) ||
                   (layout == RK_LAYOUT_TILE4 && n_bstate == 4) || (layout == RK_LAYOUT_TILEP && n_bstate >= 4), RK_ERR_INVALID,
               "rk_gauss_obs_logpost: bad layout %d for n_bstate %d", layout, n_bstate);
    RK_REQUIRE(n_traj >= 1 && n_obs >= 0 && n_block >= 1 && n_bstate >= 1 && n_steps >= 1, RK_ERR_INVALID,
               "rk_gauss_obs_logpost: bad dimension");
    RK_HIP(hipSetDevice(h->device));
    LaunchTimer t(h, "gauss_logpost_kernel");
    hipLaunchKernelGGL(gauss_logpost_kernel, dim3(n_traj), dim3(64), 0, h->stream, n_traj, n_steps, n_block,
                       n_bstate, tile3 ? 12 : (layout == RK_LAYOUT_BATCH_MINOR ? 0 : n_bstate * (n_bstate + 1)),
                       tile3 ? 3 : n_bstate * n_bstate, layout == RK_LAYOUT_TILE3_PACKED, x_state, obs, obs_ind, n_obs, noise_sd, upars, n_prior, prior_sd, logpost);
    t.stop();
    RK_HIP(hipGetLastError());
    return RK_OK;
}

}  // extern "C"
