// fenrir_at: host side of rk_fenrir_backward_at, Fenrir's backward pass for Gaussian observations at
// arbitrary times, after rk_solve_filter with the same cfg / in.  Two launches: fenrir_at_hops_kernel (the hop records of every
// interval that holds an observation, time-parallel) and the chain kernel of the route the filter took:
//   tiles  -- fenrir_bwd_at_tile3_kernel (solve_tile3.hip): n_bstate = 3, n_bobs = 1, no flags, RK_LAYOUT_TILE3 records;
//   lanes  -- fenrir_bwd_at_kernel (fenrir_at_kernels.hpp): n_bstate 2..6, n_bobs 1..3, RK_FLAG_STORE_PRED | RK_FLAG_BATCH_MINOR.
// Both are fenrir's own chain kernels with the off-grid parts added: the tile one is an instance of the same body
// (fenrir_tile3_body), the lane one shares the Markov step and the conditioning (fenrir_kernels.hpp, dalton_observe).
#include "common.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "fenrir_at_kernels.hpp"

namespace rk {

// What is served and on which route, from the configuration alone (no handle, no pointer but cfg is looked at).
static int fenrir_at_route(const rk_solve_cfg* c, int n_bobs, bool* tile) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_fenrir_backward_at (fenrir_at): null cfg");
    RK_REQUIRE(c->kalman_type != RK_KALMAN_SQRT, RK_ERR_UNSUPPORTED,
               "fenrir_at: the square-root form is not built (kalman_type standard only)");
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD, RK_ERR_UNSUPPORTED, "fenrir_at: unknown kalman_type %d", c->kalman_type);
    RK_REQUIRE(n_bobs >= 1 && n_bobs <= 3, RK_ERR_UNSUPPORTED, "fenrir_at: n_bobs in 1..3, got %d", n_bobs);
    RK_REQUIRE(c->n_bstate >= 2 && c->n_bstate <= 6, RK_ERR_UNSUPPORTED, "fenrir_at: n_bstate in 2..6, got %d", c->n_bstate);
    RK_REQUIRE(c->n_traj >= 1 && c->n_steps >= 1 && c->n_block >= 1, RK_ERR_INVALID,
               "fenrir_at: non-positive dimension (n_traj=%d n_steps=%d n_block=%d)", c->n_traj, c->n_steps, c->n_block);
    const int both = RK_FLAG_STORE_PRED | RK_FLAG_BATCH_MINOR;
    if ((c->flags & both) == both) {
        *tile = false;
        return RK_OK;
    }
    RK_REQUIRE(!(c->flags & both), RK_ERR_INVALID,
               "fenrir_at: the lane route needs RK_FLAG_STORE_PRED and RK_FLAG_BATCH_MINOR together (flags = %d)", c->flags);
    RK_REQUIRE(n_bobs == 1 && solve_path(c, RK_MODE_FILTER) == SolvePath::Tile3, RK_ERR_UNSUPPORTED,
               "fenrir_at reads the RK_LAYOUT_TILE3 records (n_bstate = 3, n_bobs = 1) or the batch-minor filtered and predicted "
               "moments of a filter with RK_FLAG_STORE_PRED | RK_FLAG_BATCH_MINOR; this configuration (n_bstate %d, n_bobs %d, no "
               "flags) writes neither: the blocked-tile records are not served", c->n_bstate, n_bobs);
    *tile = true;
    return RK_OK;
}

static size_t fenrir_at_ws_doubles(const rk_solve_cfg* c, bool tile, int n_rec) {
    const size_t per = tile ? (size_t)FENRIR_AT_TILE_REC : (size_t)FenrirAtLaneRec(c->n_bstate).width;
    return (size_t)n_rec * c->n_block * per * (size_t)c->n_traj;
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_fenrir_at_workspace_bytes(const rk_solve_cfg* c, int32_t n_bobs, int32_t n_records, size_t* bytes) {
    bool tile = false;
    int rc = fenrir_at_route(c, n_bobs, &tile);
    if (rc) return rc;
    RK_REQUIRE(bytes && n_records >= 1, RK_ERR_INVALID, "rk_fenrir_at_workspace_bytes (fenrir_at): null bytes or n_records < 1");
    *bytes = sizeof(double) * fenrir_at_ws_doubles(c, tile, n_records);
    return RK_OK;
}

int rk_fenrir_backward_at(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, const double* obs,
                          const double* obs_weight, const double* obs_var, const rk_fenrir_at_in* at, int32_t n_obs,
                          int32_t n_bobs, void* workspace, double* logdens) {
    // what is not served is refused on the configuration alone, before the handle or any array is looked at
    bool tile = false;
    int rc = fenrir_at_route(c, n_bobs, &tile);
    if (rc) return rc;
    RK_REQUIRE(h && in && out && at && workspace && logdens, RK_ERR_INVALID, "rk_fenrir_backward_at (fenrir_at): null argument");
    RK_REQUIRE(n_obs >= 1 && obs && obs_weight && obs_var && at->table, RK_ERR_INVALID,
               "fenrir_at: null observation array or table, or n_obs < 1");
    RK_REQUIRE(at->n_pre >= 1 && at->n_post >= 1 && at->pre_trans && at->pre_noise && at->post_trans && at->post_noise,
               RK_ERR_INVALID, "fenrir_at: n_pre and n_post must be at least 1 and the four prior arrays present, got %d, %d",
               at->n_pre, at->n_post);
    RK_REQUIRE(out->var_state && (tile || (out->mean_state && out->mean_pred && out->var_pred)), RK_ERR_INVALID,
               "fenrir_at: the output of rk_solve_filter is missing (tiles: var_state; lanes: the filtered and predicted moments)");
    SolveArgs a;
    rc = make_args(c, in, out, a);
    if (rc) return rc;
    FenrirAt f;
    f.obs = obs; f.obs_w = obs_weight; f.obs_v = obs_var; f.tab = at->table;
    f.n_obs = n_obs; f.n_pre = at->n_pre; f.n_post = at->n_post; f.prior_b = at->prior_batched ? 1 : 0;
    f.pre_q = at->pre_trans; f.pre_r = at->pre_noise; f.post_q = at->post_trans; f.post_r = at->post_noise;
    f.hops = (double*)workspace; f.logdens = logdens;
    RK_HIP(hipSetDevice(h->device));
    RK_HIP(hipMemsetAsync(logdens, 0, sizeof(double) * (size_t)c->n_traj, h->stream));
    const dim3 hgrid(2 * n_obs * div_up(a.B * a.D, 64)), grid(div_up(a.B * a.D, 64)), block(64);
    if (tile) {
        LaunchTimer t(h, "fenrir_at_hops_kernel");
        hipLaunchKernelGGL((fenrir_at_hops_kernel<3, RK_LAYOUT_TILE3>), hgrid, block, 0, h->stream, a, f);
        t.stop();
        RK_HIP(hipGetLastError());
        return tile3_fenrir_backward_at(h, a, out->var_state, f);
    }
    bool ok = false;
    dispatch_int<2, 6>(c->n_bstate, [&](auto P) {
        {
            LaunchTimer t(h, "fenrir_at_hops_kernel");
            hipLaunchKernelGGL((fenrir_at_hops_kernel<P, RK_LAYOUT_BATCH_MINOR>), hgrid, block, 0, h->stream, a, f);
            t.stop();
        }
        dispatch_int<1, 3>(n_bobs, [&](auto M) {
            LaunchTimer t(h, "fenrir_bwd_at_kernel");
            hipLaunchKernelGGL((fenrir_bwd_at_kernel<P, M>), grid, block, 0, h->stream, a, f);
            t.stop();
            ok = true;
        });
    });
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "fenrir_at: no kernel for n_bstate %d, n_bobs %d", c->n_bstate, n_bobs);
    RK_HIP(hipGetLastError());
    return RK_OK;
}

}  // extern "C"
