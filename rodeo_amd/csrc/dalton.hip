// DALTON for Gaussian observations (src/rodeo/inference/dalton.py:39-545): host side of rk_dalton_layout /
// rk_dalton_loglik / rk_dalton_solve.  Two routes for the forward filters:
//   tiles  -- dalton_fwd_tile3_kernel (dalton_tile3_kernels.hpp): n_bstate = 3, n_bobs = 1, n_block 1..4, a configuration of
//             fwd_tile3_kernel (rodeo / schober / kramer); writes RK_LAYOUT_TILE3 records;
//   lanes  -- dalton_fwd_kernel (dalton_kernels.hpp): everything else with n_bstate 2..6, n_bobs 1..3; batch-minor moments.
// RK_DALTON_LANES=1 forces the lane route where the tile route exists (cross-checks).  The smoothing and sampling passes
// of rk_dalton_solve are the solver's own on either route (dalton.py:416-460 / :514-545 are solve.py:257-302 / :162-204,
// same indices).
#include <cstdlib>
#include "common.hpp"
#include "rhs.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "dalton_kernels.hpp"
#include "dalton_tile3_kernels.hpp"

namespace rk {

// Is this configuration served?  RK_OK, or RK_ERR_UNSUPPORTED with the reason.
static int dalton_check(const rk_solve_cfg* c, int n_bobs) {
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD, RK_ERR_UNSUPPORTED,
               "dalton: kalman_type %d is not built (only the standard form)", c->kalman_type);
    RK_REQUIRE(c->interrogate >= RK_INTERROGATE_RODEO && c->interrogate <= RK_INTERROGATE_KRAMER, RK_ERR_UNSUPPORTED,
               "dalton: interrogate id %d is not supported (rodeo, schober, kramer)", c->interrogate);
    RK_REQUIRE(c->n_bmeas == 1, RK_ERR_UNSUPPORTED, "dalton: n_bmeas = 1 only, got %d", c->n_bmeas);
    RK_REQUIRE(c->n_bstate >= 2 && c->n_bstate <= 6, RK_ERR_UNSUPPORTED, "dalton: n_bstate in 2..6, got %d", c->n_bstate);
    RK_REQUIRE(n_bobs >= 1 && n_bobs <= 3, RK_ERR_UNSUPPORTED, "dalton: n_bobs in 1..3, got %d", n_bobs);
    if (is_user_rhs(c->rhs_id)) {
        const int rc = user_rhs_check(c);
        if (rc) return rc;
        // the register budget of the built-in instances (dalton_pmax): three or more blocks stop at n_bstate = 5
        RK_REQUIRE(c->n_block < 3 || c->n_bstate <= 5, RK_ERR_UNSUPPORTED,
                   "dalton: n_bstate up to 5 with three or more blocks (the lane kernel spills), got %d", c->n_bstate);
        return RK_OK;
    }
    bool known = false, fits = false;
    int pmax = 6;
    with_builtin_rhs(c->rhs_id, [&](auto rhs) {
        known = true;
        fits = decltype(rhs)::D == c->n_block;
        pmax = dalton_pmax<decltype(rhs)>();
    });
    RK_REQUIRE(known, RK_ERR_UNSUPPORTED, "dalton: unknown rhs_id %d", c->rhs_id);
    RK_REQUIRE(fits, RK_ERR_UNSUPPORTED, "dalton: rhs %d needs another n_block than %d", c->rhs_id, c->n_block);
    RK_REQUIRE(c->n_bstate <= pmax, RK_ERR_UNSUPPORTED, "dalton: rhs %d supports n_bstate up to %d, got %d", c->rhs_id, pmax,
               c->n_bstate);
    return RK_OK;
}

// Does the tile route serve this (served, dalton_check) configuration?  Decided on the configuration without flags: the
// layout is what the filter writes, whatever layout the caller's flags ask of the plain solver.
static bool dalton_tile_route(const rk_solve_cfg* c, int n_bobs) {
    if (n_bobs != 1 || c->n_bstate != 3 || c->n_block > 4 || c->interrogate > RK_INTERROGATE_KRAMER) return false;
    const char* e = getenv("RK_DALTON_LANES");
    if (e && atoi(e) != 0) return false;
    rk_solve_cfg plain = *c;
    plain.flags = 0;
    return tile3_supported(&plain, RK_MODE_FILTER);
}

// one launch of dalton_fwd_tile3_kernel<RHS, ITG, STORE> for a built-in right-hand side (tile3_supported: n_block 1..3)
template <class RHS, bool STORE>
static int launch_dalton_tile_rhs(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, double* out) {
    if constexpr (RHS::D > 4 || RHS::NDEP != 1) {
        set_error("dalton: rhs %d has no tile form", c->rhs_id);
        return RK_ERR_UNSUPPORTED;
    } else {
        const LaunchGeom g = dalton_tile_geom(a.B, RHS::D, !STORE);
        bool ok = false;
        dispatch_int<RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(c->interrogate, [&](auto I) {
            LaunchTimer t(h, STORE ? "dalton_fwd_tile3_kernel<store>" : "dalton_fwd_tile3_kernel<loglik>");
            hipLaunchKernelGGL((dalton_fwd_tile3_kernel<RHS, I, STORE>), g.grid, g.block, 0, h->stream, a, o, out);
            t.stop();
            ok = true;
        });
        RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "dalton: interrogate %d has no tile kernel", c->interrogate);
        RK_HIP(hipGetLastError());
        return RK_OK;
    }
}

// one launch of dalton_fwd_kernel<RHS, P, ITG, n_bobs, STORE> for a built-in right-hand side
template <class RHS, bool STORE>
static int launch_dalton_rhs(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, int n_bobs,
                             double* logdens) {
    const LaunchGeom g = dalton_lane_geom(a.B, !STORE);
    bool ok = false;
    dispatch_int<2, dalton_pmax<RHS>()>(c->n_bstate, [&](auto P) {
        dispatch_int<RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(c->interrogate, [&](auto I) {
            dispatch_int<1, 3>(n_bobs, [&](auto M) {
                LaunchTimer t(h, STORE ? "dalton_fwd_kernel<store>" : "dalton_fwd_kernel<loglik>");
                hipLaunchKernelGGL((dalton_fwd_kernel<RHS, P, I, M, STORE>), g.grid, g.block, 0, h->stream, a, o, logdens);
                t.stop();
                ok = true;
            });
        });
    });
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "dalton: no kernel for n_bstate %d, interrogate %d, n_bobs %d", c->n_bstate,
               c->interrogate, n_bobs);
    RK_HIP(hipGetLastError());
    return RK_OK;
}

// the forward filter(s) on the chosen route: out = logdens (B) for the log-likelihood, the tile records or nothing (the
// batch-minor moments go through a.mean / a.var) for the store form
template <bool STORE>
static int dalton_forward(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, int n_bobs, bool tile,
                          double* out) {
    int rc = RK_ERR_UNSUPPORTED;
    if (is_user_rhs(c->rhs_id)) return user_dalton(h, c, a, o, n_bobs, STORE, tile, out);
    with_builtin_rhs(c->rhs_id, [&](auto rhs) {
        using RHS = decltype(rhs);
        rc = check_n_theta<RHS>(c, a);
        if (rc) return;
        if (tile) {
            rc = launch_dalton_tile_rhs<RHS, STORE>(h, c, a, o, out);
        } else {
            rc = launch_dalton_rhs<RHS, STORE>(h, c, a, o, n_bobs, out);
        }
    });
    return rc;
}

static int dalton_inputs(const rk_solve_cfg* c, const rk_solve_in* in, const double* obs, const double* obs_weight,
                         const double* obs_var, const int32_t* obs_ind, int n_obs, int n_bobs, DaltonObs& o) {
    int rc = check_cfg(c, in);
    if (rc) return rc;
    rc = dalton_check(c, n_bobs);
    if (rc) return rc;
    RK_REQUIRE(n_obs >= 0 && (n_obs == 0 || (obs && obs_weight && obs_var && obs_ind)), RK_ERR_INVALID,
               "dalton: null observation array or n_obs < 0");
    o.obs = obs; o.obs_w = obs_weight; o.obs_v = obs_var; o.obs_ind = obs_ind; o.n_obs = n_obs;
    return RK_OK;
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_dalton_layout(const rk_solve_cfg* c, int32_t mode, int32_t n_bobs, int32_t* layout) {
    RK_REQUIRE(c && layout, RK_ERR_INVALID, "rk_dalton_layout: null argument");
    RK_REQUIRE(mode >= RK_MODE_FILTER && mode <= RK_MODE_SIM, RK_ERR_INVALID, "rk_dalton_layout: bad mode %d", mode);
    const int rc = dalton_check(c, n_bobs);
    if (rc) return rc;
    *layout = dalton_tile_route(c, n_bobs) ? RK_LAYOUT_TILE3 : RK_LAYOUT_BATCH_MINOR;
    return RK_OK;
}

int rk_dalton_loglik(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const double* obs, const double* obs_weight,
                     const double* obs_var, const int32_t* obs_ind, int32_t n_obs, int32_t n_bobs, double* logdens) {
    RK_REQUIRE(h && logdens, RK_ERR_INVALID, "rk_dalton_loglik: null argument");
    DaltonObs o;
    int rc = dalton_inputs(c, in, obs, obs_weight, obs_var, obs_ind, n_obs, n_bobs, o);
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, nullptr, a);
    const bool tile = dalton_tile_route(c, n_bobs);
    if (tile) RK_HIP(hipMemsetAsync(logdens, 0, sizeof(double) * (size_t)c->n_traj, h->stream));   // (two atomic adds each)
    return dalton_forward<false>(h, c, a, o, n_bobs, tile, logdens);
}

int rk_dalton_solve(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, int32_t mode,
                    const double* obs, const double* obs_weight, const double* obs_var, const int32_t* obs_ind,
                    int32_t n_obs, int32_t n_bobs) {
    RK_REQUIRE(h && out, RK_ERR_INVALID, "rk_dalton_solve: null argument");
    RK_REQUIRE(mode >= RK_MODE_FILTER && mode <= RK_MODE_SIM, RK_ERR_INVALID, "rk_dalton_solve: bad mode %d", mode);
    DaltonObs o;
    int rc = dalton_inputs(c, in, obs, obs_weight, obs_var, obs_ind, n_obs, n_bobs, o);
    if (rc) return rc;
    int32_t lay = 0, want = 0;
    rk_solve_cfg natural = *c;                     // (the DALTON kernels write natural rows whatever the caller asked of rk_solve_mv)
    natural.flags &= ~RK_FLAG_TILE3_PACKED_MV;
    rc = rk_solve_layout(&natural, mode, &lay);
    if (rc) return rc;
    rc = rk_dalton_layout(c, mode, n_bobs, &want);
    if (rc) return rc;
    RK_REQUIRE(lay == want, RK_ERR_UNSUPPORTED,
               "rk_dalton_solve writes layout %d but rk_solve_layout reports %d for this cfg (set RK_FLAG_BATCH_MINOR)", want, lay);
    const bool tile = want == RK_LAYOUT_TILE3;
    const bool sp = (c->flags & RK_FLAG_STORE_PRED) != 0;
    RK_REQUIRE((tile || out->mean_state) && out->var_state && (!sp || (out->mean_pred && out->var_pred)) &&
               (mode != RK_MODE_SIM || out->x_state), RK_ERR_INVALID,
               "rk_dalton_solve: out->mean_state / var_state (+ mean_pred / var_pred with RK_FLAG_STORE_PRED, x_state for "
               "RK_MODE_SIM) must not be NULL");
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, out, a);
    if (!sp) a.mean_pred = a.var_pred = nullptr;                          // (the kernel stores predictions iff mean_pred is set)
    rc = dalton_forward<true>(h, c, a, o, n_bobs, tile, tile ? out->var_state : nullptr);
    if (rc || mode == RK_MODE_FILTER) return rc;
    return tile ? tile3_backward(h, a, out->var_state, mode) : small_backward_pass(h, c, a, mode);
}

}  // extern "C"
