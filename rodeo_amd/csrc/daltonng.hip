// DALTON for non-Gaussian observations (src/rodeo/inference/dalton.py:547-1039): host side of rk_daltonng_workspace_bytes /
// rk_daltonng_loglik / rk_daltonng_solve.  The forward filter and the observation kernel are hiprtc builds around the user's
// log-likelihood (rhs_jit.hip: ng_forward, ng_obs_eval); the gain and chain kernels of the two backward log-density passes
// are built here, and rk_daltonng_solve ends in the solver's own smoothing pass.
#include "common.hpp"
#include "rhs.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "daltonng_kernels.hpp"

namespace rk {

// Is this configuration served?  RK_OK, or RK_ERR_UNSUPPORTED / RK_ERR_INVALID with the reason; `who` names the entry in the
// messages (also asked by rk_daltonng_grid_*, daltonng_grid.hip: declared in solve_paths.hpp).
int ng_check(const char* who, const rk_solve_cfg* c, int obs_id) {
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD, RK_ERR_UNSUPPORTED,
               "%s: kalman_type %d is not built (only the standard form)", who, c->kalman_type);
    RK_REQUIRE(c->interrogate >= RK_INTERROGATE_RODEO && c->interrogate <= RK_INTERROGATE_KRAMER, RK_ERR_UNSUPPORTED,
               "%s: interrogate id %d is not supported (rodeo, schober, kramer)", who, c->interrogate);
    RK_REQUIRE(c->n_bmeas == 1, RK_ERR_UNSUPPORTED, "%s: n_bmeas = 1 only, got %d", who, c->n_bmeas);
    RK_REQUIRE(c->n_bstate >= 2 && c->n_bstate <= 6, RK_ERR_UNSUPPORTED, "%s: n_bstate in 2..6, got %d", who, c->n_bstate);
    RK_REQUIRE(c->n_block < 3 || c->n_bstate <= 5, RK_ERR_UNSUPPORTED,
               "%s: n_bstate up to 5 with three or more blocks (the lane kernel spills), got %d", who, c->n_bstate);
    NgObsInfo ob;
    int rc = ng_obs_info(obs_id, &ob);
    if (rc) return rc;
    RK_REQUIRE(ob.n_block == c->n_block && ob.n_bstate == c->n_bstate, RK_ERR_INVALID,
               "%s: observation model %d was registered for (n_block, n_bstate) = (%d, %d), the solver has (%d, %d)", who, obs_id,
               ob.n_block, ob.n_bstate, c->n_block, c->n_bstate);
    if (is_user_rhs(c->rhs_id)) {
        rc = user_rhs_check(c);
        if (rc) return rc;
    } else {
        bool known = false, fits = false;
        with_builtin_rhs(c->rhs_id, [&](auto rhs) {
            known = true;
            fits = decltype(rhs)::D == c->n_block;
        });
        RK_REQUIRE(known, RK_ERR_UNSUPPORTED, "%s: unknown rhs_id %d", who, c->rhs_id);
        RK_REQUIRE(fits, RK_ERR_UNSUPPORTED, "%s: rhs %d needs another n_block than %d", who, c->rhs_id, c->n_block);
    }
    // (the traced struct packs the same parameters as the right-hand side; both keep one dummy slot when there are none)
    RK_REQUIRE(ob.n_theta == c->n_theta, RK_ERR_INVALID, "%s: observation model %d takes %d parameters, the solver %d", who,
               obs_id, ob.n_theta, c->n_theta);
    return RK_OK;
}

struct NgSizes { size_t mom, var, rec, sm, part; };
static NgSizes ng_sizes(const rk_solve_cfg* c, int n_obs) {
    const size_t B = (size_t)c->n_traj, N = (size_t)c->n_steps, D = (size_t)c->n_block, P = (size_t)c->n_bstate;
    NgSizes s;
    s.mom = (N + 1) * D * P * B;
    s.var = s.mom * P;
    s.rec = (N - 1) * D * (size_t)ng_rec_doubles((int)P) * B;
    s.sm = (size_t)(n_obs > 0 ? n_obs : 0) * D * P * B;
    s.part = 2 * D * B;
    return s;
}
static size_t ng_ws_doubles(const NgSizes& s) { return 2 * (s.mom + s.var) + s.rec + s.sm + s.part; }

// the workspace of rk_daltonng_workspace_bytes carved into its parts, after its size is checked (also the workspace of
// rk_daltonng_grid_loglik: declared in solve_paths.hpp)
int ng_workspace(const char* who, const rk_solve_cfg* c, int n_obs, void* workspace, size_t workspace_bytes, NgWs& w) {
    const NgSizes s = ng_sizes(c, n_obs);
    RK_REQUIRE(workspace && workspace_bytes >= sizeof(double) * ng_ws_doubles(s), RK_ERR_INVALID,
               "%s: workspace of %zu bytes, rk_daltonng_workspace_bytes asks for %zu", who, workspace_bytes,
               sizeof(double) * ng_ws_doubles(s));
    w.jm = (double*)workspace;
    w.jv = w.jm + s.mom;
    w.zm = w.jv + s.var;
    w.zv = w.zm + s.mom;
    w.rec = w.zv + s.var;
    w.sm = w.rec + s.rec;
    w.part = w.sm + s.sm;
    return RK_OK;
}

// the sequential half of the two backward log-density passes (also that of rk_daltonng_grid_loglik: declared in solve_paths.hpp)
int ng_chain(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const NgWs& w, const NgObs& o) {
    LaunchTimer t(h, "daltonng_chain_kernel");
    const bool ok = dispatch_int<2, 6>(c->n_bstate, [&](auto P) {
        hipLaunchKernelGGL((daltonng_chain_kernel<P>), dim3(div_up(a.B * a.D, 64)), dim3(64), 0, h->stream, a, w, o);
    });
    t.stop();
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "daltonng: no backward kernels for n_bstate %d", c->n_bstate);
    return RK_OK;
}

static int ng_inputs(const rk_solve_cfg* c, const rk_solve_in* in, int obs_id, const double* obs, const int32_t* obs_ind, int n_obs,
                     NgObs& o) {
    int rc = check_cfg(c, in);
    if (rc) return rc;
    rc = ng_check("daltonng", c, obs_id);
    if (rc) return rc;
    RK_REQUIRE(n_obs >= 0 && (n_obs == 0 || (obs && obs_ind)), RK_ERR_INVALID, "daltonng: null observation array or n_obs < 0");
    o.y = obs; o.obs_ind = obs_ind; o.n_obs = n_obs;
    return RK_OK;
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_daltonng_workspace_bytes(const rk_solve_cfg* c, int32_t n_obs, size_t* bytes) {
    RK_REQUIRE(c && bytes, RK_ERR_INVALID, "rk_daltonng_workspace_bytes: null argument");
    RK_REQUIRE(c->n_traj >= 1 && c->n_steps >= 1 && c->n_block >= 1 && c->n_bstate >= 2 && c->n_bstate <= 6 && n_obs >= 0,
               RK_ERR_INVALID, "rk_daltonng_workspace_bytes: bad dimensions");
    *bytes = sizeof(double) * ng_ws_doubles(ng_sizes(c, n_obs));
    return RK_OK;
}

int rk_daltonng_loglik(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, int32_t obs_id, const double* obs,
                       const int32_t* obs_ind, int32_t n_obs, void* workspace, size_t workspace_bytes, double* logdens) {
    RK_REQUIRE(h && logdens, RK_ERR_INVALID, "rk_daltonng_loglik: null argument");
    NgObs o;
    int rc = ng_inputs(c, in, obs_id, obs, obs_ind, n_obs, o);
    if (rc) return rc;
    NgWs w;
    rc = ng_workspace("rk_daltonng_loglik", c, n_obs, workspace, workspace_bytes, w);
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, nullptr, a);
    a.mean = w.jm; a.var = w.jv; a.mean_pred = a.var_pred = a.x = nullptr;
    rc = ng_forward(h, c, obs_id, a, o, true, w.zm, w.zv);
    if (rc) return rc;
    const size_t items = (size_t)(a.N - 1) * a.D * a.B;
    RK_REQUIRE(items / 64 < 0x7fffffffu, RK_ERR_UNSUPPORTED, "daltonng: too many (step, block, trajectory) items for one launch");
    if (items) {
        LaunchTimer t(h, "daltonng_gain_kernel");
        const bool ok = dispatch_int<2, 6>(c->n_bstate, [&](auto P) {
            hipLaunchKernelGGL((daltonng_gain_kernel<P>), dim3((unsigned)((items + 63) / 64)), dim3(64), 0, h->stream, a, w);
        });
        t.stop();
        RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "daltonng: no backward kernels for n_bstate %d", c->n_bstate);
    }
    rc = ng_chain(h, c, a, w, o);
    if (rc) return rc;
    RK_HIP(hipGetLastError());
    return ng_obs_eval(h, c, obs_id, a, o, w.sm, w.part, logdens);
}

int rk_daltonng_solve(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, int32_t mode,
                      int32_t obs_id, const double* obs, const int32_t* obs_ind, int32_t n_obs) {
    RK_REQUIRE(h && out, RK_ERR_INVALID, "rk_daltonng_solve: null argument");
    RK_REQUIRE(mode == RK_MODE_FILTER || mode == RK_MODE_MV, RK_ERR_UNSUPPORTED,
               "rk_daltonng_solve: mode %d is not built (the filter and solve_mv_nn; the reference has no sampler here)", mode);
    NgObs o;
    int rc = ng_inputs(c, in, obs_id, obs, obs_ind, n_obs, o);
    if (rc) return rc;
    int32_t lay = 0;
    rc = rk_solve_layout(c, mode, &lay);
    if (rc) return rc;
    RK_REQUIRE(lay == RK_LAYOUT_BATCH_MINOR, RK_ERR_UNSUPPORTED,
               "rk_daltonng_solve writes the batch-minor layout but rk_solve_layout reports %d for this cfg (set RK_FLAG_BATCH_MINOR)",
               lay);
    RK_REQUIRE(out->mean_state && out->var_state, RK_ERR_INVALID, "rk_daltonng_solve: out->mean_state / var_state must not be NULL");
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, out, a);
    a.mean_pred = a.var_pred = nullptr;
    rc = ng_forward(h, c, obs_id, a, o, false, nullptr, nullptr);
    if (rc || mode == RK_MODE_FILTER) return rc;
    return small_backward_pass(h, c, a, mode);
}

}  // extern "C"
