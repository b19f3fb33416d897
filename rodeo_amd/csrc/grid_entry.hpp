// What the host sides of the non-uniform-grid entries share (host code only, not part of the hiprtc set; DESIGN.md section 7
// (22)): the configuration check in pieces, the staging of rk_grid_in and the test of the output pointers -- the longer bodies
// are in grid.hip -- and the three launch patterns as templates.  Included by grid.hip, grid_calib.hip, grid_draws.hip,
// dalton_grid.hip, daltonng_grid.hip, fenrir_grid.hip, dalton_grad.hip and fenrir_grad.hip, and by dynamic.hip for the launch patterns.
#pragma once
#include "common.hpp"
#include "solve_paths.hpp"

namespace rk {

// ---- the configuration check ---------------------------------------------------------------------------------------------
// An entry's check calls the pieces in this order with its own tests (mode, n_bobs, ...) between them, where they have always
// been: which of two refusals a doubly wrong configuration gets is part of the interface (tests/golden/grid_entry_refusals.npz).
// `who` is the name that opens every message.

// the limits of one entry, for grid_served_check
struct GridServed {
    const char* who;
    const char* records;        // the parenthesis of the RK_FLAG_BATCH_MINOR message: which records are the batch-minor ones
    int itg_last;               // last interrogation served: RK_INTERROGATE_KRAMER or RK_INTERROGATE_CHKREBTII
    const char* no_chkrebtii;   // the reason interrogate_chkrebtii gets a message of its own, or nullptr: the range's message
    int pmin, pmax, pmax3;      // n_bstate served, and up to where with three or more blocks
};
constexpr const char* GRID_RECORDS = "the records are the batch-minor ones";

// no non-positive dimension: RK_ERR_INVALID
inline int grid_sizes_check(const char* who, const rk_solve_cfg* c) {
    RK_REQUIRE(c->n_traj >= 1 && c->n_steps >= 1 && c->n_block >= 1 && c->n_bstate >= 1 && c->n_bmeas >= 1, RK_ERR_INVALID,
               "%s: non-positive dimension (n_traj=%d n_steps=%d n_block=%d n_bstate=%d n_bmeas=%d)", who, c->n_traj,
               c->n_steps, c->n_block, c->n_bstate, c->n_bmeas);
    return RK_OK;
}
// RK_FLAG_BATCH_MINOR (RK_ERR_INVALID), no RK_FLAG_STORE_PRED, a known kalman_type (RK_ERR_UNSUPPORTED)
int grid_flags_check(const char* who, const char* records, const rk_solve_cfg* c);
// grid_flags_check, then the standard form, the interrogation, n_bmeas = 1 and the n_bstate range: RK_ERR_UNSUPPORTED
int grid_served_check(const GridServed& s, const rk_solve_cfg* c);
// the right-hand side: a user one against its registration (user_lane_check), a built-in one by its id and n_block.  With
// `rule` the user check is another entry's (the forward pass is that entry's): its message under its name, prefixed with ours.
int grid_rhs_check(const char* who, const rk_solve_cfg* c, const char* rule = nullptr);

// The whole check of a gradient entry (dalton_grad.hip, fenrir_grad.hip), decided on the configuration, n_bobs and n_dir alone:
// RK_OK, RK_ERR_INVALID or RK_ERR_UNSUPPORTED, worded "not built: ..." (tests/golden/grad_entry_refusals.npz).  What differs
// between the two: the item limit -- n_traj * n_dir lanes, or with `per_block` that times n_block --, the check of a user
// right-hand side, the last n_bstate served (from GRAD_PMIN on) and the parenthesis of the last refusal (null: the range).
constexpr int GRAD_PMIN = 2;
template <class RHS>
constexpr bool grad_has_rhs() { return std::is_same<RHS, FitzHughNagumo>::value || std::is_same<RHS, Lorenz63>::value; }
int grad_check(const char* who, const rk_solve_cfg* c, int n_bobs, int n_dir, bool per_block, int (*user_check)(const rk_solve_cfg*),
               int pmax, const char* why_not = nullptr);

// ---- the pointers of a served call -----------------------------------------------------------------------------------------
// rk_grid_in's arrays and n_slots >= 1, and the kernels' view of it
int grid_args(const char* who, const rk_grid_in* g, GridArgs& ga);
// out->mean_state / var_state, and x_state for RK_MODE_SIM (an entry without a sampler passes RK_MODE_MV)
int grid_out_check(const char* who, const rk_solve_out* out, int mode);

// ---- launches ---------------------------------------------------------------------------------------------------------------
// user() for a user right-hand side (the hiprtc build's launch, rhs_jit.hip); else builtin(RHS{}) once the parameter count fits
template <class User, class Builtin>
int launch_by_rhs(const rk_solve_cfg* c, const SolveArgs& a, User&& user, Builtin&& builtin) {
    if (is_user_rhs(c->rhs_id)) return user();
    int rc = RK_ERR_UNSUPPORTED;
    with_builtin_rhs(c->rhs_id, [&](auto rhs) {
        rc = check_n_theta<decltype(rhs)>(c, a);
        if (!rc) rc = builtin(rhs);
    });
    return rc;
}

// one forward launch: launch(P, I) for n_bstate in [PLo, PHi] and interrogate in [ILo, IHi] (the instances built are exactly
// these), timed under `kernel`
template <int PLo, int PHi, int ILo, int IHi, class Launch>
int launch_fwd_instance(rk_handle h, const rk_solve_cfg* c, const char* kernel, const char* who, Launch&& launch) {
    bool ok = false;
    dispatch_int<PLo, PHi>(c->n_bstate, [&](auto P) {
        dispatch_int<ILo, IHi>(c->interrogate, [&](auto I) {
            LaunchTimer t(h, kernel);
            launch(P, I);
            t.stop();
            ok = true;
        });
    });
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "%s: no kernel for rhs %d, n_bstate %d, interrogate %d", who, c->rhs_id, c->n_bstate,
               c->interrogate);
    RK_HIP(hipGetLastError());
    return RK_OK;
}

// one backward launch, the smoother or the sampler: launch(P, sim) for n_bstate in [PLo, PHi], timed under kernel_mv / kernel_sim
template <int PLo, int PHi, class Launch>
int launch_bwd_instance(rk_handle h, const rk_solve_cfg* c, int mode, const char* kernel_mv, const char* kernel_sim, const char* who,
                        Launch&& launch) {
    const bool sim = mode == RK_MODE_SIM;
    LaunchTimer t(h, sim ? kernel_sim : kernel_mv);
    const bool ok = dispatch_int<PLo, PHi>(c->n_bstate, [&](auto P) { launch(P, sim); });
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "%s: no backward kernel for n_bstate %d", who, c->n_bstate);
    t.stop();
    RK_HIP(hipGetLastError());
    return RK_OK;
}

}  // namespace rk
