// solve_mv_grid / solve_sim_grid (an addition): host side of rk_solve_grid, the solver on a
// non-uniform grid shared by the batch -- every step has its own length, hence its own prior pair (Q, R), named by a slot
// (grid_kernels.hpp) -- and the two backward kernels.  One route: the lanes on batch-minor records -- grid_fwd_kernel, one
// lane per trajectory, then grid_bwd_mv_kernel or grid_bwd_sim_kernel, one lane per (trajectory, block): the passes of
// bwd_mv_kernel / bwd_sim_kernel (lane_backward.hpp: bwd_smooth_lane / bwd_sample_lane over bwd_walk) under the prediction
// policy SlotPrior, Q_n Sigma_f[n] Q_n^T + R_n with the gain from Q_n.  Standard form, n_bmeas = 1.  No workspace.
// Also here: the bodies of what every entry on the grid shares (grid_entry.hpp) -- the pieces of the configuration check, the
// staging of rk_grid_in and the test of the output pointers.
#include <cmath>
#include <cstdio>
#include "common.hpp"
#include "rhs.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "grid_entry.hpp"
#include "grid_kernels.hpp"
#include "lane_backward.hpp"

namespace rk {

// ---- backward passes: one lane per (block, trajectory) -----------------------------------------------------------
// bwd_walk's prediction policy with the prior pair of step n -> n + 1, which is fetched next to filt[n] (so one step ahead of
// its use, like the record) and is the transition matrix of that step's smoothing gain.  The lane's own Q, R are not read.
template <int P>
struct SlotPrior {
    GridArgs g;
    struct Datum { double Q[P][P], R[P][P]; };
    __device__ __forceinline__ Datum fetch(const SolveArgs& a, const BwdLane<P>& ln, int n) const {
        Datum c;
        grid_load_pair<P>(g, a.B, a.D, grid_slot(g, n), ln.blk, ln.b, c.Q, c.R);
        return c;
    }
    __device__ __forceinline__ void predict(const BwdLane<P>&, const Datum& c, const double (&mf)[P], const double (&Sf)[P][P],
                                            double (&mp)[P], double (&Sp)[P][P]) const {
        predict_block<P>(c.Q, c.R, mf, Sf, mp, Sp);       // pred[n+1] from filt[n] and the pair of step n
    }
    __device__ __forceinline__ const auto& trans(const BwdLane<P>&, const Datum& c) const { return c.Q; }
};

template <int P>
__global__ void __launch_bounds__(64) grid_bwd_mv_kernel(SolveArgs a, GridArgs g) {
    BwdLane<P> ln;
    if (ln.init(a)) bwd_smooth_lane<P>(a, ln, SlotPrior<P>{g});
}

template <int P>
__global__ void __launch_bounds__(64) grid_bwd_sim_kernel(SolveArgs a, GridArgs g) {
    BwdLane<P> ln;
    if (ln.init(a)) bwd_sample_lane<P>(a, ln, SlotPrior<P>{g});
}

// ---- dispatch ---------------------------------------------------------------------------------------------------
// n_bstate of the forward instances: an instance ships only if it needs no more scratch than fwd_kernel at the same
// (RHS, P, ITG) -- DESIGN.md section 7 (15) has the figures of every instance and of the ones that are left out
constexpr int GRID_PMIN = 2, GRID_PMAX = 6;
constexpr int GRID_PMAX_THREE_BLOCKS = 5;
template <class RHS>
constexpr int grid_pmax() { return RHS::D >= 3 ? GRID_PMAX_THREE_BLOCKS : GRID_PMAX; }

// ---- what the grid entries share (grid_entry.hpp; the sizes piece is written out there) ------------------------------
int grid_flags_check(const char* who, const char* records, const rk_solve_cfg* c) {
    RK_REQUIRE((c->flags & RK_FLAG_BATCH_MINOR) != 0, RK_ERR_INVALID, "%s: cfg->flags must carry RK_FLAG_BATCH_MINOR (%s)", who,
               records);
    RK_REQUIRE((c->flags & RK_FLAG_STORE_PRED) == 0, RK_ERR_UNSUPPORTED, "%s: RK_FLAG_STORE_PRED is not served", who);
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD || c->kalman_type == RK_KALMAN_SQRT, RK_ERR_UNSUPPORTED,
               "%s: unknown kalman_type %d", who, c->kalman_type);
    return RK_OK;
}

int grid_served_check(const GridServed& s, const rk_solve_cfg* c) {
    const int rc = grid_flags_check(s.who, s.records, c);
    if (rc) return rc;
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD, RK_ERR_UNSUPPORTED, "%s: kalman_type square-root is not built", s.who);
    RK_REQUIRE(!s.no_chkrebtii || c->interrogate != RK_INTERROGATE_CHKREBTII, RK_ERR_UNSUPPORTED,
               "%s: interrogate_chkrebtii is not served (%s)", s.who, s.no_chkrebtii);
    RK_REQUIRE(c->interrogate >= RK_INTERROGATE_RODEO && c->interrogate <= s.itg_last, RK_ERR_UNSUPPORTED,
               "%s: interrogate id %d is not supported (rodeo, schober, kramer%s)", s.who, c->interrogate,
               s.itg_last == RK_INTERROGATE_CHKREBTII ? ", chkrebtii" : "");
    RK_REQUIRE(c->n_bmeas == 1, RK_ERR_UNSUPPORTED, "%s: n_bmeas = 1 only (the dense / indep_init form is not served), got %d",
               s.who, c->n_bmeas);
    RK_REQUIRE(c->n_bstate >= s.pmin && c->n_bstate <= s.pmax, RK_ERR_UNSUPPORTED, "%s: n_bstate in %d..%d, got %d", s.who, s.pmin,
               s.pmax, c->n_bstate);
    RK_REQUIRE(c->n_block < 3 || c->n_bstate <= s.pmax3, RK_ERR_UNSUPPORTED,
               "%s: n_bstate up to %d with three or more blocks, got %d", s.who, s.pmax3, c->n_bstate);
    return RK_OK;
}

int grid_rhs_check(const char* who, const rk_solve_cfg* c, const char* rule) {
    if (is_user_rhs(c->rhs_id)) {
        const int rc = user_lane_check(c, rule ? rule : who);
        if (rc && rule) {
            const std::string why = rk_last_error();
            set_error("%s: %s", who, why.c_str());
        }
        return rc;
    }
    RK_REQUIRE(with_builtin_rhs(c->rhs_id, [](auto) {}), RK_ERR_UNSUPPORTED, "%s: unknown rhs_id %d", who, c->rhs_id);
    RK_REQUIRE(builtin_has_n_block(c->rhs_id, c->n_block), RK_ERR_UNSUPPORTED, "%s: rhs %d needs another n_block than %d", who,
               c->rhs_id, c->n_block);
    return RK_OK;
}

int grad_check(const char* who, const rk_solve_cfg* c, int n_bobs, int n_dir, bool per_block, int (*user_check)(const rk_solve_cfg*),
               int pmax, const char* why_not) {
    const int rc = grid_sizes_check(who, c);                             // (from here on the wording is the gradient entries' own)
    if (rc) return rc;
    RK_REQUIRE(n_dir >= 1, RK_ERR_INVALID, "%s: n_dir must be at least 1, got %d", who, n_dir);
    const long long items = (long long)c->n_traj * n_dir * (per_block ? c->n_block : 1);
    RK_REQUIRE(items <= 0x7fffffffLL, RK_ERR_INVALID, "%s: n_traj * n_dir%s = %lld exceeds 2^31 - 1", who, per_block ? " * n_block" : "",
               items);
    RK_REQUIRE((c->flags & RK_FLAG_BATCH_MINOR) != 0, RK_ERR_INVALID, "%s: cfg->flags must carry RK_FLAG_BATCH_MINOR", who);
    RK_REQUIRE((c->flags & RK_FLAG_STORE_PRED) == 0, RK_ERR_UNSUPPORTED, "%s: RK_FLAG_STORE_PRED is not served", who);
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD, RK_ERR_UNSUPPORTED, "%s: not built: kalman_type %d (standard only)", who,
               c->kalman_type);
    RK_REQUIRE(c->interrogate >= RK_INTERROGATE_RODEO && c->interrogate <= RK_INTERROGATE_KRAMER, RK_ERR_UNSUPPORTED,
               "%s: not built: interrogate id %d (rodeo, schober, kramer)", who, c->interrogate);
    RK_REQUIRE(c->n_bmeas == 1, RK_ERR_UNSUPPORTED, "%s: not built: n_bmeas = %d (1 only)", who, c->n_bmeas);
    RK_REQUIRE(n_bobs == 1, RK_ERR_UNSUPPORTED, "%s: not built: n_bobs = %d (1 only: the derivative of the "
               "eigendecomposition's cut-off density is out of scope)", who, n_bobs);
    if (is_user_rhs(c->rhs_id)) return user_check(c);
    bool known = false;
    with_builtin_rhs(c->rhs_id, [&](auto rhs) { known = grad_has_rhs<decltype(rhs)>(); });
    RK_REQUIRE(known, RK_ERR_UNSUPPORTED, "%s: not built: rhs %d (fitzhugh_nagumo and lorenz63)", who, c->rhs_id);
    RK_REQUIRE(builtin_has_n_block(c->rhs_id, c->n_block), RK_ERR_UNSUPPORTED, "%s: rhs %d needs another n_block than %d", who,
               c->rhs_id, c->n_block);
    char range[32];
    snprintf(range, sizeof range, "%d .. %d", GRAD_PMIN, pmax);
    RK_REQUIRE(c->n_bstate >= GRAD_PMIN && c->n_bstate <= pmax, RK_ERR_UNSUPPORTED, "%s: not built: rhs %d at n_bstate %d (%s)", who,
               c->rhs_id, c->n_bstate, why_not ? why_not : range);
    return RK_OK;
}

int grid_args(const char* who, const rk_grid_in* g, GridArgs& ga) {
    RK_REQUIRE(g->t && g->slot && g->q && g->r && g->n_slots >= 1, RK_ERR_INVALID,
               "%s: grid needs t, slot, q, r and n_slots >= 1 (got %d)", who, g->n_slots);
    ga = GridArgs{g->t, g->slot, g->q, g->r, g->q_batched != 0, g->r_batched != 0, g->n_slots};
    return RK_OK;
}

int grid_out_check(const char* who, const rk_solve_out* out, int mode) {
    RK_REQUIRE(out->mean_state && out->var_state, RK_ERR_INVALID, "%s: out->mean_state / var_state must not be NULL", who);
    RK_REQUIRE(mode != RK_MODE_SIM || out->x_state, RK_ERR_INVALID, "%s: RK_MODE_SIM needs out->x_state", who);
    return RK_OK;
}

// ---- rk_solve_grid ----------------------------------------------------------------------------------------------
// Is this call served?  Decided on the configuration and the mode alone: RK_OK, RK_ERR_INVALID or RK_ERR_UNSUPPORTED.
static int grid_check(const rk_solve_cfg* c, int mode) {
    int rc = grid_sizes_check("grid", c);
    if (rc) return rc;
    RK_REQUIRE(mode == RK_MODE_MV || mode == RK_MODE_SIM, RK_ERR_INVALID, "grid: mode must be RK_MODE_MV or RK_MODE_SIM, got %d",
               mode);
    rc = grid_served_check({"grid", GRID_RECORDS, RK_INTERROGATE_CHKREBTII, nullptr, GRID_PMIN, GRID_PMAX, GRID_PMAX_THREE_BLOCKS}, c);
    if (rc) return rc;
    return grid_rhs_check("grid", c);
}

// the forward pass for a built-in or a user right-hand side (also that of rk_fenrir_grid_*, fenrir_grid.hip, and of
// rk_solve_sim_draws_grid, grid_draws.hip: declared in solve_paths.hpp)
int launch_grid_forward(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& ga) {
    return launch_by_rhs(c, a, [&] { return user_grid(h, c, a, ga); }, [&](auto rhs) {
        using RHS = decltype(rhs);
        const LaunchGeom g = fwd_lane_geom(a.B);
        return launch_fwd_instance<GRID_PMIN, grid_pmax<RHS>(), RK_INTERROGATE_RODEO, RK_INTERROGATE_CHKREBTII>(
            h, c, "grid_fwd_kernel", "grid", [&](auto P, auto I) {
                hipLaunchKernelGGL((grid_fwd_kernel<RHS, P, I>), g.grid, g.block, 0, h->stream, a, ga);
            });
    });
}

// (also the backward pass of rk_dalton_grid_solve, dalton_grid.hip, and of rk_daltonng_grid_solve, daltonng_grid.hip: declared in
// solve_paths.hpp)
int launch_grid_bwd(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, int mode, const GridArgs& ga) {
    const LaunchGeom g = bwd_lane_geom(a.B, a.D);
    return launch_bwd_instance<GRID_PMIN, GRID_PMAX>(h, c, mode, "grid_bwd_mv_kernel", "grid_bwd_sim_kernel", "grid",
                                                     [&](auto P, bool sim) {
        if (sim) hipLaunchKernelGGL((grid_bwd_sim_kernel<P>), g.grid, g.block, 0, h->stream, a, ga);
        else hipLaunchKernelGGL((grid_bwd_mv_kernel<P>), g.grid, g.block, 0, h->stream, a, ga);
    });
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_solve_grid(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, int32_t mode,
                  const rk_grid_in* g) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_solve_grid: null cfg");
    int rc = grid_check(c, mode);                                   // (the configuration alone, before anything else is looked at)
    if (rc) return rc;
    RK_REQUIRE(h && out && g, RK_ERR_INVALID, "rk_solve_grid: null argument");
    GridArgs ga;
    rc = grid_args("rk_solve_grid", g, ga);
    if (rc) return rc;
    rc = check_cfg(c, in);
    if (rc) return rc;
    rc = grid_out_check("rk_solve_grid", out, mode);
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, out, a);
    rc = launch_grid_forward(h, c, a, ga);
    if (rc) return rc;
    return launch_grid_bwd(h, c, a, mode, ga);
}

}  // extern "C"
