// dalton_grid / dalton.solve_mv_grid / dalton.solve_sim_grid (an addition): host side of
// rk_dalton_grid_loglik / rk_dalton_grid_solve, DALTON for Gaussian observations on a non-uniform grid shared by the batch, every
// observation on a node.  One route: the lanes on batch-minor records -- dalton_grid_fwd_kernel (dalton_grid_kernels.hpp), two
// filters per trajectory in the halves of a wave for the log-likelihood, one lane per trajectory for the store form, then
// grid.hip's own backward launch (grid_bwd_mv_kernel / grid_bwd_sim_kernel).  Standard form, n_bmeas = 1.  No workspace.
// The pieces of the configuration check, the grid's staging and the right-hand-side switch are grid_entry.hpp's; the forward
// launch stays written out here: it dispatches on n_bobs as well and decides per instance whether there is a kernel at all.
#include "common.hpp"
#include "rhs.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "grid_entry.hpp"
#include "dalton_grid_kernels.hpp"

namespace rk {

// The rule an instance ships by: no more scratch than the larger of dalton_fwd_kernel<RHS, P, ITG, MO,
// STORE> and grid_fwd_kernel<RHS, P, ITG>.  profiles/dalton_grid_code_objects.txt has every instance next to the two; left out:
// the log-likelihood form of (FitzHugh-Nagumo, 4, any interrogation, n_bobs = 3) -- two register sets of the pair (D P^2 = 32)
// next to two filters' 3 x 3 eigendecomposition: 512 registers + 120 .. 188 B where both siblings have none.  Its store form ships.
// -DRK_DALTON_GRID_ALL_INSTANCES builds them all, for that listing (`make variant`).
template <class RHS, int P, int MO, bool STORE>
constexpr bool dalton_grid_ships() {
#ifdef RK_DALTON_GRID_ALL_INSTANCES
    return true;
#else
    return !(std::is_same<RHS, FitzHughNagumo>::value && P == 4 && MO == 3 && !STORE);
#endif
}
// n_bstate served: dalton's lane range (dalton_pmax<RHS>() of solve_paths.hpp is the built-in instances' upper end)
constexpr int DALTON_GRID_PMIN = 2, DALTON_GRID_PMAX = 6, DALTON_GRID_PMAX_THREE_BLOCKS = 5;
static_assert(dalton_pmax<FitzHughNagumo>() == DALTON_GRID_PMAX && dalton_pmax<Lorenz63>() == DALTON_GRID_PMAX_THREE_BLOCKS,
              "the check's limits are the instances'");

// (also asked by rk_dalton_grid_sim_draws, grid_draws.hip: declared in solve_paths.hpp)
bool dalton_grid_left_out(const rk_solve_cfg* c, int n_bobs, bool store) {
    bool out = false;
    with_builtin_rhs(c->rhs_id, [&](auto rhs) {
        dispatch_int<DALTON_GRID_PMIN, DALTON_GRID_PMAX>(c->n_bstate, [&](auto P) {
            dispatch_int<1, 3>(n_bobs, [&](auto M) {
                out = store ? !dalton_grid_ships<decltype(rhs), P, M, true>() : !dalton_grid_ships<decltype(rhs), P, M, false>();
            });
        });
    });
    return out;
}

// Is this call served?  Decided on the configuration, the mode and n_bobs alone: RK_OK, RK_ERR_INVALID or RK_ERR_UNSUPPORTED.
// grid_check's pattern (grid.hip; the pieces are grid_entry.hpp's) joined with dalton_check's limits (dalton.hip).  mode < 0: the
// log-likelihood, which has none.
static int dalton_grid_check(const rk_solve_cfg* c, int mode, int n_bobs) {
    int rc = grid_sizes_check("dalton_grid", c);
    if (rc) return rc;
    RK_REQUIRE(mode < 0 || mode == RK_MODE_MV || mode == RK_MODE_SIM, RK_ERR_INVALID,
               "dalton_grid: mode must be RK_MODE_MV or RK_MODE_SIM, got %d", mode);
    rc = grid_served_check({"dalton_grid", GRID_RECORDS, RK_INTERROGATE_KRAMER, nullptr, DALTON_GRID_PMIN, DALTON_GRID_PMAX,
                            DALTON_GRID_PMAX_THREE_BLOCKS}, c);
    if (rc) return rc;
    RK_REQUIRE(n_bobs >= 1 && n_bobs <= 3, RK_ERR_UNSUPPORTED, "dalton_grid: n_bobs in 1..3, got %d", n_bobs);
    rc = grid_rhs_check("dalton_grid", c);
    if (rc) return rc;
    // (never so for a user right-hand side: it has no instance to leave out)
    RK_REQUIRE(!dalton_grid_left_out(c, n_bobs, mode >= 0), RK_ERR_UNSUPPORTED,
               "dalton_grid: the %s form of rhs %d at n_bstate %d with n_bobs %d is left out (it needs more scratch than dalton's "
               "and the grid solver's kernels at the same parameters)", mode >= 0 ? "store" : "log-likelihood", c->rhs_id,
               c->n_bstate, n_bobs);
    return RK_OK;
}

// one launch of dalton_grid_fwd_kernel<RHS, P, ITG, n_bobs, STORE> for a built-in right-hand side
template <class RHS, bool STORE>
static int launch_dalton_grid_rhs(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, const GridArgs& ga,
                                  int n_bobs, double* logdens) {
    const LaunchGeom g = dalton_lane_geom(a.B, !STORE);
    bool ok = false;
    dispatch_int<DALTON_GRID_PMIN, dalton_pmax<RHS>()>(c->n_bstate, [&](auto P) {
        dispatch_int<RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(c->interrogate, [&](auto I) {
            dispatch_int<1, 3>(n_bobs, [&](auto M) {
                if constexpr (dalton_grid_ships<RHS, P, M, STORE>()) {
                    LaunchTimer t(h, STORE ? "dalton_grid_fwd_kernel<store>" : "dalton_grid_fwd_kernel<loglik>");
                    hipLaunchKernelGGL((dalton_grid_fwd_kernel<RHS, P, I, M, STORE>), g.grid, g.block, 0, h->stream, a, o, ga, logdens);
                    t.stop();
                    ok = true;
                }
            });
        });
    });
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "dalton_grid: no kernel for rhs %d, n_bstate %d, interrogate %d, n_bobs %d", c->rhs_id,
               c->n_bstate, c->interrogate, n_bobs);
    RK_HIP(hipGetLastError());
    return RK_OK;
}

template <bool STORE>
static int dalton_grid_forward(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, const GridArgs& ga,
                               int n_bobs, double* logdens) {
    return launch_by_rhs(c, a, [&] { return user_dalton_grid(h, c, a, o, ga, n_bobs, STORE, logdens); }, [&](auto rhs) {
        return launch_dalton_grid_rhs<decltype(rhs), STORE>(h, c, a, o, ga, n_bobs, logdens);
    });
}

// the store form's forward pass (also that of rk_dalton_grid_sim_draws, grid_draws.hip: declared in solve_paths.hpp)
int dalton_grid_store_forward(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, const GridArgs& ga,
                              int n_bobs) {
    return dalton_grid_forward<true>(h, c, a, o, ga, n_bobs, nullptr);
}

// the pointers of a served call: the grid (rk_solve_grid's rule), the solver inputs and the observations (dalton_inputs' rule)
// (also those of rk_dalton_grid_sim_draws, grid_draws.hip: declared in solve_paths.hpp)
int dalton_grid_inputs(const char* who, const rk_solve_cfg* c, const rk_solve_in* in, const double* obs,
                       const double* obs_weight, const double* obs_var, const int32_t* obs_ind, int n_obs, const rk_grid_in* g,
                       DaltonObs& o, GridArgs& ga) {
    int rc = grid_args(who, g, ga);
    if (rc) return rc;
    rc = check_cfg(c, in);
    if (rc) return rc;
    RK_REQUIRE(n_obs >= 0 && (n_obs == 0 || (obs && obs_weight && obs_var && obs_ind)), RK_ERR_INVALID,
               "%s: null observation array or n_obs < 0", who);
    o.obs = obs; o.obs_w = obs_weight; o.obs_v = obs_var; o.obs_ind = obs_ind; o.n_obs = n_obs;
    return RK_OK;
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_dalton_grid_loglik(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const double* obs, const double* obs_weight,
                          const double* obs_var, const int32_t* obs_ind, int32_t n_obs, int32_t n_bobs, const rk_grid_in* g,
                          double* logdens) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_dalton_grid_loglik: null cfg");
    int rc = dalton_grid_check(c, -1, n_bobs);                      // (the configuration alone, before anything else is looked at)
    if (rc) return rc;
    RK_REQUIRE(h && g && logdens, RK_ERR_INVALID, "rk_dalton_grid_loglik: null argument");
    DaltonObs o;
    GridArgs ga;
    rc = dalton_grid_inputs("rk_dalton_grid_loglik", c, in, obs, obs_weight, obs_var, obs_ind, n_obs, g, o, ga);
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, nullptr, a);
    return dalton_grid_forward<false>(h, c, a, o, ga, n_bobs, logdens);     // (one writer per logdens[b]: nothing to clear)
}

int rk_dalton_grid_solve(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, int32_t mode,
                         const double* obs, const double* obs_weight, const double* obs_var, const int32_t* obs_ind,
                         int32_t n_obs, int32_t n_bobs, const rk_grid_in* g) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_dalton_grid_solve: null cfg");
    RK_REQUIRE(mode >= 0, RK_ERR_INVALID, "dalton_grid: mode must be RK_MODE_MV or RK_MODE_SIM, got %d", mode);
    int rc = dalton_grid_check(c, mode, n_bobs);
    if (rc) return rc;
    RK_REQUIRE(h && out && g, RK_ERR_INVALID, "rk_dalton_grid_solve: null argument");
    DaltonObs o;
    GridArgs ga;
    rc = dalton_grid_inputs("rk_dalton_grid_solve", c, in, obs, obs_weight, obs_var, obs_ind, n_obs, g, o, ga);
    if (rc) return rc;
    rc = grid_out_check("rk_dalton_grid_solve", out, mode);
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, out, a);
    rc = dalton_grid_store_forward(h, c, a, o, ga, n_bobs);
    if (rc) return rc;
    return launch_grid_bwd(h, c, a, mode, ga);
}

}  // extern "C"
