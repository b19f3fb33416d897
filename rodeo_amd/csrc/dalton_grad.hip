// dalton_grid_jvp / dalton_grid_grad / dalton_grad (an addition): host side of rk_dalton_grid_jvp,
// directional derivatives of rk_dalton_grid_loglik's value with respect to the ODE parameters and the initial state.  One
// route: dalton_grid_jvp_kernel (dalton_grad_kernels.hpp), one (trajectory, direction) item per lane pair, 32 items per wave.
// Standard form, n_bmeas = 1, n_bobs = 1, built-in FitzHugh-Nagumo and Lorenz63, or a user right-hand side of the gradient kind
// (hiprtc, rhs_jit.hip's JIT_DALTON_GRAD).  rk_dalton_grid_jvp_hyper (section 7 (25)) is the same entry with the log sigma / log
// observation variance directions, on dalton_grid_jvp_hyper_kernel (JIT_DALTON_GRAD_HYPER).  No workspace.  The sizes test, the grid's staging (through dalton_grid_inputs) and
// the launch patterns are grid_entry.hpp's; the rest of the configuration check is worded for this entry alone ("not built: ...").
#include "common.hpp"
#include "rhs.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "grid_entry.hpp"
#include "dalton_grad_kernels.hpp"

namespace rk {

// The rule an instance ships by: no more scratch than dalton_grid_fwd_kernel<RHS, P, ITG, 1, false>.
// profiles/dalton_grad_code_objects.txt has every instance next to its sibling.  The lane's state is four moment sets per block
// next to the walk's pairs; what passes is n_bstate 2 and 3 of FitzHugh-Nagumo and Lorenz63 (D P^2 <= 27).  FitzHugh-Nagumo at 4
// (D P^2 = 32: 512 registers + 204 .. 388 B where the value kernel has none) and beyond, and Lorenz63 from 4 on, are left out.
// -DRK_DALTON_GRAD_ALL_INSTANCES builds FitzHugh-Nagumo at 4 and 5 and Lorenz63 at 4 as well, for that listing (`make variant`).
template <class RHS>
constexpr int dalton_grad_pmax() {
#ifdef RK_DALTON_GRAD_ALL_INSTANCES
    return std::is_same<RHS, FitzHughNagumo>::value ? 5 : 4;
#else
    return 3;
#endif
}
template <class RHS>
constexpr bool dalton_grad_has_rhs() { return std::is_same<RHS, FitzHughNagumo>::value || std::is_same<RHS, Lorenz63>::value; }

// Is this call served?  Decided on the configuration, n_bobs and n_dir alone: RK_OK, RK_ERR_INVALID or RK_ERR_UNSUPPORTED.
static int dalton_grad_check(const rk_solve_cfg* c, int n_bobs, int n_dir) {
    const int rc = grid_sizes_check("dalton_grid_jvp", c);               // (grid_entry.hpp; from here on the wording is this entry's own)
    if (rc) return rc;
    RK_REQUIRE(n_dir >= 1, RK_ERR_INVALID, "dalton_grid_jvp: n_dir must be at least 1, got %d", n_dir);
    RK_REQUIRE((long long)c->n_traj * n_dir <= 0x7fffffffLL, RK_ERR_INVALID, "dalton_grid_jvp: n_traj * n_dir = %lld exceeds 2^31 - 1",
               (long long)c->n_traj * n_dir);
    RK_REQUIRE((c->flags & RK_FLAG_BATCH_MINOR) != 0, RK_ERR_INVALID, "dalton_grid_jvp: cfg->flags must carry RK_FLAG_BATCH_MINOR");
    RK_REQUIRE((c->flags & RK_FLAG_STORE_PRED) == 0, RK_ERR_UNSUPPORTED, "dalton_grid_jvp: RK_FLAG_STORE_PRED is not served");
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD, RK_ERR_UNSUPPORTED, "dalton_grid_jvp: not built: kalman_type %d (standard only)",
               c->kalman_type);
    RK_REQUIRE(c->interrogate >= RK_INTERROGATE_RODEO && c->interrogate <= RK_INTERROGATE_KRAMER, RK_ERR_UNSUPPORTED,
               "dalton_grid_jvp: not built: interrogate id %d (rodeo, schober, kramer)", c->interrogate);
    RK_REQUIRE(c->n_bmeas == 1, RK_ERR_UNSUPPORTED, "dalton_grid_jvp: not built: n_bmeas = %d (1 only)", c->n_bmeas);
    RK_REQUIRE(n_bobs == 1, RK_ERR_UNSUPPORTED, "dalton_grid_jvp: not built: n_bobs = %d (1 only: the derivative of the "
               "eigendecomposition's cut-off density is out of scope)", n_bobs);
    if (is_user_rhs(c->rhs_id)) return user_dalton_grad_check(c);
    bool known = false, fits = false;
    with_builtin_rhs(c->rhs_id, [&](auto rhs) {
        using RHS = decltype(rhs);
        if constexpr (dalton_grad_has_rhs<RHS>()) {
            known = true;
            fits = c->n_bstate >= 2 && c->n_bstate <= dalton_grad_pmax<RHS>();
        }
    });
    RK_REQUIRE(known, RK_ERR_UNSUPPORTED, "dalton_grid_jvp: not built: rhs %d (fitzhugh_nagumo and lorenz63)", c->rhs_id);
    RK_REQUIRE(builtin_has_n_block(c->rhs_id, c->n_block), RK_ERR_UNSUPPORTED, "dalton_grid_jvp: rhs %d needs another n_block than %d",
               c->rhs_id, c->n_block);
    RK_REQUIRE(fits, RK_ERR_UNSUPPORTED, "dalton_grid_jvp: not built: rhs %d at n_bstate %d (the instance needs more scratch than "
               "dalton_grid's kernel at the same parameters)", c->rhs_id, c->n_bstate);
    return RK_OK;
}

// `hy`: null for rk_dalton_grid_jvp, the hyper directions for rk_dalton_grid_jvp_hyper (dalton_grid_jvp_hyper_kernel)
// The hyper form's instances (dalton_grid_jvp_hyper_kernel) ship by the rule above with dalton_grid_jvp_kernel
// <RHS, P, ITG> as the yardstick.  All twelve pass without scratch (profiles/hyper_grad_code_objects.txt; Lorenz63 at 3 with rodeo
// takes the last of the 512 registers), so rk_dalton_grid_jvp_hyper serves what rk_dalton_grid_jvp serves.
static int dalton_grid_jvp_launch(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, const GridArgs& ga,
                                  const JvpDirs& dir, const JvpHyper* hy, double* value, double* dvalue) {
    const auto user = [&] {
        return hy ? user_dalton_grad_hyper(h, c, a, o, ga, dir, *hy, a.B * dir.K, value, dvalue)
                  : user_dalton_grad(h, c, a, o, ga, dir, a.B * dir.K, value, dvalue);
    };
    return launch_by_rhs(c, a, user, [&](auto rhs) {
        using RHS = decltype(rhs);
        if constexpr (dalton_grad_has_rhs<RHS>()) {
            const LaunchGeom g = dalton_lane_geom(a.B * dir.K, true);       // 32 (trajectory, direction) items per wave
            // (one writer per element: nothing to clear)
            if (hy)
                return launch_fwd_instance<2, 3, RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(
                    h, c, "dalton_grid_jvp_hyper_kernel", "dalton_grid_jvp_hyper", [&](auto P, auto I) {
                        hipLaunchKernelGGL((dalton_grid_jvp_hyper_kernel<RHS, P, I>), g.grid, g.block, 0, h->stream, a, o, ga, dir, *hy,
                                           value, dvalue);
                    });
            return launch_fwd_instance<2, dalton_grad_pmax<RHS>(), RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(
                h, c, "dalton_grid_jvp_kernel", "dalton_grid_jvp", [&](auto P, auto I) {
                    hipLaunchKernelGGL((dalton_grid_jvp_kernel<RHS, P, I>), g.grid, g.block, 0, h->stream, a, o, ga, dir, value, dvalue);
                });
        } else {
            return (int)RK_ERR_UNSUPPORTED;                                 // (dalton_grad_check has refused it)
        }
    });
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_dalton_grid_jvp(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const double* obs, const double* obs_weight,
                       const double* obs_var, const int32_t* obs_ind, int32_t n_obs, int32_t n_bobs, const rk_grid_in* g,
                       int32_t n_dir, const double* dtheta, int32_t dtheta_batched, const double* dinit, int32_t dinit_batched,
                       double* value, double* dvalue) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_dalton_grid_jvp: null cfg");
    int rc = dalton_grad_check(c, n_bobs, n_dir);                   // (the configuration alone, before anything else is looked at)
    if (rc) return rc;
    RK_REQUIRE(h && g && value && dvalue, RK_ERR_INVALID, "rk_dalton_grid_jvp: null argument");
    DaltonObs o;
    GridArgs ga;
    rc = dalton_grid_inputs("rk_dalton_grid_jvp", c, in, obs, obs_weight, obs_var, obs_ind, n_obs, g, o, ga);
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, nullptr, a);
    const JvpDirs dir{dtheta, dinit, dtheta_batched != 0, dinit_batched != 0, n_dir};
    return dalton_grid_jvp_launch(h, c, a, o, ga, dir, nullptr, value, dvalue);
}

int rk_dalton_grid_jvp_hyper(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const double* obs, const double* obs_weight,
                             const double* obs_var, const int32_t* obs_ind, int32_t n_obs, int32_t n_bobs, const rk_grid_in* g,
                             int32_t n_dir, const double* dtheta, int32_t dtheta_batched, const double* dinit, int32_t dinit_batched,
                             const double* dlog_sigma, int32_t dlog_sigma_batched, const double* dlog_obs_var,
                             int32_t dlog_obs_var_batched, double* value, double* dvalue) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_dalton_grid_jvp_hyper: null cfg");
    int rc = dalton_grad_check(c, n_bobs, n_dir);                   // (the configuration alone, before anything else is looked at)
    if (rc) return rc;
    RK_REQUIRE(h && g && value && dvalue, RK_ERR_INVALID, "rk_dalton_grid_jvp_hyper: null argument");
    DaltonObs o;
    GridArgs ga;
    rc = dalton_grid_inputs("rk_dalton_grid_jvp_hyper", c, in, obs, obs_weight, obs_var, obs_ind, n_obs, g, o, ga);
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, nullptr, a);
    const JvpDirs dir{dtheta, dinit, dtheta_batched != 0, dinit_batched != 0, n_dir};
    const JvpHyper hy{dlog_sigma, dlog_obs_var, dlog_sigma_batched != 0, dlog_obs_var_batched != 0};
    return dalton_grid_jvp_launch(h, c, a, o, ga, dir, &hy, value, dvalue);
}

}  // extern "C"
