// dalton_grid_jvp / dalton_grid_grad / dalton_grad (an addition): host side of rk_dalton_grid_jvp,
// directional derivatives of rk_dalton_grid_loglik's value with respect to the ODE parameters and the initial state.  One
// route: dalton_grid_jvp_kernel (dalton_grad_kernels.hpp), one (trajectory, direction) item per lane pair, 32 items per wave.
// Standard form, n_bmeas = 1, n_bobs = 1, built-in FitzHugh-Nagumo and Lorenz63, or a user right-hand side of the gradient kind
// (hiprtc, rhs_jit.hip's JIT_DALTON_GRAD).  rk_dalton_grid_jvp_hyper (section 7 (25)) is the same entry with the log sigma / log
// observation variance directions, on dalton_grid_jvp_hyper_kernel (JIT_DALTON_GRAD_HYPER).  No workspace.  The configuration
// check (grad_check, shared with fenrir_grad.hip and worded "not built: ..."), the grid's staging (through dalton_grid_inputs) and
// the launch patterns are grid_entry.hpp's.
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

// Is this call served?  grid_entry.hpp's grad_check with this entry's item count (one lane pair per item), rule for a user
// right-hand side, range and wording.
static int dalton_grad_check(const rk_solve_cfg* c, int n_bobs, int n_dir) {
    int pmax = 0;
    with_builtin_rhs(c->rhs_id, [&](auto rhs) { pmax = dalton_grad_pmax<decltype(rhs)>(); });
    return grad_check("dalton_grid_jvp", c, n_bobs, n_dir, false, user_dalton_grad_check, pmax,
                      "the instance needs more scratch than dalton_grid's kernel at the same parameters");
}

// `hy`: null for rk_dalton_grid_jvp, the hyper directions for rk_dalton_grid_jvp_hyper (dalton_grid_jvp_hyper_kernel)
// The hyper form's instances (dalton_grid_jvp_hyper_kernel) ship by the rule above with dalton_grid_jvp_kernel
// <RHS, P, ITG> as the yardstick.  All twelve pass without scratch (profiles/hyper_grad_code_objects.txt; Lorenz63 at 3 with rodeo
// takes the last of the 512 registers), so rk_dalton_grid_jvp_hyper serves what rk_dalton_grid_jvp serves.
static int dalton_grid_jvp_launch(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, const GridArgs& ga,
                                  const JvpDirs& dir, const JvpHyper* hy, double* value, double* dvalue) {
    const auto user = [&] { return user_dalton_grad(h, c, a, o, ga, dir, hy, a.B * dir.K, value, dvalue); };
    return launch_by_rhs(c, a, user, [&](auto rhs) {
        using RHS = decltype(rhs);
        if constexpr (grad_has_rhs<RHS>()) {
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

// the body of rk_dalton_grid_jvp (hy null) and rk_dalton_grid_jvp_hyper
static int dalton_grid_jvp_run(const char* who, rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const double* obs,
                               const double* obs_weight, const double* obs_var, const int32_t* obs_ind, int32_t n_obs, int32_t n_bobs,
                               const rk_grid_in* g, const JvpDirs& dir, const JvpHyper* hy, double* value, double* dvalue) {
    RK_REQUIRE(c, RK_ERR_INVALID, "%s: null cfg", who);
    int rc = dalton_grad_check(c, n_bobs, dir.K);                   // (the configuration alone, before anything else is looked at)
    if (rc) return rc;
    RK_REQUIRE(h && g && value && dvalue, RK_ERR_INVALID, "%s: null argument", who);
    DaltonObs o;
    GridArgs ga;
    rc = dalton_grid_inputs(who, c, in, obs, obs_weight, obs_var, obs_ind, n_obs, g, o, ga);
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, nullptr, a);
    return dalton_grid_jvp_launch(h, c, a, o, ga, dir, hy, value, dvalue);
}

extern "C" {

int rk_dalton_grid_jvp(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const double* obs, const double* obs_weight,
                       const double* obs_var, const int32_t* obs_ind, int32_t n_obs, int32_t n_bobs, const rk_grid_in* g,
                       int32_t n_dir, const double* dtheta, int32_t dtheta_batched, const double* dinit, int32_t dinit_batched,
                       double* value, double* dvalue) {
    const JvpDirs dir{dtheta, dinit, dtheta_batched != 0, dinit_batched != 0, n_dir};
    return dalton_grid_jvp_run("rk_dalton_grid_jvp", h, c, in, obs, obs_weight, obs_var, obs_ind, n_obs, n_bobs, g, dir, nullptr, value,
                               dvalue);
}

int rk_dalton_grid_jvp_hyper(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const double* obs, const double* obs_weight,
                             const double* obs_var, const int32_t* obs_ind, int32_t n_obs, int32_t n_bobs, const rk_grid_in* g,
                             int32_t n_dir, const double* dtheta, int32_t dtheta_batched, const double* dinit, int32_t dinit_batched,
                             const double* dlog_sigma, int32_t dlog_sigma_batched, const double* dlog_obs_var,
                             int32_t dlog_obs_var_batched, double* value, double* dvalue) {
    const JvpDirs dir{dtheta, dinit, dtheta_batched != 0, dinit_batched != 0, n_dir};
    const JvpHyper hy{dlog_sigma, dlog_obs_var, dlog_sigma_batched != 0, dlog_obs_var_batched != 0};
    return dalton_grid_jvp_run("rk_dalton_grid_jvp_hyper", h, c, in, obs, obs_weight, obs_var, obs_ind, n_obs, n_bobs, g, dir, &hy, value,
                               dvalue);
}

}  // extern "C"
