// solve_mv_dynamic / solve_sim_dynamic (an addition): host side of rk_solve_dynamic, the solver with
// the prior variance of every step scaled, per block, by the estimate made at that step (dynamic_kernels.hpp), and the two
// backward kernels.  One route: the lanes on batch-minor records -- dynamic_fwd_kernel, one lane per trajectory, then
// dynamic_bwd_mv_kernel or dynamic_bwd_sim_kernel, one lane per (trajectory, block): the passes of bwd_mv_kernel /
// bwd_sim_kernel (lane_backward.hpp: bwd_smooth_lane / bwd_sample_lane over bwd_walk) under the prediction policy ScaledPrior,
// Q Sigma_f[n] Q^T + scale[n] R.  Standard form, n_bstate 2..5 (2..4 with three or more blocks).  No workspace.
#include <cmath>
#include "common.hpp"
#include "rhs.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "grid_entry.hpp"
#include "dynamic_kernels.hpp"
#include "lane_backward.hpp"

namespace rk {

// ---- backward passes: one lane per (block, trajectory) -----------------------------------------------------------
// bwd_walk's prediction policy with the prior variance of step n -> n + 1 scaled by scale[n], which travels with filt[n]
template <int P>
struct ScaledPrior {
    const double* __restrict__ scale;
    using Datum = double;
    __device__ __forceinline__ double fetch(const SolveArgs& a, const BwdLane<P>& ln, int n) const {
        return *bm_item(scale, 1, ln.B, a.D, n, ln.blk, ln.b);
    }
    __device__ __forceinline__ void predict(const BwdLane<P>& ln, double c, const double (&mf)[P], const double (&Sf)[P][P],
                                            double (&mp)[P], double (&Sp)[P][P]) const {
        dynamic_propagate<P>(ln.Q, mf, Sf, mp, Sp);      // pred[n+1] from filt[n] and scale[n]
        dynamic_add_noise<P>(Sp, c, ln.R, Sp);
    }
    __device__ __forceinline__ const auto& trans(const BwdLane<P>& ln, const Datum&) const { return ln.Q; }
};

template <int P>
__global__ void __launch_bounds__(64) dynamic_bwd_mv_kernel(SolveArgs a, const double* __restrict__ scale) {
    BwdLane<P> ln;
    if (ln.init(a)) bwd_smooth_lane<P>(a, ln, ScaledPrior<P>{scale});
}

template <int P>
__global__ void __launch_bounds__(64) dynamic_bwd_sim_kernel(SolveArgs a, const double* __restrict__ scale) {
    BwdLane<P> ln;
    if (ln.init(a)) bwd_sample_lane<P>(a, ln, ScaledPrior<P>{scale});
}

// ---- dispatch ---------------------------------------------------------------------------------------------------
constexpr int DYNAMIC_PMIN = 2, DYNAMIC_PMAX = 5;
// largest n_bstate of the forward instances: with three blocks at n_bstate = 5 the lane needs more scratch than evidence_kernel
// at the same (RHS, P) (716 / 588 / 588 against 604 / 500 / 548 B for Lorenz63), which is the rule an instance ships by
constexpr int DYNAMIC_PMAX_THREE_BLOCKS = 4;
template <class RHS>
constexpr int dynamic_pmax() { return RHS::D >= 3 ? DYNAMIC_PMAX_THREE_BLOCKS : DYNAMIC_PMAX; }

// Is this call served?  Decided on the configuration, the mode and scale_min alone: RK_OK, RK_ERR_INVALID (sizes, mode,
// scale_min) or RK_ERR_UNSUPPORTED.
static int dynamic_check(const rk_solve_cfg* c, int mode, double scale_min) {
    RK_REQUIRE(c->n_traj >= 1 && c->n_steps >= 1 && c->n_block >= 1 && c->n_bstate >= 1 && c->n_bmeas >= 1, RK_ERR_INVALID,
               "dynamic: non-positive dimension (n_traj=%d n_steps=%d n_block=%d n_bstate=%d n_bmeas=%d)", c->n_traj,
               c->n_steps, c->n_block, c->n_bstate, c->n_bmeas);
    RK_REQUIRE(mode == RK_MODE_MV || mode == RK_MODE_SIM, RK_ERR_INVALID, "dynamic: mode must be RK_MODE_MV or RK_MODE_SIM, got %d",
               mode);
    RK_REQUIRE(std::isfinite(scale_min) && scale_min >= 0.0, RK_ERR_INVALID, "dynamic: scale_min must be finite and >= 0, got %g",
               scale_min);
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD || c->kalman_type == RK_KALMAN_SQRT, RK_ERR_UNSUPPORTED,
               "dynamic: unknown kalman_type %d", c->kalman_type);
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD, RK_ERR_UNSUPPORTED, "dynamic: kalman_type square-root is not built");
    RK_REQUIRE(c->interrogate != RK_INTERROGATE_CHKREBTII, RK_ERR_UNSUPPORTED,
               "dynamic: interrogate_chkrebtii is not served (its point is drawn from the predicted variance, which here "
               "depends on the point through the scale)");
    RK_REQUIRE(c->interrogate >= RK_INTERROGATE_RODEO && c->interrogate <= RK_INTERROGATE_KRAMER, RK_ERR_UNSUPPORTED,
               "dynamic: interrogate id %d is not supported (rodeo, schober, kramer)", c->interrogate);
    RK_REQUIRE(c->n_bmeas == 1, RK_ERR_UNSUPPORTED, "dynamic: n_bmeas = 1 only (the dense / indep_init form is not served), "
               "got %d", c->n_bmeas);
    RK_REQUIRE(c->n_bstate >= DYNAMIC_PMIN && c->n_bstate <= DYNAMIC_PMAX, RK_ERR_UNSUPPORTED,
               "dynamic: n_bstate in %d..%d, got %d", DYNAMIC_PMIN, DYNAMIC_PMAX, c->n_bstate);
    RK_REQUIRE(c->n_block < 3 || c->n_bstate <= DYNAMIC_PMAX_THREE_BLOCKS, RK_ERR_UNSUPPORTED,
               "dynamic: n_bstate up to %d with three or more blocks (the lane kernel spills more than solve_evidence's), got %d",
               DYNAMIC_PMAX_THREE_BLOCKS, c->n_bstate);
    if (is_user_rhs(c->rhs_id)) return user_lane_check(c, "dynamic");
    RK_REQUIRE(with_builtin_rhs(c->rhs_id, [](auto) {}), RK_ERR_UNSUPPORTED, "dynamic: unknown rhs_id %d", c->rhs_id);
    RK_REQUIRE(builtin_has_n_block(c->rhs_id, c->n_block), RK_ERR_UNSUPPORTED, "dynamic: rhs %d needs another n_block than %d",
               c->rhs_id, c->n_block);
    return RK_OK;
}

// ---- launches (grid_entry.hpp's patterns) -------------------------------------------------------------------------------
// The backward launch stands first: a kernel is emitted where its launch is first seen, and the code object keeps the order it
// has had -- the backward kernels, then dynamic_fwd_kernel's instances.
static int launch_dynamic_bwd(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, int mode, const double* scale) {
    const LaunchGeom g = bwd_lane_geom(a.B, a.D);
    return launch_bwd_instance<DYNAMIC_PMIN, DYNAMIC_PMAX>(h, c, mode, "dynamic_bwd_mv_kernel", "dynamic_bwd_sim_kernel", "dynamic",
                                                           [&](auto P, bool sim) {
        if (sim) hipLaunchKernelGGL((dynamic_bwd_sim_kernel<P>), g.grid, g.block, 0, h->stream, a, scale);
        else hipLaunchKernelGGL((dynamic_bwd_mv_kernel<P>), g.grid, g.block, 0, h->stream, a, scale);
    });
}

// the forward pass for a built-in or a user right-hand side
static int dynamic_forward(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, double scale_min, double* scale,
                           double* logdens) {
    return launch_by_rhs(c, a, [&] { return user_dynamic(h, c, a, scale_min, scale, logdens); }, [&](auto rhs) {
        using RHS = decltype(rhs);
        const LaunchGeom g = fwd_lane_geom(a.B);
        return launch_fwd_instance<DYNAMIC_PMIN, dynamic_pmax<RHS>(), RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(
            h, c, "dynamic_fwd_kernel", "dynamic", [&](auto P, auto I) {
                hipLaunchKernelGGL((dynamic_fwd_kernel<RHS, P, I>), g.grid, g.block, 0, h->stream, a, scale_min, scale, logdens);
            });
    });
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_solve_dynamic(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, int32_t mode,
                     double scale_min, double* scale, double* logdens) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_solve_dynamic: null cfg");
    int rc = dynamic_check(c, mode, scale_min);                     // (the configuration alone, before anything else is looked at)
    if (rc) return rc;
    RK_REQUIRE(h && out && scale && logdens, RK_ERR_INVALID, "rk_solve_dynamic: null argument");
    rc = check_cfg(c, in);
    if (rc) return rc;
    RK_REQUIRE(out->mean_state && out->var_state, RK_ERR_INVALID, "rk_solve_dynamic: out->mean_state / var_state must not be NULL");
    RK_REQUIRE(mode != RK_MODE_SIM || out->x_state, RK_ERR_INVALID, "rk_solve_dynamic: RK_MODE_SIM needs out->x_state");
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, out, a);
    rc = dynamic_forward(h, c, a, scale_min, scale, logdens);
    if (rc) return rc;
    return launch_dynamic_bwd(h, c, a, mode, scale);
}

}  // extern "C"
