// solve_evidence_grid / solve_mv_dynamic_grid / solve_sim_dynamic_grid (an addition): host side of
// rk_solve_evidence_grid and rk_solve_dynamic_grid, the two calibration tools on the non-uniform grid of rk_solve_grid, and the
// two backward kernels of the dynamic solver on that grid.  One route each, the lanes on batch-minor records:
// grid_evidence_kernel, or grid_dynamic_fwd_kernel (grid_calib_kernels.hpp), one lane per trajectory, then
// grid_dynamic_bwd_mv_kernel or grid_dynamic_bwd_sim_kernel, one lane per (trajectory, block): the passes of bwd_mv_kernel /
// bwd_sim_kernel (lane_backward.hpp: bwd_smooth_lane / bwd_sample_lane over bwd_walk) under the prediction policy
// ScaledSlotPrior, Q_n Sigma_f[n] Q_n^T + scale[n] R_n with the gain from Q_n.  Standard form, n_bmeas = 1.  No workspace.
// The pieces of the configuration check, the grid's staging and the launch patterns are grid_entry.hpp's.
#include <cmath>
#include "common.hpp"
#include "rhs.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "grid_entry.hpp"
#include "grid_calib_kernels.hpp"
#include "lane_backward.hpp"

namespace rk {

// ---- backward passes: one lane per (block, trajectory) -----------------------------------------------------------
// bwd_walk's prediction policy with the prior pair of step n -> n + 1 and the scale that the forward pass put on that step's
// R: both are fetched next to filt[n] (so one step ahead of their use, like the record), and the pair's Q is the transition
// matrix of that step's smoothing gain.  The lane's own Q, R are not read.
template <int P>
struct ScaledSlotPrior {
    GridArgs g;
    const double* __restrict__ scale;
    struct Datum { double Q[P][P], R[P][P], c; };
    __device__ __forceinline__ Datum fetch(const SolveArgs& a, const BwdLane<P>& ln, int n) const {
        Datum d;
        grid_load_pair<P>(g, a.B, a.D, grid_slot(g, n), ln.blk, ln.b, d.Q, d.R);
        d.c = *bm_item(scale, 1, ln.B, a.D, n, ln.blk, ln.b);
        return d;
    }
    __device__ __forceinline__ void predict(const BwdLane<P>&, const Datum& d, const double (&mf)[P], const double (&Sf)[P][P],
                                            double (&mp)[P], double (&Sp)[P][P]) const {
        dynamic_propagate<P>(d.Q, mf, Sf, mp, Sp);       // pred[n+1] from filt[n], the pair of step n and scale[n]
        dynamic_add_noise<P>(Sp, d.c, d.R, Sp);
    }
    __device__ __forceinline__ const auto& trans(const BwdLane<P>&, const Datum& d) const { return d.Q; }
};

template <int P>
__global__ void __launch_bounds__(64) grid_dynamic_bwd_mv_kernel(SolveArgs a, GridArgs g, const double* __restrict__ scale) {
    BwdLane<P> ln;
    if (ln.init(a)) bwd_smooth_lane<P>(a, ln, ScaledSlotPrior<P>{g, scale});
}

template <int P>
__global__ void __launch_bounds__(64) grid_dynamic_bwd_sim_kernel(SolveArgs a, GridArgs g, const double* __restrict__ scale) {
    BwdLane<P> ln;
    if (ln.init(a)) bwd_sample_lane<P>(a, ln, ScaledSlotPrior<P>{g, scale});
}

// ---- what is served ---------------------------------------------------------------------------------------------
// n_bstate of the forward instances: the ranges of solve_evidence's standard lanes and of solve_mv_dynamic.  An instance ships
// only if it needs no more scratch than evidence_kernel / dynamic_fwd_kernel at the same (RHS, P, ITG): DESIGN.md section 7 (18)
// and profiles/grid_calib_code_objects.txt have the figures of every instance.
constexpr int GRID_EVIDENCE_PMIN = 2, GRID_EVIDENCE_PMAX = 6, GRID_EVIDENCE_PMAX_THREE_BLOCKS = 5;
constexpr int GRID_DYNAMIC_PMIN = 2, GRID_DYNAMIC_PMAX = 5, GRID_DYNAMIC_PMAX_THREE_BLOCKS = 4;
template <class RHS>
constexpr int grid_evidence_pmax() { return RHS::D >= 3 ? GRID_EVIDENCE_PMAX_THREE_BLOCKS : GRID_EVIDENCE_PMAX; }
template <class RHS>
constexpr int grid_dynamic_pmax() { return RHS::D >= 3 ? GRID_DYNAMIC_PMAX_THREE_BLOCKS : GRID_DYNAMIC_PMAX; }

// what both entries refuse, on the configuration alone (grid_entry.hpp's pieces); `who` names the entry in the message
static int grid_calib_check(const rk_solve_cfg* c, const char* who, int pmin, int pmax, int pmax3) {
    int rc = grid_sizes_check(who, c);
    if (rc) return rc;
    rc = grid_served_check({who, GRID_RECORDS, RK_INTERROGATE_KRAMER,
                            "it draws its point from the predicted variance: no scale law, and a variance that depends on the point "
                            "through the scale", pmin, pmax, pmax3}, c);
    if (rc) return rc;
    return grid_rhs_check(who, c);
}

static int evidence_grid_check(const rk_solve_cfg* c) {
    return grid_calib_check(c, "evidence_grid", GRID_EVIDENCE_PMIN, GRID_EVIDENCE_PMAX, GRID_EVIDENCE_PMAX_THREE_BLOCKS);
}

// (cfg, the mode and scale_min alone)
static int dynamic_grid_check(const rk_solve_cfg* c, int mode, double scale_min) {
    RK_REQUIRE(mode == RK_MODE_MV || mode == RK_MODE_SIM, RK_ERR_INVALID,
               "dynamic_grid: mode must be RK_MODE_MV or RK_MODE_SIM, got %d", mode);
    RK_REQUIRE(std::isfinite(scale_min) && scale_min >= 0.0, RK_ERR_INVALID,
               "dynamic_grid: scale_min must be finite and >= 0, got %g", scale_min);
    return grid_calib_check(c, "dynamic_grid", GRID_DYNAMIC_PMIN, GRID_DYNAMIC_PMAX, GRID_DYNAMIC_PMAX_THREE_BLOCKS);
}

// ---- launches (grid_entry.hpp's patterns) -------------------------------------------------------------------------------
// The backward launch stands first: a kernel is emitted where its launch is first seen, and the code object keeps the order it
// has had -- the backward kernels, then grid_evidence_kernel's instances, then grid_dynamic_fwd_kernel's.
static int launch_grid_dynamic_bwd(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, int mode, const GridArgs& ga,
                                   const double* scale) {
    const LaunchGeom g = bwd_lane_geom(a.B, a.D);
    return launch_bwd_instance<GRID_DYNAMIC_PMIN, GRID_DYNAMIC_PMAX>(h, c, mode, "grid_dynamic_bwd_mv_kernel",
                                                                     "grid_dynamic_bwd_sim_kernel", "dynamic_grid",
                                                                     [&](auto P, bool sim) {
        if (sim) hipLaunchKernelGGL((grid_dynamic_bwd_sim_kernel<P>), g.grid, g.block, 0, h->stream, a, ga, scale);
        else hipLaunchKernelGGL((grid_dynamic_bwd_mv_kernel<P>), g.grid, g.block, 0, h->stream, a, ga, scale);
    });
}

// the forward passes, for a built-in or a user right-hand side
static int grid_evidence_forward(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& ga, double* logdens,
                                 double* quad, double* logdet) {
    return launch_by_rhs(c, a, [&] { return user_grid_evidence(h, c, a, ga, logdens, quad, logdet); }, [&](auto rhs) {
        using RHS = decltype(rhs);
        const LaunchGeom g = fwd_lane_geom(a.B);
        return launch_fwd_instance<GRID_EVIDENCE_PMIN, grid_evidence_pmax<RHS>(), RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(
            h, c, "grid_evidence_kernel", "evidence_grid", [&](auto P, auto I) {
                hipLaunchKernelGGL((grid_evidence_kernel<RHS, P, I>), g.grid, g.block, 0, h->stream, a, ga, logdens, quad, logdet);
            });
    });
}

static int grid_dynamic_forward(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& ga, double scale_min,
                                double* scale, double* logdens) {
    return launch_by_rhs(c, a, [&] { return user_grid_dynamic(h, c, a, ga, scale_min, scale, logdens); }, [&](auto rhs) {
        using RHS = decltype(rhs);
        const LaunchGeom g = fwd_lane_geom(a.B);
        return launch_fwd_instance<GRID_DYNAMIC_PMIN, grid_dynamic_pmax<RHS>(), RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(
            h, c, "grid_dynamic_fwd_kernel", "dynamic_grid", [&](auto P, auto I) {
                hipLaunchKernelGGL((grid_dynamic_fwd_kernel<RHS, P, I>), g.grid, g.block, 0, h->stream, a, ga, scale_min, scale,
                                   logdens);
            });
    });
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_solve_evidence_grid(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_grid_in* g, double* logdens,
                           double* quad, double* logdet) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_solve_evidence_grid: null cfg");
    int rc = evidence_grid_check(c);                                // (the configuration alone, before anything else is looked at)
    if (rc) return rc;
    RK_REQUIRE(h && g && logdens && quad && logdet, RK_ERR_INVALID, "rk_solve_evidence_grid: null argument");
    GridArgs ga;
    rc = grid_args("rk_solve_evidence_grid", g, ga);
    if (rc) return rc;
    rc = check_cfg(c, in);
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, nullptr, a);
    return grid_evidence_forward(h, c, a, ga, logdens, quad, logdet);
}

int rk_solve_dynamic_grid(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, int32_t mode,
                          const rk_grid_in* g, double scale_min, double* scale, double* logdens) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_solve_dynamic_grid: null cfg");
    int rc = dynamic_grid_check(c, mode, scale_min);                // (cfg, mode and scale_min alone, before anything else is looked at)
    if (rc) return rc;
    RK_REQUIRE(h && out && g && scale && logdens, RK_ERR_INVALID, "rk_solve_dynamic_grid: null argument");
    GridArgs ga;
    rc = grid_args("rk_solve_dynamic_grid", g, ga);
    if (rc) return rc;
    rc = check_cfg(c, in);
    if (rc) return rc;
    rc = grid_out_check("rk_solve_dynamic_grid", out, mode);
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, out, a);
    rc = grid_dynamic_forward(h, c, a, ga, scale_min, scale, logdens);
    if (rc) return rc;
    return launch_grid_dynamic_bwd(h, c, a, mode, ga, scale);
}

}  // extern "C"
