// solve_evidence_grid / solve_mv_dynamic_grid / solve_sim_dynamic_grid (an addition): host side of
// rk_solve_evidence_grid and rk_solve_dynamic_grid, the two calibration tools on the non-uniform grid of rk_solve_grid, and the
// two backward kernels of the dynamic solver on that grid.  One route each, the lanes on batch-minor records:
// grid_evidence_kernel, or grid_dynamic_fwd_kernel (grid_calib_kernels.hpp), one lane per trajectory, then
// grid_dynamic_bwd_mv_kernel or grid_dynamic_bwd_sim_kernel, one lane per (trajectory, block): the passes of bwd_mv_kernel /
// bwd_sim_kernel (lane_backward.hpp: bwd_smooth_lane / bwd_sample_lane over bwd_walk) under the prediction policy
// ScaledSlotPrior, Q_n Sigma_f[n] Q_n^T + scale[n] R_n with the gain from Q_n.  Standard form, n_bmeas = 1.  No workspace.
#include <cmath>
#include "common.hpp"
#include "rhs.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
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

// what both entries refuse, on the configuration alone; `who` names the entry in the message
static int grid_calib_check(const rk_solve_cfg* c, const char* who, int pmin, int pmax, int pmax3) {
    RK_REQUIRE(c->n_traj >= 1 && c->n_steps >= 1 && c->n_block >= 1 && c->n_bstate >= 1 && c->n_bmeas >= 1, RK_ERR_INVALID,
               "%s: non-positive dimension (n_traj=%d n_steps=%d n_block=%d n_bstate=%d n_bmeas=%d)", who, c->n_traj,
               c->n_steps, c->n_block, c->n_bstate, c->n_bmeas);
    RK_REQUIRE((c->flags & RK_FLAG_BATCH_MINOR) != 0, RK_ERR_INVALID, "%s: cfg->flags must carry RK_FLAG_BATCH_MINOR (the "
               "records are the batch-minor ones)", who);
    RK_REQUIRE((c->flags & RK_FLAG_STORE_PRED) == 0, RK_ERR_UNSUPPORTED, "%s: RK_FLAG_STORE_PRED is not served", who);
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD || c->kalman_type == RK_KALMAN_SQRT, RK_ERR_UNSUPPORTED,
               "%s: unknown kalman_type %d", who, c->kalman_type);
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD, RK_ERR_UNSUPPORTED, "%s: kalman_type square-root is not built", who);
    RK_REQUIRE(c->interrogate != RK_INTERROGATE_CHKREBTII, RK_ERR_UNSUPPORTED,
               "%s: interrogate_chkrebtii is not served (it draws its point from the predicted variance: no scale law, and a "
               "variance that depends on the point through the scale)", who);
    RK_REQUIRE(c->interrogate >= RK_INTERROGATE_RODEO && c->interrogate <= RK_INTERROGATE_KRAMER, RK_ERR_UNSUPPORTED,
               "%s: interrogate id %d is not supported (rodeo, schober, kramer)", who, c->interrogate);
    RK_REQUIRE(c->n_bmeas == 1, RK_ERR_UNSUPPORTED, "%s: n_bmeas = 1 only (the dense / indep_init form is not served), got %d",
               who, c->n_bmeas);
    RK_REQUIRE(c->n_bstate >= pmin && c->n_bstate <= pmax, RK_ERR_UNSUPPORTED, "%s: n_bstate in %d..%d, got %d", who, pmin, pmax,
               c->n_bstate);
    RK_REQUIRE(c->n_block < 3 || c->n_bstate <= pmax3, RK_ERR_UNSUPPORTED,
               "%s: n_bstate up to %d with three or more blocks, got %d", who, pmax3, c->n_bstate);
    if (is_user_rhs(c->rhs_id)) return user_grid_calib_check(c, who);
    RK_REQUIRE(with_builtin_rhs(c->rhs_id, [](auto) {}), RK_ERR_UNSUPPORTED, "%s: unknown rhs_id %d", who, c->rhs_id);
    RK_REQUIRE(builtin_has_n_block(c->rhs_id, c->n_block), RK_ERR_UNSUPPORTED, "%s: rhs %d needs another n_block than %d", who,
               c->rhs_id, c->n_block);
    return RK_OK;
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

static int grid_in_check(const rk_grid_in* g, const char* who) {
    RK_REQUIRE(g->t && g->slot && g->q && g->r && g->n_slots >= 1, RK_ERR_INVALID,
               "%s: grid needs t, slot, q, r and n_slots >= 1 (got %d)", who, g->n_slots);
    return RK_OK;
}

// ---- launches ---------------------------------------------------------------------------------------------------
template <class RHS>
static int launch_grid_evidence(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& ga, double* logdens,
                                double* quad, double* logdet) {
    const LaunchGeom g = fwd_lane_geom(a.B);
    bool ok = false;
    dispatch_int<GRID_EVIDENCE_PMIN, grid_evidence_pmax<RHS>()>(c->n_bstate, [&](auto P) {
        dispatch_int<RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(c->interrogate, [&](auto I) {
            LaunchTimer t(h, "grid_evidence_kernel");
            hipLaunchKernelGGL((grid_evidence_kernel<RHS, P, I>), g.grid, g.block, 0, h->stream, a, ga, logdens, quad, logdet);
            t.stop();
            ok = true;
        });
    });
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "evidence_grid: no kernel for rhs %d, n_bstate %d, interrogate %d", c->rhs_id, c->n_bstate,
               c->interrogate);
    RK_HIP(hipGetLastError());
    return RK_OK;
}

template <class RHS>
static int launch_grid_dynamic_fwd(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& ga, double scale_min,
                                   double* scale, double* logdens) {
    const LaunchGeom g = fwd_lane_geom(a.B);
    bool ok = false;
    dispatch_int<GRID_DYNAMIC_PMIN, grid_dynamic_pmax<RHS>()>(c->n_bstate, [&](auto P) {
        dispatch_int<RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(c->interrogate, [&](auto I) {
            LaunchTimer t(h, "grid_dynamic_fwd_kernel");
            hipLaunchKernelGGL((grid_dynamic_fwd_kernel<RHS, P, I>), g.grid, g.block, 0, h->stream, a, ga, scale_min, scale,
                               logdens);
            t.stop();
            ok = true;
        });
    });
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "dynamic_grid: no kernel for rhs %d, n_bstate %d, interrogate %d", c->rhs_id, c->n_bstate,
               c->interrogate);
    RK_HIP(hipGetLastError());
    return RK_OK;
}

static int launch_grid_dynamic_bwd(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, int mode, const GridArgs& ga,
                                   const double* scale) {
    const LaunchGeom g = bwd_lane_geom(a.B, a.D);
    const bool sim = mode == RK_MODE_SIM;
    LaunchTimer t(h, sim ? "grid_dynamic_bwd_sim_kernel" : "grid_dynamic_bwd_mv_kernel");
    const bool ok = dispatch_int<GRID_DYNAMIC_PMIN, GRID_DYNAMIC_PMAX>(c->n_bstate, [&](auto P) {
        if (sim) hipLaunchKernelGGL((grid_dynamic_bwd_sim_kernel<P>), g.grid, g.block, 0, h->stream, a, ga, scale);
        else hipLaunchKernelGGL((grid_dynamic_bwd_mv_kernel<P>), g.grid, g.block, 0, h->stream, a, ga, scale);
    });
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "dynamic_grid: no backward kernel for n_bstate %d", c->n_bstate);
    t.stop();
    RK_HIP(hipGetLastError());
    return RK_OK;
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
    rc = grid_in_check(g, "rk_solve_evidence_grid");
    if (rc) return rc;
    rc = check_cfg(c, in);
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, nullptr, a);
    const GridArgs ga{g->t, g->slot, g->q, g->r, g->q_batched != 0, g->r_batched != 0, g->n_slots};
    if (is_user_rhs(c->rhs_id)) return user_grid_evidence(h, c, a, ga, logdens, quad, logdet);
    rc = RK_ERR_UNSUPPORTED;
    with_builtin_rhs(c->rhs_id, [&](auto rhs) {
        using RHS = decltype(rhs);
        rc = check_n_theta<RHS>(c, a);
        if (rc) return;
        rc = launch_grid_evidence<RHS>(h, c, a, ga, logdens, quad, logdet);
    });
    return rc;
}

int rk_solve_dynamic_grid(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, int32_t mode,
                          const rk_grid_in* g, double scale_min, double* scale, double* logdens) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_solve_dynamic_grid: null cfg");
    int rc = dynamic_grid_check(c, mode, scale_min);                // (cfg, mode and scale_min alone, before anything else is looked at)
    if (rc) return rc;
    RK_REQUIRE(h && out && g && scale && logdens, RK_ERR_INVALID, "rk_solve_dynamic_grid: null argument");
    rc = grid_in_check(g, "rk_solve_dynamic_grid");
    if (rc) return rc;
    rc = check_cfg(c, in);
    if (rc) return rc;
    RK_REQUIRE(out->mean_state && out->var_state, RK_ERR_INVALID,
               "rk_solve_dynamic_grid: out->mean_state / var_state must not be NULL");
    RK_REQUIRE(mode != RK_MODE_SIM || out->x_state, RK_ERR_INVALID, "rk_solve_dynamic_grid: RK_MODE_SIM needs out->x_state");
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, out, a);
    const GridArgs ga{g->t, g->slot, g->q, g->r, g->q_batched != 0, g->r_batched != 0, g->n_slots};
    if (is_user_rhs(c->rhs_id)) {
        rc = user_grid_dynamic(h, c, a, ga, scale_min, scale, logdens);
    } else {
        rc = RK_ERR_UNSUPPORTED;
        with_builtin_rhs(c->rhs_id, [&](auto rhs) {
            using RHS = decltype(rhs);
            rc = check_n_theta<RHS>(c, a);
            if (rc) return;
            rc = launch_grid_dynamic_fwd<RHS>(h, c, a, ga, scale_min, scale, logdens);
        });
    }
    if (rc) return rc;
    return launch_grid_dynamic_bwd(h, c, a, mode, ga, scale);
}

}  // extern "C"
