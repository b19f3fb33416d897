// solve_evidence (an addition): host side of rk_solve_evidence, the solver's own marginal
// likelihood log p(Z_{1:N} = 0) with its per-block parts.  Three routes:
//   tiles  -- evidence_tile3_kernel (evidence_tile3_kernels.hpp): standard form, n_bstate = 3, n_block 1..4, every
//             right-hand side the tile solver accepts in filter mode (a user one: whenever this kernel builds for it);
//   lanes  -- evidence_kernel (evidence_kernels.hpp): standard form, n_bstate 2..6 (2..5 with three or more blocks);
//   square-root lanes -- evidence_sqrt_kernel (evidence_kernels.hpp): n_bstate 2..8.
// RK_EVIDENCE_LANES=1, read per call, forces the lanes where the tile route exists (cross-checks).  Nothing but the three
// outputs is written; there is no workspace.
#include <cstdlib>
#include "common.hpp"
#include "rhs.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "evidence_kernels.hpp"
#include "evidence_tile3_kernels.hpp"

namespace rk {

// Is this configuration served?  Decided on the configuration alone: RK_OK, RK_ERR_INVALID (sizes) or RK_ERR_UNSUPPORTED.
static int evidence_check(const rk_solve_cfg* c) {
    RK_REQUIRE(c->n_traj >= 1 && c->n_steps >= 1 && c->n_block >= 1 && c->n_bstate >= 1 && c->n_bmeas >= 1, RK_ERR_INVALID,
               "evidence: non-positive dimension (n_traj=%d n_steps=%d n_block=%d n_bstate=%d n_bmeas=%d)", c->n_traj,
               c->n_steps, c->n_block, c->n_bstate, c->n_bmeas);
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD || c->kalman_type == RK_KALMAN_SQRT, RK_ERR_UNSUPPORTED,
               "evidence: unknown kalman_type %d", c->kalman_type);
    RK_REQUIRE(c->interrogate != RK_INTERROGATE_CHKREBTII, RK_ERR_UNSUPPORTED,
               "evidence: interrogate_chkrebtii is not served (it draws its point from the predicted variance, so the scale "
               "law behind the closed-form calibration does not hold)");
    RK_REQUIRE(c->interrogate >= RK_INTERROGATE_RODEO && c->interrogate <= RK_INTERROGATE_KRAMER, RK_ERR_UNSUPPORTED,
               "evidence: interrogate id %d is not supported (rodeo, schober, kramer)", c->interrogate);
    RK_REQUIRE(c->n_bmeas == 1, RK_ERR_UNSUPPORTED, "evidence: n_bmeas = 1 only (the dense / indep_init form is not served), "
               "got %d", c->n_bmeas);
    const bool sq = c->kalman_type == RK_KALMAN_SQRT;
    const int hi = sq ? 8 : 6;
    RK_REQUIRE(c->n_bstate >= 2 && c->n_bstate <= hi, RK_ERR_UNSUPPORTED, "evidence: n_bstate in 2..%d (%s form), got %d", hi,
               sq ? "square-root" : "standard", c->n_bstate);
    if (is_user_rhs(c->rhs_id)) {
        const int rc = user_lane_check(c, "evidence");               // (n_block / n_bmeas of the registration; the range is the one above)
        if (rc) return rc;
        RK_REQUIRE(sq || c->n_block < 3 || c->n_bstate <= 5, RK_ERR_UNSUPPORTED,
                   "evidence: n_bstate up to 5 with three or more blocks (the lane kernel spills), got %d", c->n_bstate);
        return RK_OK;
    }
    bool known = false, fits = false;
    int pmax = hi;
    with_builtin_rhs(c->rhs_id, [&](auto rhs) {
        known = true;
        fits = decltype(rhs)::D == c->n_block;
        if (!sq) pmax = dalton_pmax<decltype(rhs)>();
    });
    RK_REQUIRE(known, RK_ERR_UNSUPPORTED, "evidence: unknown rhs_id %d", c->rhs_id);
    RK_REQUIRE(fits, RK_ERR_UNSUPPORTED, "evidence: rhs %d needs another n_block than %d", c->rhs_id, c->n_block);
    RK_REQUIRE(c->n_bstate <= pmax, RK_ERR_UNSUPPORTED, "evidence: rhs %d supports n_bstate up to %d, got %d", c->rhs_id, pmax,
               c->n_bstate);
    return RK_OK;
}

// Does the tile route serve this (served, evidence_check) configuration?
static bool evidence_tile_route(const rk_solve_cfg* c) {
    if (c->kalman_type != RK_KALMAN_STANDARD || c->n_bstate != 3 || c->n_block > 4) return false;
    const char* e = getenv("RK_EVIDENCE_LANES");
    if (e && atoi(e) != 0) return false;
    if (is_user_rhs(c->rhs_id)) return user_evidence_tile_available(c);     // (builds the kernel it is about to launch, nothing else)
    rk_solve_cfg plain = *c;
    plain.flags = 0;
    return tile3_supported(&plain, RK_MODE_FILTER);
}

enum class EvRoute { Tile, Lane, Sqrt };

template <class RHS>
static int launch_evidence_rhs(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, EvRoute route, double* logdens,
                               double* quad, double* logdet) {
    bool ok = false;
    if (route == EvRoute::Tile) {
        if constexpr (RHS::D <= 4 && RHS::NDEP == 1) {
            const LaunchGeom g = dalton_tile_geom(a.B, RHS::D, false);
            dispatch_int<RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(c->interrogate, [&](auto I) {
                LaunchTimer t(h, "evidence_tile3_kernel");
                hipLaunchKernelGGL((evidence_tile3_kernel<RHS, I>), g.grid, g.block, 0, h->stream, a, logdens, quad, logdet);
                t.stop();
                ok = true;
            });
        }
    } else if (route == EvRoute::Lane) {
        const LaunchGeom g = fwd_lane_geom(a.B);
        dispatch_int<2, dalton_pmax<RHS>()>(c->n_bstate, [&](auto P) {
            dispatch_int<RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(c->interrogate, [&](auto I) {
                LaunchTimer t(h, "evidence_kernel");
                hipLaunchKernelGGL((evidence_kernel<RHS, P, I>), g.grid, g.block, 0, h->stream, a, logdens, quad, logdet);
                t.stop();
                ok = true;
            });
        });
    } else {
        const LaunchGeom g = fwd_sqrt_geom(a.B, RHS::D);
        dispatch_int<2, 8>(c->n_bstate, [&](auto P) {
            dispatch_int<RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(c->interrogate, [&](auto I) {
                LaunchTimer t(h, "evidence_sqrt_kernel");
                hipLaunchKernelGGL((evidence_sqrt_kernel<RHS, P, I>), g.grid, g.block, 0, h->stream, a, logdens, quad, logdet);
                t.stop();
                ok = true;
            });
        });
    }
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "evidence: no kernel for rhs %d, n_bstate %d, interrogate %d on this route", c->rhs_id,
               c->n_bstate, c->interrogate);
    RK_HIP(hipGetLastError());
    return RK_OK;
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_solve_evidence(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, double* logdens, double* quad,
                      double* logdet) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_solve_evidence: null cfg");
    int rc = evidence_check(c);                                     // (the configuration alone, before anything else is looked at)
    if (rc) return rc;
    RK_REQUIRE(h && logdens && quad && logdet, RK_ERR_INVALID, "rk_solve_evidence: null argument");
    rc = check_cfg(c, in);
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, nullptr, a);
    const EvRoute route = c->kalman_type == RK_KALMAN_SQRT ? EvRoute::Sqrt : (evidence_tile_route(c) ? EvRoute::Tile : EvRoute::Lane);
    if (is_user_rhs(c->rhs_id)) return user_evidence(h, c, a, (int)route, logdens, quad, logdet);
    rc = RK_ERR_UNSUPPORTED;
    with_builtin_rhs(c->rhs_id, [&](auto rhs) {
        using RHS = decltype(rhs);
        rc = check_n_theta<RHS>(c, a);
        if (rc) return;
        rc = launch_evidence_rhs<RHS>(h, c, a, route, logdens, quad, logdet);
    });
    return rc;
}

}  // extern "C"
