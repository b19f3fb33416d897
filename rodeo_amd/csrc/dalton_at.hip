// dalton_at: host side of rk_dalton_loglik_at, DALTON's log-likelihood for Gaussian observations
// at arbitrary times.  What is served and which route runs is rk_dalton_layout's answer (dalton.hip), so dalton and
// dalton_at cannot disagree:
//   tiles  -- dalton_fwd_at_tile3_kernel (dalton_at_tile3_kernels.hpp): n_bstate = 3, n_bobs = 1, n_block 1..4;
//   lanes  -- dalton_fwd_at_kernel (dalton_at_kernels.hpp): everything else with n_bstate 2..6, n_bobs 1..3.
// RK_DALTON_LANES=1 forces the lane route.
#include <string>
#include "common.hpp"
#include "rhs.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "dalton_at_kernels.hpp"
#include "dalton_at_tile3_kernels.hpp"

namespace rk {

template <class RHS>
static int launch_dalton_at_tile_rhs(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o,
                                     const DaltonAt& s, double* out) {
    if constexpr (RHS::D > 4 || RHS::NDEP != 1) {
        set_error("dalton_at: rhs %d has no tile form", c->rhs_id);
        return RK_ERR_UNSUPPORTED;
    } else {
        const LaunchGeom g = dalton_tile_geom(a.B, RHS::D, true);
        bool ok = false;
        dispatch_int<RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(c->interrogate, [&](auto I) {
            LaunchTimer t(h, "dalton_fwd_at_tile3_kernel");
            hipLaunchKernelGGL((dalton_fwd_at_tile3_kernel<RHS, I>), g.grid, g.block, 0, h->stream, a, o, s, out);
            t.stop();
            ok = true;
        });
        RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "dalton_at: interrogate %d has no tile kernel", c->interrogate);
        RK_HIP(hipGetLastError());
        return RK_OK;
    }
}

template <class RHS>
static int launch_dalton_at_rhs(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, const DaltonAt& s,
                                int n_bobs, double* logdens) {
    const LaunchGeom g = dalton_lane_geom(a.B, true);
    bool ok = false;
    dispatch_int<2, dalton_pmax<RHS>()>(c->n_bstate, [&](auto P) {
        dispatch_int<RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(c->interrogate, [&](auto I) {
            dispatch_int<1, 3>(n_bobs, [&](auto M) {
                LaunchTimer t(h, "dalton_fwd_at_kernel");
                hipLaunchKernelGGL((dalton_fwd_at_kernel<RHS, P, I, M>), g.grid, g.block, 0, h->stream, a, o, s, logdens);
                t.stop();
                ok = true;
            });
        });
    });
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "dalton_at: no kernel for n_bstate %d, interrogate %d, n_bobs %d", c->n_bstate,
               c->interrogate, n_bobs);
    RK_HIP(hipGetLastError());
    return RK_OK;
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_dalton_loglik_at(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const double* obs, const double* obs_weight,
                        const double* obs_var, const rk_dalton_at_in* at, int32_t n_obs, int32_t n_bobs, double* logdens) {
    // what is not served is refused on the configuration alone, before the handle or any array is looked at
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_dalton_loglik_at (dalton_at): null cfg");
    int32_t lay = 0;
    int rc = rk_dalton_layout(c, RK_MODE_FILTER, n_bobs, &lay);           // dalton's own refusals and route
    if (rc) {
        const std::string why = rk_last_error();
        set_error("dalton_at serves what dalton serves: %s", why.c_str());
        return rc;
    }
    RK_REQUIRE(h && in && at && logdens, RK_ERR_INVALID, "rk_dalton_loglik_at (dalton_at): null argument");
    rc = check_cfg(c, in);
    if (rc) return rc;
    RK_REQUIRE(n_obs >= 1 && obs && obs_weight && obs_var && at->table, RK_ERR_INVALID,
               "dalton_at: null observation array or table, or n_obs < 1");
    RK_REQUIRE(at->n_pre >= 1 && at->n_post >= 1 && at->pre_trans && at->pre_noise && at->post_trans && at->post_noise,
               RK_ERR_INVALID, "dalton_at: n_pre and n_post must be at least 1 and the four prior arrays present, got %d, %d",
               at->n_pre, at->n_post);
    DaltonObs o;
    o.obs = obs; o.obs_w = obs_weight; o.obs_v = obs_var; o.obs_ind = nullptr; o.n_obs = n_obs;
    DaltonAt s;
    s.pre_q = at->pre_trans; s.pre_r = at->pre_noise; s.post_q = at->post_trans; s.post_r = at->post_noise;
    s.tab = at->table; s.n_pre = at->n_pre; s.n_post = at->n_post; s.prior_b = at->prior_batched ? 1 : 0;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, nullptr, a);
    const bool tile = lay == RK_LAYOUT_TILE3;
    if (tile) RK_HIP(hipMemsetAsync(logdens, 0, sizeof(double) * (size_t)c->n_traj, h->stream));   // (two atomic adds each)
    if (is_user_rhs(c->rhs_id)) return user_dalton_at(h, c, a, o, s, n_bobs, tile, logdens);
    rc = RK_ERR_UNSUPPORTED;
    with_builtin_rhs(c->rhs_id, [&](auto rhs) {
        using RHS = decltype(rhs);
        rc = check_n_theta<RHS>(c, a);
        if (rc) return;
        if (tile) {
            rc = launch_dalton_at_tile_rhs<RHS>(h, c, a, o, s, logdens);
        } else {
            rc = launch_dalton_at_rhs<RHS>(h, c, a, o, s, n_bobs, logdens);
        }
    });
    return rc;
}

}  // extern "C"
