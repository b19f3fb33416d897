// daltonng_grid / solve_mv_nn_grid (an addition): host side of rk_daltonng_grid_loglik /
// rk_daltonng_grid_solve, DALTON for non-Gaussian observations on rk_solve_grid's non-uniform grid, every observation on a node.
// The forward filter is a hiprtc build around the user's log-likelihood (rhs_jit.hip: ng_grid_forward,
// daltonng_grid_kernels.hpp); the gain kernel of the two backward log-density passes is built here, with every step's own prior
// pair; the chain and observation kernels are rk_daltonng_loglik's own, which read records and never the prior, and
// rk_daltonng_grid_solve ends in rk_solve_grid's smoothing pass.  The workspace is rk_daltonng_workspace_bytes's.
// The pieces of the configuration check ahead of ng_check, the grid's staging and the test of the output pointers are
// grid_entry.hpp's.
#include "common.hpp"
#include "rhs.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "grid_entry.hpp"
#include "grid_kernels.hpp"
#include "daltonng_kernels.hpp"

namespace rk {

// daltonng_gain_kernel (daltonng_kernels.hpp) with the item's pair from the grid: one lane per (step n = 1 .. N-1, block,
// trajectory), record (n - 1, blk) in that kernel's layout, pred[n+1] re-evaluated from filt[n] with (q, r)[slot[n]] -- Q_n in
// the gain G = Sigma_f Q_n^T (Sigma-)^{-1}, R_n in Sigma- -- which is what the forward filter predicted with.
template <int P>
__global__ void __launch_bounds__(64) daltonng_grid_gain_kernel(SolveArgs a, NgWs w, GridArgs g) {
    constexpr int E = ng_rec_doubles(P);
    const size_t B = (size_t)a.B;
    const size_t l = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (l >= (size_t)(a.N - 1) * a.D * B) return;
    const int b = (int)(l % B), blk = (int)((l / B) % a.D), r = (int)(l / (B * a.D));
    double Q[P][P], R[P][P];
    grid_load_pair<P>(g, a.B, a.D, grid_slot(g, r + 1), blk, b, Q, R);      // (r + 1 <= N - 1: inside the slot table)
    double* rec = bm_item(w.rec, E, B, a.D, r, blk, b);
#pragma unroll
    for (int z = 0; z < 2; ++z) {
        double mf[P], Sf[P][P], mp[P], Sp[P][P], T[P][P], G[P][P], GT[P][P], A[P][P];
        load_moments_bm<P>(z ? w.zm : w.jm, z ? w.zv : w.jv, B, a.D, r + 1, blk, b, mf, Sf);
        predict_block<P>(Q, R, mf, Sf, mp, Sp);                             // pred[n+1] re-evaluated from filt[n]
        smooth_gain<P>(Q, Sf, Sp, T, G);
        mm_nt<P, P, P>(G, T, GT);
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int j = 0; j < P; ++j) GT[i][j] = Sf[i][j] - GT[i][j];     // var_sim (standard.py:254)
        const double c = z ? ng_masked<P, true>(GT, A) : ng_masked<P, false>(GT, A);
        double* o = rec + (size_t)(z ? P * P + P + 1 : 0) * B;
#pragma unroll
        for (int i = 0; i < P; ++i) {
#pragma unroll
            for (int j = 0; j < P; ++j) o[(size_t)(i * P + j) * B] = G[i][j];
            o[(size_t)(P * P + i) * B] = mp[i];
        }
        if (z) {
#pragma unroll
            for (int i = 0; i < P; ++i)
#pragma unroll
                for (int j = 0; j < P; ++j) o[(size_t)(P * P + P + i * P + j) * B] = A[i][j];
            o[(size_t)(2 * P * P + P) * B] = c;
        } else {
            o[(size_t)(P * P + P) * B] = c;
        }
    }
}

// Is this call served?  Decided on the configuration, the mode and the registered model alone: RK_OK, RK_ERR_INVALID or
// RK_ERR_UNSUPPORTED.  dalton_grid_check's pattern (dalton_grid.hip; the pieces are grid_entry.hpp's) joined with rk_daltonng_*'s
// limits (ng_check).
// mode < 0: the log-likelihood, which has none.
static int ng_grid_check(const rk_solve_cfg* c, int mode, int obs_id) {
    const char* who = "daltonng_grid";
    int rc = grid_sizes_check(who, c);
    if (rc) return rc;
    RK_REQUIRE(mode < 0 || mode == RK_MODE_FILTER || mode == RK_MODE_MV, RK_ERR_INVALID,
               "%s: mode must be RK_MODE_FILTER or RK_MODE_MV (the uniform-grid form has no sampler either), got %d", who, mode);
    rc = grid_flags_check(who, GRID_RECORDS, c);
    if (rc) return rc;
    return ng_check(who, c, obs_id);
}

// the pointers of a served call: the grid (rk_solve_grid's rule), the solver inputs and the observations
static int ng_grid_inputs(const char* who, const rk_solve_cfg* c, const rk_solve_in* in, const double* obs, const int32_t* obs_node,
                          int n_obs, const rk_grid_in* g, NgObs& o, GridArgs& ga) {
    int rc = grid_args(who, g, ga);
    if (rc) return rc;
    rc = check_cfg(c, in);
    if (rc) return rc;
    RK_REQUIRE(n_obs >= 0 && (n_obs == 0 || (obs && obs_node)), RK_ERR_INVALID, "%s: null observation array or n_obs < 0", who);
    o.y = obs; o.obs_ind = obs_node; o.n_obs = n_obs;
    return RK_OK;
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_daltonng_grid_loglik(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, int32_t obs_id, const double* obs,
                            const int32_t* obs_node, int32_t n_obs, const rk_grid_in* g, void* workspace, size_t workspace_bytes,
                            double* logdens) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_daltonng_grid_loglik: null cfg");
    int rc = ng_grid_check(c, -1, obs_id);                          // (the configuration alone, before anything else is looked at)
    if (rc) return rc;
    RK_REQUIRE(h && g && logdens, RK_ERR_INVALID, "rk_daltonng_grid_loglik: null argument");
    NgObs o;
    GridArgs ga;
    rc = ng_grid_inputs("rk_daltonng_grid_loglik", c, in, obs, obs_node, n_obs, g, o, ga);
    if (rc) return rc;
    NgWs w;
    rc = ng_workspace("rk_daltonng_grid_loglik", c, n_obs, workspace, workspace_bytes, w);      // (before any launch)
    if (rc) return rc;
    const size_t items = (size_t)(c->n_steps - 1) * c->n_block * c->n_traj;
    RK_REQUIRE(items / 64 < 0x7fffffffu, RK_ERR_UNSUPPORTED,
               "daltonng_grid: too many (step, block, trajectory) items for one launch");
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, nullptr, a);
    a.mean = w.jm; a.var = w.jv; a.mean_pred = a.var_pred = a.x = nullptr;
    rc = ng_grid_forward(h, c, obs_id, a, o, ga, true, w.zm, w.zv);
    if (rc) return rc;
    if (items) {
        LaunchTimer t(h, "daltonng_grid_gain_kernel");
        const bool ok = dispatch_int<2, 6>(c->n_bstate, [&](auto P) {
            hipLaunchKernelGGL((daltonng_grid_gain_kernel<P>), dim3((unsigned)((items + 63) / 64)), dim3(64), 0, h->stream, a, w, ga);
        });
        t.stop();
        RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "daltonng_grid: no gain kernel for n_bstate %d", c->n_bstate);
    }
    rc = ng_chain(h, c, a, w, o);
    if (rc) return rc;
    RK_HIP(hipGetLastError());
    return ng_obs_eval(h, c, obs_id, a, o, w.sm, w.part, logdens);
}

int rk_daltonng_grid_solve(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, int32_t mode,
                           int32_t obs_id, const double* obs, const int32_t* obs_node, int32_t n_obs, const rk_grid_in* g) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_daltonng_grid_solve: null cfg");
    RK_REQUIRE(mode >= 0, RK_ERR_INVALID, "daltonng_grid: mode must be RK_MODE_FILTER or RK_MODE_MV, got %d", mode);
    int rc = ng_grid_check(c, mode, obs_id);
    if (rc) return rc;
    RK_REQUIRE(h && out && g, RK_ERR_INVALID, "rk_daltonng_grid_solve: null argument");
    NgObs o;
    GridArgs ga;
    rc = ng_grid_inputs("rk_daltonng_grid_solve", c, in, obs, obs_node, n_obs, g, o, ga);
    if (rc) return rc;
    rc = grid_out_check("rk_daltonng_grid_solve", out, mode);        // (FILTER or MV: no sampler)
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, out, a);
    a.mean_pred = a.var_pred = nullptr;
    rc = ng_grid_forward(h, c, obs_id, a, o, ga, false, nullptr, nullptr);
    if (rc || mode == RK_MODE_FILTER) return rc;
    return launch_grid_bwd(h, c, a, mode, ga);
}

}  // extern "C"
