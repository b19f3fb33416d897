// The solver's posterior at arbitrary times: launch side of rk_eval_at (the entry point and its refusals are in api.hip).
// eval_at_kernel<P, LAYOUT> (eval_at_kernels.hpp) reads the records of one rk_solve_filter and one rk_solve_mv call of the
// same configuration, in whichever layout rk_solve_layout gave both, and writes T records per trajectory.
#include "common.hpp"
#include "solve_paths.hpp"
#include "eval_at_kernels.hpp"

namespace rk {

template <int P, int LAYOUT, int SLAYOUT = LAYOUT>
static void eval_at_go(rk_handle h, const EvalAtArgs& a, dim3 grid) {
    LaunchTimer t(h, "eval_at_kernel");
    hipLaunchKernelGGL((eval_at_kernel<P, LAYOUT, SLAYOUT>), grid, dim3(64), 0, h->stream, a);
    t.stop();
}

int eval_at_launch(rk_handle h, const rk_solve_cfg* c, int layout, const rk_solve_out* filt, const rk_solve_out* smooth,
                   const rk_eval_at_in* q, double* mean_out, double* var_out) {
    EvalAtArgs a;
    a.B = c->n_traj; a.N = c->n_steps; a.D = c->n_block; a.T = q->n_query; a.n_quad = q->n_quad;
    a.fmean = filt->mean_state; a.fvar = filt->var_state;
    a.smean = smooth->mean_state; a.svar = smooth->var_state;
    a.query = q->query;
    a.trans = q->trans; a.noise = q->noise;
    a.trans_b = q->trans_batched != 0; a.noise_b = q->noise_batched != 0;
    a.mean_out = mean_out; a.var_out = var_out;
    const int brc = begin_solve(h);
    if (brc) return brc;
    const dim3 grid((unsigned)((int64_t)div_up(a.B * a.D, 64) * a.T));
    bool ok = false;
    switch (layout) {
        case RK_LAYOUT_TILE3:
            eval_at_go<3, RK_LAYOUT_TILE3>(h, a, grid);
            ok = true;
            break;
        case RK_LAYOUT_TILE3_PACKED:           // the smoother's records; the filter's are natural
            eval_at_go<3, RK_LAYOUT_TILE3, RK_LAYOUT_TILE3_PACKED>(h, a, grid);
            ok = true;
            break;
        case RK_LAYOUT_TILE4:
            eval_at_go<4, RK_LAYOUT_TILE4>(h, a, grid);
            ok = true;
            break;
        case RK_LAYOUT_TILEP:
            ok = dispatch_int<5, EVAL_AT_PMAX>(c->n_bstate, [&](auto P) { eval_at_go<P, RK_LAYOUT_TILEP>(h, a, grid); });
            break;
        case RK_LAYOUT_BATCH_MINOR:
            ok = dispatch_int<EVAL_AT_PMIN, EVAL_AT_PMAX>(c->n_bstate,
                                                          [&](auto P) { eval_at_go<P, RK_LAYOUT_BATCH_MINOR>(h, a, grid); });
            break;
    }
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "eval_at: no kernel for n_bstate %d in layout %d", c->n_bstate, layout);
    RK_HIP(hipGetLastError());
    return RK_OK;
}

}  // namespace rk
