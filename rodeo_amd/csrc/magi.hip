// MAGI log-density (src/rodeo/inference/magi.py:6-99): host side of rk_magi_logdens.  magi_kernel<P, NA, SQRT>
// (magi_kernels.hpp) runs one lane per (trajectory, block) and writes the block sums; with more than one block they go to
// the handle's grow-only scratch and magi_sum_kernel adds them in block order.  The caller supplies the data (x0 and the
// measured components of x_{1:N}); nothing else is read.
#include "common.hpp"
#include "solve_paths.hpp"
#include "magi_kernels.hpp"

namespace rk {

// Largest n_bstate served.  Beyond it the kernels spill to scratch: the standard predict holds Q, R, Sigma and Q Sigma at
// once (256 doubles at P = 7 with the rest of the step); the square-root form keeps its factors triangular and goes one
// further (at P = 8 one instance of eight, n_active = 5, spilled: the served range is kept contiguous).
constexpr int MAGI_PMAX_STD = 6, MAGI_PMAX_SQRT = 7;
static int magi_pmax(bool sqrt_form) { return sqrt_form ? MAGI_PMAX_SQRT : MAGI_PMAX_STD; }

static int magi_check(const rk_magi_cfg* c, const rk_magi_in* in) {
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD || c->kalman_type == RK_KALMAN_SQRT, RK_ERR_UNSUPPORTED,
               "magi: unknown kalman_type %d", c->kalman_type);
    RK_REQUIRE(c->n_traj >= 1 && c->n_steps >= 0 && c->n_block >= 1, RK_ERR_INVALID,
               "magi: n_traj >= 1, n_steps >= 0 and n_block >= 1, got %d, %d, %d", c->n_traj, c->n_steps, c->n_block);
    const int pmax = magi_pmax(c->kalman_type == RK_KALMAN_SQRT);
    RK_REQUIRE(c->n_bstate >= 2 && c->n_bstate <= pmax, RK_ERR_UNSUPPORTED,
               "magi: n_bstate in 2..%d for this kalman_type (beyond, the lane kernel spills), got %d", pmax, c->n_bstate);
    RK_REQUIRE(c->n_active >= 1 && c->n_active <= c->n_bstate, RK_ERR_INVALID, "magi: n_active in 1..%d, got %d",
               c->n_bstate, c->n_active);
    RK_REQUIRE((int64_t)div_up(c->n_traj, 64) * c->n_block <= 0x7fffffff, RK_ERR_INVALID,
               "magi: ceil(n_traj / 64) * n_block must fit a grid (%d, %d)", c->n_traj, c->n_block);
    RK_REQUIRE(in->x0 && in->prior_weight && in->prior_var && (c->n_steps == 0 || in->x_meas), RK_ERR_INVALID,
               "magi: null input array");
    return RK_OK;
}

// The handle's grow-only device scratch (shared with the large-block operators, solve_dense_ops.hpp), at least `need` bytes.
// (also where rk_fenrir_grid_loglik keeps its block sums, fenrir_grid.hip: declared in solve_paths.hpp)
int lane_scratch(rk_handle h, size_t need, double** p) {
    if (h->op_scratch_bytes < need) {
        if (h->op_scratch) {
            RK_HIP(hipStreamSynchronize(h->stream));
            RK_HIP(hipFree(h->op_scratch));
            h->op_scratch = nullptr;
            h->op_scratch_bytes = 0;
        }
        RK_HIP(hipMalloc(&h->op_scratch, need));
        h->op_scratch_bytes = need;
    }
    *p = (double*)h->op_scratch;
    return RK_OK;
}

// logdens[b] = the D block sums part[blk * B + b] of trajectory b, added in block order (magi_sum_kernel; declared in
// solve_paths.hpp like lane_scratch)
int launch_block_sum(rk_handle h, const double* part, int B, int D, double* logdens) {
    LaunchTimer t(h, "magi_sum_kernel");
    hipLaunchKernelGGL(magi_sum_kernel, dim3(div_up(B, 256)), dim3(256), 0, h->stream, part, B, D, logdens);
    t.stop();
    RK_HIP(hipGetLastError());
    return RK_OK;
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_magi_logdens(rk_handle h, const rk_magi_cfg* c, const rk_magi_in* in, double* logdens) {
    RK_REQUIRE(h && c && in && logdens, RK_ERR_INVALID, "rk_magi_logdens: null argument");
    const int rc = magi_check(c, in);
    if (rc) return rc;
    MagiArgs a;
    a.B = c->n_traj; a.N = c->n_steps; a.D = c->n_block;
    a.x0 = in->x0; a.xm = in->x_meas; a.Q = in->prior_weight; a.R = in->prior_var;
    a.x0_b = in->x0_batched != 0; a.xm_b = in->x_meas_batched != 0;
    a.Q_b = in->prior_weight_batched != 0; a.R_b = in->prior_var_batched != 0;
    const int brc = begin_solve(h);
    if (brc) return brc;
    double* part = logdens;
    if (a.D > 1) {
        const int src = lane_scratch(h, sizeof(double) * (size_t)a.B * (size_t)a.D, &part);
        if (src) return src;
    }
    const dim3 grid(div_up(a.B, 64) * a.D), block(64);
    const bool sq = c->kalman_type == RK_KALMAN_SQRT;
    bool ok = false;
    if (sq) {
        dispatch_int<2, MAGI_PMAX_SQRT>(c->n_bstate, [&](auto P) {
            dispatch_int<1, decltype(P)::value>(c->n_active, [&](auto NA) {
                LaunchTimer t(h, "magi_kernel<sqrt>");
                hipLaunchKernelGGL((magi_kernel<P, NA, true>), grid, block, 0, h->stream, a, part);
                t.stop();
                ok = true;
            });
        });
    } else {
        dispatch_int<2, MAGI_PMAX_STD>(c->n_bstate, [&](auto P) {
            dispatch_int<1, decltype(P)::value>(c->n_active, [&](auto NA) {
                LaunchTimer t(h, "magi_kernel<standard>");
                hipLaunchKernelGGL((magi_kernel<P, NA, false>), grid, block, 0, h->stream, a, part);
                t.stop();
                ok = true;
            });
        });
    }
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "magi: no kernel for n_bstate %d, n_active %d", c->n_bstate, c->n_active);
    RK_HIP(hipGetLastError());
    if (a.D > 1) return launch_block_sum(h, part, a.B, a.D, logdens);
    return RK_OK;
}

}  // extern "C"
