// Host side of the Laplace driver's device pieces (laplace_kernels.hpp): rk_fd_stencil, rk_fd_grad_hess, rk_newton_step, and
// for the gradient mode rk_fd_grad_stencil, rk_fd_hess_from_grad.
// Every array is a device pointer, row-major with the centre axis first (the driver downloads the stencil as the
// (C S, k) batch of its user's log-posterior).  Nothing is allocated here; every launch goes to the handle's stream.
#include "common.hpp"
#include "solve_paths.hpp"
#include "laplace_kernels.hpp"

namespace rk {

static int laplace_check(const char* who, int C, int k) {
    RK_REQUIRE(C >= 1 && k >= 1, RK_ERR_INVALID, "%s: n_centre >= 1 and k >= 1, got %d, %d", who, C, k);
    RK_REQUIRE(k <= LAPLACE_KMAX, RK_ERR_UNSUPPORTED, "%s: k <= %d (the Newton step keeps the factor in registers), got %d",
               who, LAPLACE_KMAX, k);
    RK_REQUIRE((int64_t)C * (2 * k * k + 1) * k <= 0x7fffffff, RK_ERR_INVALID, "%s: n_centre %d does not fit a grid", who, C);
    return RK_OK;
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_fd_stencil(rk_handle h, int32_t n_centre, int32_t k, const double* u, const double* step, double* out) {
    RK_REQUIRE(h && u && step && out, RK_ERR_INVALID, "rk_fd_stencil: null argument");
    const int rc = laplace_check("rk_fd_stencil", n_centre, k);
    if (rc) return rc;
    const int brc = begin_solve(h);
    if (brc) return brc;
    const int64_t n = (int64_t)n_centre * (2 * k * k + 1) * k;
    LaunchTimer t(h, "fd_stencil_kernel");
    hipLaunchKernelGGL(fd_stencil_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, u, step, n_centre, k, out);
    t.stop();
    RK_HIP(hipGetLastError());
    return RK_OK;
}

int rk_fd_grad_hess(rk_handle h, int32_t n_centre, int32_t k, const double* vals, const double* step, double* grad,
                    double* hess, int32_t* n_bad) {
    RK_REQUIRE(h && vals && step && grad && hess && n_bad, RK_ERR_INVALID, "rk_fd_grad_hess: null argument");
    const int rc = laplace_check("rk_fd_grad_hess", n_centre, k);
    if (rc) return rc;
    const int brc = begin_solve(h);
    if (brc) return brc;
    LaunchTimer t(h, "fd_grad_hess_kernel");
    hipLaunchKernelGGL(fd_grad_hess_kernel, dim3(n_centre), dim3(256), 0, h->stream, vals, step, k, grad, hess, n_bad);
    t.stop();
    RK_HIP(hipGetLastError());
    return RK_OK;
}

int rk_newton_step(rk_handle h, int32_t n_centre, int32_t k, const double* grad, const double* hess, const double* damping,
                   double* delta, double* logdet, int32_t* ok) {
    RK_REQUIRE(h && grad && hess && damping && delta && logdet && ok, RK_ERR_INVALID, "rk_newton_step: null argument");
    const int rc = laplace_check("rk_newton_step", n_centre, k);
    if (rc) return rc;
    const int brc = begin_solve(h);
    if (brc) return brc;
    const bool served = dispatch_int<1, LAPLACE_KMAX>(k, [&](auto K) {
        LaunchTimer t(h, "newton_step_kernel");
        hipLaunchKernelGGL((newton_step_kernel<decltype(K)::value>), dim3(div_up(n_centre, 64)), dim3(64), 0, h->stream, grad,
                           hess, damping, n_centre, delta, logdet, ok);
        t.stop();
    });
    RK_REQUIRE(served, RK_ERR_UNSUPPORTED, "rk_newton_step: no kernel for k = %d", k);
    RK_HIP(hipGetLastError());
    return RK_OK;
}

int rk_fd_grad_stencil(rk_handle h, int32_t n_centre, int32_t k, const double* u, const double* step, double* out) {
    RK_REQUIRE(h && u && step && out, RK_ERR_INVALID, "rk_fd_grad_stencil: null argument");
    const int rc = laplace_check("rk_fd_grad_stencil", n_centre, k);
    if (rc) return rc;
    const int brc = begin_solve(h);
    if (brc) return brc;
    const int64_t n = (int64_t)n_centre * (2 * k + 1) * k;           // (below laplace_check's bound on C (2 k^2 + 1) k)
    LaunchTimer t(h, "fd_grad_stencil_kernel");
    hipLaunchKernelGGL(fd_grad_stencil_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, u, step, n_centre, k,
                       out);
    t.stop();
    RK_HIP(hipGetLastError());
    return RK_OK;
}

int rk_fd_hess_from_grad(rk_handle h, int32_t n_centre, int32_t k, const double* vals, const double* grads,
                         const double* step, double* grad, double* hess, double* grad_fd, int32_t* n_bad) {
    RK_REQUIRE(h && vals && grads && step && grad && hess && grad_fd && n_bad, RK_ERR_INVALID,
               "rk_fd_hess_from_grad: null argument");
    const int rc = laplace_check("rk_fd_hess_from_grad", n_centre, k);
    if (rc) return rc;
    const int brc = begin_solve(h);
    if (brc) return brc;
    LaunchTimer t(h, "fd_hess_from_grad_kernel");
    hipLaunchKernelGGL(fd_hess_from_grad_kernel, dim3(n_centre), dim3(256), 0, h->stream, vals, grads, step, k, grad, hess,
                       grad_fd, n_bad);
    t.stop();
    RK_HIP(hipGetLastError());
    return RK_OK;
}

}  // extern "C"
