// What the lane-per-trajectory forward filters share besides the Kalman maps (kalman_small.hpp): the model constants and the
// initial state of a lane, the grid time of a step, and the batch-minor records ("Batch-minor records") that they
// write and the lane-per-(block, trajectory) kernels read.  For the ahead-of-time build and the hiprtc program text alike
// (embed_sources.py).  RTC-safe: no host code, no <hip/hip_runtime.h> under __HIPCC_RTC__.
#pragma once
#include "solve_args.hpp"

namespace rk {

// t_{n+1} of the solver grid (solve.py:74)
__device__ __forceinline__ double step_time(const SolveArgs& a, int n) {
    return a.t_min + (a.t_max - a.t_min) * (double)(n + 1) / (double)a.N;
}

// Q, R and W of every block and theta of trajectory b
template <class RHS, int P>
__device__ __forceinline__ void lane_load_model(const SolveArgs& a, int b, double (&Q)[RHS::D][P][P], double (&R)[RHS::D][P][P],
                                                double (&W)[RHS::D][P], double (&th)[RHS::NTHETA]) {
#pragma unroll
    for (int blk = 0; blk < RHS::D; ++blk) {
        load_block_consts<P>(a, blk, b, Q[blk], R[blk]);
#pragma unroll
        for (int j = 0; j < P; ++j) W[blk][j] = ld(a.W, (size_t)blk * P + j, a.W_b, a.B, b);
    }
#pragma unroll
    for (int k = 0; k < RHS::NTHETA; ++k) th[k] = a.theta ? ld(a.theta, k, a.theta_b, a.B, b) : 0.0;
}

// time index 0: (ode_init, 0) (solve.py:114-121)
template <int D, int P>
__device__ __forceinline__ void lane_load_init(const SolveArgs& a, int b, double (&mu)[D][P], double (&S)[D][P][P]) {
#pragma unroll
    for (int blk = 0; blk < D; ++blk)
#pragma unroll
        for (int i = 0; i < P; ++i) {
            mu[blk][i] = ld(a.x0, (size_t)blk * P + i, a.x0_b, a.B, b);
#pragma unroll
            for (int j = 0; j < P; ++j) S[blk][i][j] = 0.0;
        }
}

// ---- batch-minor items -----------------------------------------------------------------------------------------------
// element 0 of the `width`-double item of (n, blk, b); element e is item[(size_t)e * B]
__device__ __forceinline__ const double* bm_item(const double* base, size_t width, size_t B, int D, int n, int blk, int b) {
    return base + ((size_t)n * D + blk) * width * B + b;
}
__device__ __forceinline__ double* bm_item(double* base, size_t width, size_t B, int D, int n, int blk, int b) {
    return base + ((size_t)n * D + blk) * width * B + b;
}

// (mean, var) of (time n, block blk, trajectory b) from mean (N+1, D, P, B) / var (N+1, D, P, P, B)
template <int P>
__device__ __forceinline__ void load_moments_bm(const double* mean, const double* var, size_t B, int D, int n, int blk, int b,
                                                double (&m)[P], double (&S)[P][P]) {
    const double* mi = bm_item(mean, P, B, D, n, blk, b);
    const double* vi = bm_item(var, P * P, B, D, n, blk, b);
#pragma unroll
    for (int i = 0; i < P; ++i) {
        m[i] = mi[(size_t)i * B];
#pragma unroll
        for (int j = 0; j < P; ++j) S[i][j] = vi[((size_t)i * P + j) * B];
    }
}

// its counterpart: (m, S) to time n of mean / var
template <int P>
__device__ __forceinline__ void store_moments(double* mean, double* var, size_t B, int D, int n, int blk, int b,
                                              const double (&m)[P], const double (&S)[P][P]) {
    double* mo = bm_item(mean, P, B, D, n, blk, b);
    double* vo = bm_item(var, P * P, B, D, n, blk, b);
#pragma unroll
    for (int i = 0; i < P; ++i) {
        mo[(size_t)i * B] = m[i];
#pragma unroll
        for (int j = 0; j < P; ++j) vo[((size_t)i * P + j) * B] = S[i][j];
    }
}

// all blocks of a lane
template <int D, int P>
__device__ __forceinline__ void store_moments_all(double* mean, double* var, size_t B, int n, int b, const double (&m)[D][P],
                                                  const double (&S)[D][P][P]) {
#pragma unroll
    for (int blk = 0; blk < D; ++blk) store_moments<P>(mean, var, B, D, n, blk, b, m[blk], S[blk]);
}

}  // namespace rk
