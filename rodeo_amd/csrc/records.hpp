// Record access of the lane-per-(block, trajectory) kernels ("Batch-minor records").  An ITEM is `width` doubles of
// one (time or record index n, block, trajectory); element e of it lies at  base + ((n D + blk) width + e) B + b,  so that the
// 64 lanes of a wave (consecutive b) read one 512 B row per element.  The filtered / smoothed moments of a solver call are two
// such items, `mean` (width P) and `var` (width P^2): load_moments / store_moments; load_moments also reads them from the
// tile records, whichever layout rk_solve_layout reported.  The field offsets of a workspace record are named once, in a struct
// next to the text that defines the record (FenrirItem, SqrtGainRec, ..), which writer, reader and the host's sizing use.
// Ahead-of-time code only: not part of the hiprtc program text (embed_sources.py), whose kernels walk all blocks of a lane
// with a running index.
#pragma once
#include <stddef.h>
#include "../../include/rodeo_kalman.h"

namespace rk {

// ---- batch-minor items -----------------------------------------------------------------------------------------------
// element 0 of the `width`-double item of (n, blk, b); element e is item[(size_t)e * B]
__device__ __forceinline__ const double* bm_item(const double* base, size_t width, size_t B, int D, int n, int blk, int b) {
    return base + ((size_t)n * D + blk) * width * B + b;
}
__device__ __forceinline__ double* bm_item(double* base, size_t width, size_t B, int D, int n, int blk, int b) {
    return base + ((size_t)n * D + blk) * width * B + b;
}

// ---- the moments of one solver call ----------------------------------------------------------------------------------
// Lanes run fastest over what is contiguous in the records: (trajectory, block) for the tile records (time, B, D, record),
// the trajectory for the batch-minor columns.
template <int LAYOUT>
__device__ __forceinline__ void record_lane(int l, int B, int D, int& blk, int& b) {
    if constexpr (LAYOUT == RK_LAYOUT_BATCH_MINOR) {
        blk = l / B;
        b = l - blk * B;
    } else {
        b = l / D;
        blk = l - b * D;
    }
}

// (mean, var) of time n from the records of one solver call, in the four layouts of rk_solve_layout: RK_LAYOUT_TILE3 rows
// [Sigma[i][0..2] | mu[i]], RK_LAYOUT_TILE4 / RK_LAYOUT_TILEP [Sigma row-major | mu] (solve_tilen_kernels.hpp; `mean` is not
// read), batch-minor (N+1, D, P[, P], B).
template <int P, int LAYOUT>
__device__ __forceinline__ void load_moments(const double* mean, const double* var, size_t B, int D, int n, int blk, int b,
                                             double (&m)[P], double (&S)[P][P]) {
    if constexpr (LAYOUT == RK_LAYOUT_BATCH_MINOR) {
        const double* mi = bm_item(mean, P, B, D, n, blk, b);
        const double* vi = bm_item(var, P * P, B, D, n, blk, b);
#pragma unroll
        for (int i = 0; i < P; ++i) {
            m[i] = mi[(size_t)i * B];
#pragma unroll
            for (int j = 0; j < P; ++j) S[i][j] = vi[((size_t)i * P + j) * B];
        }
    } else if constexpr (LAYOUT == RK_LAYOUT_TILE3) {
        static_assert(P == 3, "RK_LAYOUT_TILE3 is the n_bstate = 3 record");
        const double* rec = (const double*)__builtin_assume_aligned(var + ((size_t)n * B * D + (size_t)b * D + blk) * 12, 32);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) S[i][j] = rec[4 * i + j];
            m[i] = rec[4 * i + 3];
        }
    } else {
        const double* rec =
            (const double*)__builtin_assume_aligned(var + ((size_t)n * B * D + (size_t)b * D + blk) * (P * P + P), 16);
#pragma unroll
        for (int i = 0; i < P; ++i) {
            m[i] = rec[P * P + i];
#pragma unroll
            for (int j = 0; j < P; ++j) S[i][j] = rec[i * P + j];
        }
    }
}

// the batch-minor counterpart: (m, S) to time n of mean (N+1, D, P, B) / var (N+1, D, P, P, B)
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

}  // namespace rk
