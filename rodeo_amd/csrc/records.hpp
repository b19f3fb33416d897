// Record access of the lane-per-(block, trajectory) kernels ("Batch-minor records").  An ITEM is `width` doubles of
// one (time or record index n, block, trajectory); element e of it lies at  base + ((n D + blk) width + e) B + b,  so that the
// 64 lanes of a wave (consecutive b) read one 512 B row per element.  The filtered / smoothed moments of a solver call are two
// such items, `mean` (width P) and `var` (width P^2).  bm_item, load_moments_bm and store_moments live in lane_filter.hpp,
// which the hiprtc program text shares; this header adds load_moments, which reads the moments in whichever layout
// rk_solve_layout reported, the tile records included, and is ahead-of-time code only (it needs the C header's layout names).
// The field offsets of a workspace record are named once, in a struct next to the text that defines the record (FenrirItem,
// SqrtGainRec, ..), which writer, reader and the host's sizing use.
#pragma once
#include <stddef.h>
#include "../../include/rodeo_kalman.h"
#include "lane_filter.hpp"
#include "tile3_pack.hpp"

namespace rk {

// ---- the moments of one solver call ----------------------------------------------------------------------------------
// Lanes run fastest over what is contiguous in the records: (trajectory, block) for the tile records (time, B, D, record),
// the trajectory for the batch-minor columns.
template <int LAYOUT>
__device__ __forceinline__ void record_lane(int l, int B, int D, int& blk, int& b) {
    static_assert(LAYOUT != RK_LAYOUT_TILE3_PACKED, "lanes over packed records run as over RK_LAYOUT_TILE3");
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
// read), batch-minor (N+1, D, P[, P], B).  RK_LAYOUT_TILE3_PACKED (smoothed records of rk_solve_mv): the record of (n, tile) is
// the packed one where tile3_pack_record says so -- `N` = n_steps is read for that alone -- and the natural tile elsewhere.
// SYM: Sigma's lower triangle is taken from the upper one, which is what a packed record holds; readers of SMOOTHED p = 3
// records ask for it in the natural layout too, so that both layouts give the same bits.
template <int P, int LAYOUT, bool SYM = false>
__device__ __forceinline__ void load_moments(const double* mean, const double* var, size_t B, int D, int n, int blk, int b,
                                             double (&m)[P], double (&S)[P][P], int N = 0) {
    if constexpr (LAYOUT == RK_LAYOUT_BATCH_MINOR) {
        load_moments_bm<P>(mean, var, B, D, n, blk, b, m, S);
    } else if constexpr (LAYOUT == RK_LAYOUT_TILE3 || LAYOUT == RK_LAYOUT_TILE3_PACKED) {
        static_assert(P == 3, "RK_LAYOUT_TILE3 is the n_bstate = 3 record");
        const long long n_tiles = (long long)B * D, tau = (long long)b * D + blk;
        if (LAYOUT == RK_LAYOUT_TILE3_PACKED && tile3_pack_record(N, n_tiles, n, tau)) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = i; j < 3; ++j) S[i][j] = S[j][i] = var[tile3_pack_index(n_tiles, n, tau, tile3_pack_slot(i, j))];
                m[i] = var[tile3_pack_index(n_tiles, n, tau, tile3_pack_slot(i, 3))];
            }
            return;
        }
        const double* rec = (const double*)__builtin_assume_aligned(var + ((size_t)n * B * D + (size_t)b * D + blk) * 12, 32);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) S[i][j] = rec[SYM && j < i ? 4 * j + i : 4 * i + j];
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

}  // namespace rk
