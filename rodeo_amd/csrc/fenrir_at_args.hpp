// fenrir_at: the arguments its three kernels share -- fenrir_at_hops_kernel and fenrir_bwd_at_kernel
// (fenrir_at_kernels.hpp) and fenrir_bwd_at_tile3_kernel (solve_tile3.hip: fenrir_tile3_body<true>, the body it shares with
// fenrir_bwd_tile3_kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rk {

// Observations, table and sub-step priors of rk_fenrir_backward_at (the table and the pre / post pairs of rk_dalton_at_in),
// and the hop records in the caller's workspace.  tab (n_obs, 4): node, off-grid flag, pre slot, post slot of the interval's
// last observation or -1.  An interval with the off-grid observations 1 .. k has k + 1 hops: hop j < k is the map over the gap
// in front of observation j + 1 and has record `pre slot of observation j + 1`; hop k, from the last observation to the right
// node, has record n_pre + post slot.  A record holds the forward moments s_j, e_j at the hop's two ends and the gain G_j:
//   tiles: three augmented 4 x 4 tiles [M- | G~^T | M_f] = [e_j | diag(G_j, 1)^T | s_j] of 16 doubles, row-major, per
//          (record, trajectory, block) -- the hand-off item of tile3_gain_producers without its LDS swizzle;
//   lanes: [mu(s) (P), Sigma(s) (P^2), mu(e) (P), Sigma(e) (P^2), G (P^2)] per (record, block), batch-minor.
struct FenrirAt {
    const double *obs, *obs_w, *obs_v;
    const int32_t* tab;
    int n_obs, n_pre, n_post, prior_b;
    const double *pre_q, *pre_r, *post_q, *post_r;
    double* hops;
    double* logdens;                        // (B,), zeroed by the caller
};

constexpr int FENRIR_AT_TILE_REC = 48;      // doubles per (record, tile) on the tile route
// the lane record [mu(s), Sigma(s) | mu(e), Sigma(e) | G] of n_bstate = p: element offsets of its fields and its doubles per
// (record, block, trajectory)
struct FenrirAtLaneRec {
    int s, e, G, width;
    constexpr explicit FenrirAtLaneRec(int p) : s(0), e(p + p * p), G(2 * (p + p * p)), width(3 * p * p + 2 * p) {}
};

__device__ __forceinline__ int fenrir_at_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

}  // namespace rk
