// solve_mv_grid / solve_sim_grid: the solver on a non-uniform grid shared by the batch (an addition),
// the forward lane kernel and the per-step prior that the backward kernels of grid.hip read too.  Shared by the ahead-of-time
// build (grid.hip, built-in right-hand sides) and the hiprtc build for user-supplied right-hand sides (rhs_jit.hip, its grid
// kind only).  RTC-safe: no host code.
//
// Step n -> n + 1 has length h_n = t[n+1] - t[n] and its own prior pair (Q, R) = (q, r)[slot[n]]: steps of one length share a
// slot (rodeo_amd/grid.py: grid_slots).  The step is fwd_kernel's -- predict_block, interrogate_traj, update_block_m1,
// store_moments -- with that pair and with the interrogation at the table's time t[n+1], not at step_time(a, n).
// Pairs: (n_slots, D, P, P) row-major, or (n_slots, D, P, P, B) batch-minor where the flag says so.
#pragma once
#include "rk_enums.hpp"
#include "kalman_small.hpp"
#include "philox.hpp"
#include "solve_args.hpp"
#include "solve_small_kernels.hpp"

namespace rk {

// the device side of rk_grid_in
struct GridArgs {
    const double* t;         // (N + 1) node times
    const int* slot;         // (N) slot of every step
    const double *q, *r;     // the pairs
    int q_b, r_b, n_slots;
};

// slot of step n, clamped to the pairs that exist: a table that breaks the rule reads another pair, never outside q / r
__device__ __forceinline__ int grid_clamp(const GridArgs& g, int s) { return s < 0 ? 0 : (s >= g.n_slots ? g.n_slots - 1 : s); }
__device__ __forceinline__ int grid_slot(const GridArgs& g, int n) { return grid_clamp(g, g.slot[n]); }

// (Q, R) of slot s for block blk of trajectory b.  The batched flag is tested once per matrix (it is uniform in a wave), not
// per element as ld() does: a shared matrix is then read at constant offsets from one base, with no address arithmetic per
// element -- on one wave per SIMD the selects and 64-bit adds of 36 ld() calls cost the forward step as much again as its
// fp64 work.
template <int P>
__device__ __forceinline__ void grid_load_matrix(const double* m, int batched, int B, int b, double (&M)[P][P]) {
    if (batched) {
        const double* mine = m + b;
#pragma unroll
        for (int e = 0; e < P * P; ++e) M[e / P][e % P] = mine[(size_t)e * B];
    } else {
#pragma unroll
        for (int e = 0; e < P * P; ++e) M[e / P][e % P] = m[e];
    }
}
template <int P>
__device__ __forceinline__ void grid_load_pair(const GridArgs& g, int B, int D, int s, int blk, int b, double (&Q)[P][P],
                                               double (&R)[P][P]) {
    const size_t at = ((size_t)s * D + blk) * P * P;
    grid_load_matrix<P>(g.q + at * (g.q_b ? (size_t)B : 1), g.q_b, B, b, Q);
    grid_load_matrix<P>(g.r + at * (g.r_b ? (size_t)B : 1), g.r_b, B, b, R);
}

// One step of a lane, fwd_kernel's: predictions of every block under (Q, R), the interrogation at time t, the updates and the
// stores of node n + 1 (`live`: false for a lane past B that only helps to stage the pairs and writes nothing).
template <class RHS, int P, int ITG>
__device__ __forceinline__ void grid_step(const SolveArgs& a, const double (&Q)[RHS::D][P][P], const double (&R)[RHS::D][P][P],
                                          const double (&W)[RHS::D][P], const double (&th)[RHS::NTHETA], double t, int n,
                                          uint32_t traj, int b, bool live, double (&mu)[RHS::D][P], double (&S)[RHS::D][P][P]) {
    constexpr int D = RHS::D;
    double mup[D][P], Sp[D][P][P];
#pragma unroll
    for (int blk = 0; blk < D; ++blk) predict_block<P>(Q[blk], R[blk], mu[blk], S[blk], mup[blk], Sp[blk]);
    double wgt[D][P], am[D], V[D];
    interrogate_traj<RHS, P, ITG>(W, th, t, mup, Sp, a.seed, traj, (uint32_t)n, wgt, am, V);
#pragma unroll
    for (int blk = 0; blk < D; ++blk) {
        double Wm[P];
#pragma unroll
        for (int j = 0; j < P; ++j) Wm[j] = W[blk][j] + wgt[blk][j];                          // solve.py:79
        update_block_m1<P>(Wm, am[blk], V[blk], mup[blk], Sp[blk], mu[blk], S[blk]);
        if (live) store_moments<P>(a.mean, a.var, (size_t)a.B, D, n + 1, blk, b, mu[blk], S[blk]);
    }
}

// Where does the forward lane keep its pairs?  With D P^2 <= 32 doubles per matrix set it holds TWO sets in registers: the pair
// of step n + 1 is fetched while step n computes and rotated in behind it (bwd_walk's software prefetch, lane_backward.hpp).
// Beyond, a second set costs more scratch than fwd_kernel needs at the same (RHS, P, ITG) -- the rule an instance ships by,
// DESIGN.md section 7 (15) -- wherever it is declared: the compiler moves the loads up and spills.  There a shared pair is
// STAGED in LDS (two buffers of 2 D P^2 doubles): the wave fetches the next pair together, at most three doubles in flight per
// lane, writes it behind the step and the predictions read their operands from LDS, every lane the same address; a pair with
// a batch axis goes to a row of LDS per lane at the top of its step, without a prefetch, and is read from there.
template <class RHS, int P>
constexpr bool grid_two_sets() { return RHS::D * P * P <= 32; }

// forward pass, one lane per trajectory: fwd_kernel's layout, stores and draws (keyed by trajectory and step).  No step waits
// for a load that depends on another load: the time of step n + 1 is fetched one step ahead like its pair, the slot two, and
// a fetched slot is first looked at (clamped) one step after its load was issued.
template <class RHS, int P, int ITG>
__global__ void __launch_bounds__(64) grid_fwd_kernel(SolveArgs a, GridArgs g) {
    constexpr int D = RHS::D, E = D * P * P;
    constexpr bool TWO = grid_two_sets<RHS, P>();
    const int lane_b = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = lane_b < a.B;
    if (TWO && !live) return;
    const int b = live ? lane_b : a.B - 1;                                                   // (a lane past B reads a trajectory that exists)
    double W[D][P], th[RHS::NTHETA], mu[D][P], S[D][P][P];
    {
        double Q0[D][P][P], R0[D][P][P];
        lane_load_model<RHS, P>(a, b, Q0, R0, W, th);                                        // W and theta: the plan's own pair is not read
    }
    lane_load_init<D, P>(a, b, mu, S);
    if (live) store_moments_all<D, P>(a.mean, a.var, (size_t)a.B, 0, b, mu, S);              // time index 0
    const uint32_t traj = (uint32_t)(a.traj_offset + (uint64_t)b);
    double t = g.t[1];
    int s_next = a.N >= 2 ? g.slot[1] : 0;                   // slot of step n + 1 as the table has it: clamped where it is used

    if constexpr (TWO) {
        double Q[D][P][P], R[D][P][P];
#pragma unroll
        for (int blk = 0; blk < D; ++blk) grid_load_pair<P>(g, a.B, D, grid_slot(g, 0), blk, b, Q[blk], R[blk]);
        // The loads above are complete before the loop is entered (vmcnt(0); expcnt and lgkmcnt left alone).  Without this the
        // compiler's wait for them lands in the loop body behind the prefetch it has just issued, where only vmcnt(0) covers
        // them: every step then waits for its own prefetch (5.52 against 2.54 ms for fwd_kernel on the headline shape).
        __builtin_amdgcn_s_waitcnt(0x0F70);
        for (int n = 0; n < a.N; ++n) {
            const bool more = n + 1 < a.N;
            double Qn[D][P][P], Rn[D][P][P], tn = t;
            int s_after = 0;
            if (more) {
#pragma unroll
                for (int blk = 0; blk < D; ++blk) grid_load_pair<P>(g, a.B, D, grid_clamp(g, s_next), blk, b, Qn[blk], Rn[blk]);
                tn = g.t[n + 2];
                if (n + 2 < a.N) s_after = g.slot[n + 2];
            }
            grid_step<RHS, P, ITG>(a, Q, R, W, th, t, n, traj, b, true, mu, S);
            if (more) {
                t = tn;
                // (the fetched slot stays in a vector register until here: the table may alias the stores for all the compiler
                // knows, so it is read with a vector load, and moved to a scalar register -- with a wait for every load in flight,
                // the prefetch included -- right behind that load unless something holds it back)
                asm volatile("" : "+v"(s_after));
                s_next = s_after;
#pragma unroll
                for (int blk = 0; blk < D; ++blk)
#pragma unroll
                    for (int i = 0; i < P; ++i)
#pragma unroll
                        for (int j = 0; j < P; ++j) {
                            Q[blk][i][j] = Qn[blk][i][j];
                            R[blk][i][j] = Rn[blk][i][j];
                        }
            }
        }
    } else {
        // LDS of the workgroup, which is one wave: a row of 2 E + 1 doubles per lane for pairs with a batch axis (the odd
        // length keeps the 64 rows off each other's banks), or two buffers of 2 E at its start for a shared pair
        __shared__ double lds[64 * (2 * E + 1)];
        using Mats = const double[D][P][P];
        if (g.q_b || g.r_b) {                            // (wave-uniform) every lane stages its own pair at the top of the step
            if (!live) return;
            double* mine = lds + threadIdx.x * (2 * E + 1);
            int s = g.slot[0];
            for (int n = 0; n < a.N; ++n) {
                const size_t at = (size_t)grid_clamp(g, s) * E;
                const double* qs = g.q + at * (g.q_b ? (size_t)a.B : 1);
                const double* rs = g.r + at * (g.r_b ? (size_t)a.B : 1);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    mine[e] = ld(qs, e, g.q_b, a.B, b);
                    mine[E + e] = ld(rs, e, g.r_b, a.B, b);
                }
                double tn = t;
                int s_after = 0;
                if (n + 1 < a.N) {
                    tn = g.t[n + 2];
                    if (n + 2 < a.N) s_after = g.slot[n + 2];
                }
                grid_step<RHS, P, ITG>(a, *reinterpret_cast<Mats*>(mine), *reinterpret_cast<Mats*>(mine + E), W, th, t, n, traj, b,
                                       true, mu, S);
                t = tn;
                s = s_next;
                s_next = s_after;
            }
        } else {                                         // a shared pair, staged by the whole wave one step ahead
            constexpr int KE = (2 * E + 63) / 64;
            // element e of a staged pair: Q (D, P, P) row-major for e < E, then R, as the slot lies in global memory
            const auto src = [&](int slot, int e) { return e < E ? g.q + (size_t)slot * E + e : g.r + (size_t)slot * E + (e - E); };
            {
                const int s0 = grid_slot(g, 0);
#pragma unroll
                for (int k = 0; k < KE; ++k) {
                    const int e = (int)threadIdx.x + 64 * k;
                    if (e < 2 * E) lds[e] = *src(s0, e);
                }
            }
            __syncthreads();
            for (int n = 0; n < a.N; ++n) {
                const bool more = n + 1 < a.N;
                const double* cur = lds + (n & 1) * 2 * E;
                double* nxt = lds + ((n & 1) ^ 1) * 2 * E;
                double pre[KE], tn = t;
                int s_after = 0;
                if (more) {
#pragma unroll
                    for (int k = 0; k < KE; ++k) {
                        const int e = (int)threadIdx.x + 64 * k;
                        pre[k] = e < 2 * E ? *src(grid_clamp(g, s_next), e) : 0.0;
                    }
                    tn = g.t[n + 2];
                    if (n + 2 < a.N) s_after = g.slot[n + 2];
                }
                grid_step<RHS, P, ITG>(a, *reinterpret_cast<Mats*>(cur), *reinterpret_cast<Mats*>(cur + E), W, th, t, n, traj, b,
                                       live, mu, S);
                if (more) {
                    t = tn;
                    asm volatile("" : "+v"(s_after));    // (as in the two-set loop above)
                    s_next = s_after;
#pragma unroll
                    for (int k = 0; k < KE; ++k) {
                        const int e = (int)threadIdx.x + 64 * k;
                        if (e < 2 * E) nxt[e] = pre[k];
                    }
                }
                __syncthreads();                         // the staged pair of step n + 1 is written, that of step n read
            }
        }
    }
}

}  // namespace rk
