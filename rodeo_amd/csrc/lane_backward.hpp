// What the lane-per-(block, trajectory) backward passes of the standard form share ("One walk for the lane
// backward passes"): the lane and its model constants, the walk down the filtered records -- load, prefetch, re-evaluated
// prediction, smoothing gain, rotation -- under a prediction policy and a step, a sampled path's stores, and the smoothing and
// one-draw sampling passes built from them: bwd_mv_kernel / bwd_sim_kernel (solve_small.hip), dynamic_bwd_mv_kernel /
// dynamic_bwd_sim_kernel (dynamic.hip), grid_bwd_mv_kernel / grid_bwd_sim_kernel (grid.hip); bwd_sim_draws_kernel
// (sim_draws.hip) mirrors them.  Ahead-of-time code only.
#pragma once
#include "records.hpp"
#include "kalman_small.hpp"
#include "philox.hpp"

namespace rk {

// ---- the lane ------------------------------------------------------------------------------------------------------------
// (block, trajectory) of this thread on a grid of bwd_lane_geom (blockIdx.x alone), its Philox trajectory and its Q, R
template <int P>
struct BwdLane {
    int blk, b;
    size_t B;
    uint32_t traj;
    double Q[P][P], R[P][P];
    // false for a lane past B * D, which has nothing to do
    __device__ __forceinline__ bool init(const SolveArgs& a) {
        const int l = blockIdx.x * blockDim.x + threadIdx.x;
        if (l >= a.B * a.D) return false;
        record_lane<RK_LAYOUT_BATCH_MINOR>(l, a.B, a.D, blk, b);
        B = (size_t)a.B;
        traj = (uint32_t)(a.traj_offset + (uint64_t)b);
        load_block_consts<P>(a, blk, b, Q, R);
        return true;
    }
    // the filtered (or, behind the smoother, smoothed) moments of time n
    __device__ __forceinline__ void load(const SolveArgs& a, int n, double (&m)[P], double (&S)[P][P]) const {
        load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, n, blk, b, m, S);
    }
};

// ---- sampled paths -------------------------------------------------------------------------------------------------------
// x to row `row` of a batch-minor path array (rows, D, P, B): the time n of x_state, (s K + k) of x_draws
template <int P>
__device__ __forceinline__ void store_path(double* path, size_t row, int D, const BwdLane<P>& ln, const double (&x)[P]) {
    double* xo = path + (row * D + ln.blk) * P * ln.B + ln.b;
#pragma unroll
    for (int i = 0; i < P; ++i) xo[(size_t)i * ln.B] = x[i];
}

// x[0] = ode_init exactly (solve.py:196-204): the mean of time 0, which the forward pass wrote
template <int P>
__device__ __forceinline__ void load_path_init(const SolveArgs& a, const BwdLane<P>& ln, double (&x0)[P]) {
#pragma unroll
    for (int i = 0; i < P; ++i) x0[i] = a.mean[((size_t)ln.blk * P + i) * ln.B + ln.b];
}

// ---- the walk ------------------------------------------------------------------------------------------------------------
// A prediction policy has Datum, what it needs of a node next to the node's moments, fetch(a, ln, n), predict(ln, datum,
// mf, Sf, mp, Sp) and trans(ln, datum), the transition matrix of the step that the smoothing gain needs.  The static prior's:
// predict_block, nothing to fetch, the lane's Q (the dynamic solver's is ScaledPrior in dynamic.hip, the grid solver's SlotPrior
// in grid.hip, the one whose Q changes from step to step).
template <int P>
struct StaticPrior {
    struct Datum {};
    __device__ __forceinline__ Datum fetch(const SolveArgs&, const BwdLane<P>&, int) const { return {}; }
    __device__ __forceinline__ void predict(const BwdLane<P>& ln, Datum, const double (&mf)[P], const double (&Sf)[P][P],
                                            double (&mp)[P], double (&Sp)[P][P]) const {
        predict_block<P>(ln.Q, ln.R, mf, Sf, mp, Sp);
    }
    __device__ __forceinline__ const auto& trans(const BwdLane<P>& ln, const Datum&) const { return ln.Q; }
};

// Nodes n = N-1 .. 1 (none for N = 1): step(n, mf, Sf, mp, Sp, T, G) with filt[n], pred[n+1] re-evaluated from it and the
// smoothing gain (T, G).  filt[n-1] and the policy's datum of n-1 are fetched before step n computes (a software prefetch)
// and rotated in behind it.  The caller has read filt[N] before: a smoother in place overwrites node n in step n.
template <int P, class Pred, class Step>
__device__ __forceinline__ void bwd_walk(const SolveArgs& a, const BwdLane<P>& ln, const Pred& pred, Step&& step) {
    double mf[P], Sf[P][P];
    typename Pred::Datum c{};
    if (a.N >= 2) {
        ln.load(a, a.N - 1, mf, Sf);
        c = pred.fetch(a, ln, a.N - 1);
    }
    for (int n = a.N - 1; n >= 1; --n) {
        double mfn[P], Sfn[P][P];
        typename Pred::Datum cn{};
        if (n >= 2) {
            ln.load(a, n - 1, mfn, Sfn);
            cn = pred.fetch(a, ln, n - 1);
        }
        double mp[P], Sp[P][P], T[P][P], G[P][P];
        pred.predict(ln, c, mf, Sf, mp, Sp);             // pred[n+1] re-evaluated from filt[n]
        smooth_gain<P>(pred.trans(ln, c), Sf, Sp, T, G);
        step(n, mf, Sf, mp, Sp, T, G);
        if (n >= 2) {
            c = cn;
#pragma unroll
            for (int i = 0; i < P; ++i) {
                mf[i] = mfn[i];
#pragma unroll
                for (int j = 0; j < P; ++j) Sf[i][j] = Sfn[i][j];
            }
        }
    }
}

// ---- the two passes, for the solver (StaticPrior), the dynamic solver (ScaledPrior) and the grid solver (SlotPrior) -------
// solve.py:257-301: smoothing in place over the filtered moments; time 0 keeps the forward pass's (ode_init, 0) (295-301)
template <int P, class Pred>
__device__ __forceinline__ void bwd_smooth_lane(const SolveArgs& a, const BwdLane<P>& ln, const Pred& pred) {
    double ms[P], Ss[P][P];                              // carry: smoothed moments at n+1 (solve.py:279-282)
    ln.load(a, a.N, ms, Ss);
    bwd_walk<P>(a, ln, pred, [&](int n, const auto& mf, const auto& Sf, const auto& mp, const auto& Sp, const auto& /*T*/,
                                 const auto& G) {
        smooth_mv_block<P>(G, mf, Sf, mp, Sp, ms, Ss);
        store_moments<P>(a.mean, a.var, ln.B, a.D, n, ln.blk, ln.b, ms, Ss);
    });
}

// solve.py:162-204: one sample path to a.x, Philox keyed with (seed, trajectory, n, block, PURPOSE_SMOOTH)
template <int P, class Pred>
__device__ __forceinline__ void bwd_sample_lane(const SolveArgs& a, const BwdLane<P>& ln, const Pred& pred) {
    double xn[P], z[P];
    {   // terminal draw x_N ~ N(filt[N]) (solve.py:182-186)
        double mf[P], Sf[P][P];
        ln.load(a, a.N, mf, Sf);
        normals<P>(a.seed, ln.traj, (uint32_t)a.N, (uint32_t)ln.blk, PURPOSE_SMOOTH, z);
        mvn_draw<P>(mf, Sf, z, xn);
        store_path<P>(a.x, (size_t)a.N, a.D, ln, xn);
    }
    bwd_walk<P>(a, ln, pred, [&](int n, const auto& mf, const auto& Sf, const auto& mp, const auto& /*Sp*/, const auto& T,
                                 const auto& G) {
        double msim[P], Ssim[P][P];
        smooth_sim_block<P>(G, T, mf, Sf, mp, xn, msim, Ssim);
        normals<P>(a.seed, ln.traj, (uint32_t)n, (uint32_t)ln.blk, PURPOSE_SMOOTH, z);
        mvn_draw<P>(msim, Ssim, z, xn);
        store_path<P>(a.x, (size_t)n, a.D, ln, xn);
    });
    double x0[P];
    load_path_init<P>(a, ln, x0);
    store_path<P>(a.x, 0, a.D, ln, x0);
}

}  // namespace rk
