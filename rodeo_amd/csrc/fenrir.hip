// Fenrir in the covariance form (src/rodeo/inference/fenrir.py): the backward filter over the stored forward moments, the
// smoothing sweep of fenrir's solve_mv, and the C entries rk_fenrir_backward, rk_fenrir_workspace_bytes, rk_fenrir_solve_mv and
// rk_fenrir_solve_mv_tiles, which also route to the other forms: square-root (fenrir_sqrt.hip), the n_bstate = 3 tiles
// (solve_tile3.hip).  Observations at arbitrary times: fenrir_at.hip.  The pieces shared with fenrir_bwd_at_kernel and the layout
// of the stored item are in fenrir_kernels.hpp.
#include "common.hpp"
#include "kalman_small.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "fenrir_kernels.hpp"
#include "records.hpp"

namespace rk {

// ---- Fenrir backward pass (src/rodeo/inference/fenrir.py:86-259), scalar observations per block --------------------
// One lane per (block, trajectory): the backward Markov chain X_n = A_n X_{n+1} + b_n + C_n^{1/2} eps
// (smooth_cond, standard.py:366-370) is run as a Kalman filter backwards in time over the stored forward moments
// (batch-minor filt and pred), conditioning on the observations y_i = D_i X_{n(i)} + N(0, Omega_i) at their grid
// indices; every observation contributes log N(y_i; D m, D S D^T + Omega) with utils.py:60-78's rule that a variance
// with |w| <= 1e-8 contributes nothing (jnp.isclose(w, 0, rtol=1e-300)).  Block values are summed per trajectory.
// With STORE (fenrir.py:236-258, for fenrir's solve_mv) the backward filter's predicted and updated moments of every
// time and the Markov weights A_n are kept in `states`: per (time n, block) one FenrirItem (fenrir_kernels.hpp), batch-minor.
// MO = n_bobs (observations per block, fenrir.py:106-122): obs (n_obs, d, MO), obs_w (n_obs, d, MO, P), obs_v (n_obs, d, MO, MO)
// TILES: the forward pass ran on the blocked MFMA tiles (n_bstate 4 .. 8): `tiles` holds its records and the predicted
// moments are re-evaluated from the filtered ones (standard.py:57-59, what the forward pass computed) instead of read.
template <int P, bool STORE, int MO, bool TILES = false>
__global__ void __launch_bounds__(64) fenrir_bwd_kernel(SolveArgs a, const double* __restrict__ obs,
                                                        const double* __restrict__ obs_w, const double* __restrict__ obs_v,
                                                        const int32_t* __restrict__ obs_ind, int n_obs,
                                                        double* __restrict__ logdens, double* __restrict__ states,
                                                        const double* __restrict__ tiles = nullptr) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= a.B * a.D) return;
    const int blk = l / a.B, b = l - blk * a.B;
    const size_t B = (size_t)a.B;
    double Q[P][P], R[P][P];
    load_block_consts<P>(a, blk, b, Q, R);
    double bm[P], bS[P][P];
    // the filtered moments: the blocked tiles' records (RK_LAYOUT_TILE4 and RK_LAYOUT_TILEP are the same [Sigma | mu] record
    // to load_moments), or batch-minor a.mean / a.var
    if constexpr (TILES) load_moments<P, RK_LAYOUT_TILEP>(a.mean, tiles, B, a.D, a.N, blk, b, bm, bS);
    else load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, a.N, blk, b, bm, bS);   // terminal point (fenrir.py:186-188)
    double acc = 0.0;
    int i = n_obs - 1;
    // conditioning on observation i: forecast (standard.py:333-335) + log-density + update (standard.py:93-102)
    const DaltonObs o{obs, obs_w, obs_v, obs_ind, n_obs};
    auto observe = [&](double (&m)[P], double (&S)[P][P]) {
        if constexpr (MO == 1) fenrir_observe_scalar<P>(o, (size_t)i * a.D + blk, m, S, acc);
        else dalton_observe<P, MO>(o, (size_t)i * a.D + blk, m, S, acc);
        --i;
    };
    constexpr FenrirItem IT(P);
    auto keep = [&](int n, int off, const double (&m)[P], const double (&S)[P][P]) {
        double* o = states + (((size_t)n * a.D + blk) * IT.width + off) * B + b;
#pragma unroll
        for (int r = 0; r < P; ++r) {
            o[(size_t)r * B] = m[r];
#pragma unroll
            for (int c = 0; c < P; ++c) o[(size_t)(P + r * P + c) * B] = S[r][c];
        }
    };
    if constexpr (STORE) keep(a.N, IT.pred, bm, bS);                        // "prediction" at N = the terminal point
    if (i >= 0 && obs_ind[i] >= a.N) observe(bm, bS);                      // fenrir.py:189-209
    if constexpr (STORE) keep(a.N, IT.filt, bm, bS);
    for (int n = a.N - 1; n >= 0; --n) {
        double mf[P], Sf[P][P], mp[P], Sp[P][P], G[P][P];
        if constexpr (TILES) {
            load_moments<P, RK_LAYOUT_TILEP>(a.mean, tiles, B, a.D, n, blk, b, mf, Sf);
            predict_block<P>(Q, R, mf, Sf, mp, Sp);                         // pred[n + 1] from filt[n]
        } else {
            load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, n, blk, b, mf, Sf);
            // stored predicted moments of time n + 1 (solve.py:93-96)
            const double* mi = a.mean_pred + ((size_t)(n + 1) * a.D + blk) * P * B + b;
            const double* vi = a.var_pred + ((size_t)(n + 1) * a.D + blk) * P * P * B + b;
#pragma unroll
            for (int r = 0; r < P; ++r) {
                mp[r] = mi[(size_t)r * B];
#pragma unroll
                for (int c = 0; c < P; ++c) Sp[r][c] = vi[((size_t)r * P + c) * B];
            }
        }
        fenrir_markov_step<P>(Q, mf, Sf, mp, Sp, bm, bS, G);
        if constexpr (STORE) {
            keep(n, IT.pred, bm, bS);
            double* o = states + (((size_t)n * a.D + blk) * IT.width + IT.A) * B + b;
#pragma unroll
            for (int r = 0; r < P; ++r)
#pragma unroll
                for (int c = 0; c < P; ++c) o[(size_t)(r * P + c) * B] = G[r][c];
        }
        if (i >= 0 && obs_ind[i] == n) observe(bm, bS);                     // fenrir.py:155-170
        if constexpr (STORE) keep(n, IT.filt, bm, bS);
    }
    if (logdens) atomicAdd(&logdens[b], acc);
}

// fenrir.py:333-402: the smoothing pass over the backward filter's stored moments, a forward sweep in time -- times 0 and
// 1 keep the backward filter's own estimates; for k = 0 .. N-2
//     (m, S)_{k+2} = smooth_mv(next = (m, S)_{k+1}, wgt_state = A_{k+1}, filt = bfilt_{k+2}, pred = bpred_{k+1}).
// Results go to a.mean / a.var (batch-minor), which the backward filter no longer needs.
template <int P>
__global__ void __launch_bounds__(64) fenrir_smooth_kernel(SolveArgs a, const double* __restrict__ states) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= a.B * a.D) return;
    const int blk = l / a.B, b = l - blk * a.B;
    const size_t B = (size_t)a.B;
    constexpr FenrirItem IT(P);
    auto item = [&](int n, int off, double (&m)[P], double (&S)[P][P]) {
        const double* o = states + (((size_t)n * a.D + blk) * IT.width + off) * B + b;
#pragma unroll
        for (int r = 0; r < P; ++r) {
            m[r] = o[(size_t)r * B];
#pragma unroll
            for (int c = 0; c < P; ++c) S[r][c] = o[(size_t)(P + r * P + c) * B];
        }
    };
    auto put = [&](int n, const double (&m)[P], const double (&S)[P][P]) {
        double* mo = a.mean + ((size_t)n * a.D + blk) * P * B + b;
        double* vo = a.var + ((size_t)n * a.D + blk) * P * P * B + b;
#pragma unroll
        for (int r = 0; r < P; ++r) {
            mo[(size_t)r * B] = m[r];
#pragma unroll
            for (int c = 0; c < P; ++c) vo[((size_t)r * P + c) * B] = S[r][c];
        }
    };
    double cm[P], cS[P][P];
    item(0, IT.filt, cm, cS);
    put(0, cm, cS);
    if (a.N < 1) return;
    item(1, IT.filt, cm, cS);
    put(1, cm, cS);
    for (int k = 0; k + 2 <= a.N; ++k) {
        double fm[P], fS[P][P], pm[P], pS[P][P], A[P][P], T[P][P], G[P][P];
        item(k + 2, IT.filt, fm, fS);
        item(k + 1, IT.pred, pm, pS);
        {
            const double* o = states + (((size_t)(k + 1) * a.D + blk) * IT.width + IT.A) * B + b;
#pragma unroll
            for (int r = 0; r < P; ++r)
#pragma unroll
                for (int c = 0; c < P; ++c) A[r][c] = o[(size_t)(r * P + c) * B];
        }
        smooth_gain<P>(A, fS, pS, T, G);                                    // standard.py:175-176 with wgt_state = A
        double dm[P], dS[P][P], GD[P][P], nS[P][P];
#pragma unroll
        for (int r = 0; r < P; ++r) {
            dm[r] = cm[r] - pm[r];
#pragma unroll
            for (int c = 0; c < P; ++c) dS[r][c] = cS[r][c] - pS[r][c];
        }
        mm<P, P, P>(G, dS, GD);
        mm_nt<P, P, P>(GD, G, nS);
#pragma unroll
        for (int r = 0; r < P; ++r) {
            cm[r] = fm[r] + dot<P>(G[r], dm);                               // standard.py:213-214
#pragma unroll
            for (int c = 0; c < P; ++c) cS[r][c] = fS[r][c] + nS[r][c];     // standard.py:215-216
        }
        put(k + 2, cm, cS);
    }
}

// fenrir's backward filter, one lane per (block, trajectory): fenrir_bwd_kernel<P, STORE, n_bobs, TILES> for P in [PLO, PHI]
// (tiles: the records of the blocked-tile forward pass, TILES only)
template <int PLO, int PHI, bool STORE, bool TILES>
static int launch_fenrir_bwd(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, int n_bobs, const double* obs,
                             const double* obs_w, const double* obs_v, const int32_t* obs_ind, int n_obs, double* logdens,
                             double* states, const double* tiles) {
    const dim3 grid(div_up(a.B * a.D, 64)), block(64);
    LaunchTimer t(h, TILES ? "fenrir_bwd_kernel<tiles>" : "fenrir_bwd_kernel");
    dispatch_int<PLO, PHI>(c->n_bstate, [&](auto P) {
        dispatch_int<1, 3>(n_bobs, [&](auto M) {
            hipLaunchKernelGGL((fenrir_bwd_kernel<P, STORE, M, TILES>), grid, block, 0, h->stream, a, obs, obs_w, obs_v, obs_ind, n_obs,
                               logdens, states, tiles);
        });
    });
    t.stop();
    RK_HIP(hipGetLastError());
    return RK_OK;
}

// fenrir's smoothing sweep over the stored backward filter (fenrir_smooth_kernel<P>), P in [PLO, PHI]
template <int PLO, int PHI>
static int launch_fenrir_smooth(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const double* states) {
    const dim3 grid(div_up(a.B * a.D, 64)), block(64);
    LaunchTimer t(h, "fenrir_smooth_kernel");
    dispatch_int<PLO, PHI>(c->n_bstate, [&](auto P) {
        hipLaunchKernelGGL(fenrir_smooth_kernel<P>, grid, block, 0, h->stream, a, states);
    });
    t.stop();
    RK_HIP(hipGetLastError());
    return RK_OK;
}

// the sweep on the lane route's n_bstate 2 .. 6 (also the last launch of rk_fenrir_grid_solve_mv, fenrir_grid.hip: declared in
// solve_paths.hpp)
int launch_fenrir_smooth_lanes(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const double* states) {
    return launch_fenrir_smooth<2, 6>(h, c, a, states);
}

// what every route does once its arguments are accepted: the kernels' argument block, the device, and (logdens given) the
// zeroed per-trajectory sums that the lanes of a trajectory's blocks add to
static int fenrir_begin(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, double* logdens,
                        SolveArgs& a) {
    const int rc = make_args(c, in, out, a);
    if (rc) return rc;
    RK_HIP(hipSetDevice(h->device));
    if (logdens) RK_HIP(hipMemsetAsync(logdens, 0, sizeof(double) * (size_t)c->n_traj, h->stream));
    return RK_OK;
}

// fenrir's solve_mv on the lanes: the backward filter keeps its moments in `workspace`, the smoothing sweep reads them.  TILES: the
// forward pass's records are out->var_state and the sweep writes mean_out / var_out; else it overwrites out->mean_state / var_state.
template <int PLO, int PHI, bool TILES>
static int fenrir_solve_mv_lanes(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, const double* obs,
                                 const double* obs_weight, const double* obs_var, const int32_t* obs_ind, int n_obs, int n_bobs,
                                 void* workspace, double* mean_out, double* var_out) {
    SolveArgs a;
    int rc = fenrir_begin(h, c, in, out, nullptr, a);
    if (rc) return rc;
    if (TILES) { a.mean = mean_out; a.var = var_out; }              // (the smoothing pass's output; the backward filter reads the records)
    double* st = (double*)workspace;
    rc = launch_fenrir_bwd<PLO, PHI, true, TILES>(h, c, a, n_bobs, obs, obs_weight, obs_var, obs_ind, n_obs, nullptr, st,
                                                  TILES ? out->var_state : nullptr);
    if (rc) return rc;
    return launch_fenrir_smooth<PLO, PHI>(h, c, a, st);
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_fenrir_backward(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out,
                       const double* obs, const double* obs_weight, const double* obs_var, const int32_t* obs_ind,
                       int32_t n_obs, int32_t n_bobs, double* logdens) {
    RK_REQUIRE(h && c && in && out && obs && obs_weight && obs_var && obs_ind && logdens, RK_ERR_INVALID,
               "rk_fenrir_backward: null argument");
    RK_REQUIRE(n_bobs >= 1 && n_bobs <= 3, RK_ERR_UNSUPPORTED, "rk_fenrir_backward: n_bobs in 1..3, got %d", n_bobs);
    if (c->kalman_type == RK_KALMAN_SQRT) {
        // fenrir.py:292-296: every step map from square_root.py; the filtered FACTORS of the square-root forward pass
        // (batch-minor, solve_sqrt.hip) are all it needs -- the predicted ones are re-evaluated (fenrir_sqrt.hip)
        RK_REQUIRE(out->mean_state && out->var_state && n_obs >= 0, RK_ERR_INVALID,
                   "rk_fenrir_backward (square-root): out->mean_state / var_state of rk_solve_filter are null");
        SolveArgs as;
        const int rcs = fenrir_begin(h, c, in, out, logdens, as);
        if (rcs) return rcs;
        return fenrir_sqrt_launch(h, c, as, obs, obs_weight, obs_var, obs_ind, n_obs, n_bobs, logdens, nullptr);
    }
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD, RK_ERR_UNSUPPORTED, "rk_fenrir_backward: unknown kalman_type %d", c->kalman_type);
    const bool own_layout = !(c->flags & (RK_FLAG_STORE_PRED | RK_FLAG_BATCH_MINOR));
    const SolvePath fpath = own_layout ? solve_path(c, RK_MODE_FILTER) : SolvePath::Small;      // the route rk_solve_filter took
    if (n_bobs == 1 && fpath == SolvePath::Tile3) {
        // the filter ran on the MFMA-tile path: out->var_state holds the RK_LAYOUT_TILE3 tiles, predicted moments are
        // re-evaluated from the filtered ones (solve_tile3.hip, fenrir_bwd_tile3_kernel)
        RK_REQUIRE(out->var_state && n_obs >= 0, RK_ERR_INVALID, "rk_fenrir_backward: out->var_state (tiles) is null");
        SolveArgs at;
        const int rct = fenrir_begin(h, c, in, out, logdens, at);
        if (rct) return rct;
        return tile3_fenrir_backward(h, at, out->var_state, obs, obs_weight, obs_var, obs_ind, n_obs, logdens);
    }
    if (fpath == SolvePath::Tile4 || fpath == SolvePath::TileN) {
        // the filter ran on the blocked MFMA tiles (n_bstate 4 .. 8): out->var_state holds its records [Sigma | mu]; the
        // backward filter runs one lane per (block, trajectory) on them and re-evaluates the predicted moments
        RK_REQUIRE(out->var_state && n_obs >= 0, RK_ERR_INVALID, "rk_fenrir_backward: out->var_state (tiles) is null");
        SolveArgs at;
        const int rct = fenrir_begin(h, c, in, out, logdens, at);
        if (rct) return rct;
        return launch_fenrir_bwd<4, 8, false, true>(h, c, at, n_bobs, obs, obs_weight, obs_var, obs_ind, n_obs, logdens, nullptr, out->var_state);
    }
    RK_REQUIRE(out->mean_state && out->var_state && out->mean_pred && out->var_pred, RK_ERR_INVALID,
               "rk_fenrir_backward needs the batch-minor filtered AND predicted moments of rk_solve_filter "
               "(RK_FLAG_STORE_PRED | RK_FLAG_BATCH_MINOR), or a configuration of the tile paths (n_bstate = 3 .. 8) without them");
    RK_REQUIRE(c->n_bstate >= 2 && c->n_bstate <= 6 && n_obs >= 0, RK_ERR_UNSUPPORTED,
               "rk_fenrir_backward: n_bstate in 2..6");
    SolveArgs a;
    const int rc = fenrir_begin(h, c, in, out, logdens, a);
    if (rc) return rc;
    return launch_fenrir_bwd<2, 6, false, false>(h, c, a, n_bobs, obs, obs_weight, obs_var, obs_ind, n_obs, logdens, nullptr, nullptr);
}

int rk_fenrir_workspace_bytes(const rk_solve_cfg* c, size_t* bytes) {
    RK_REQUIRE(c && bytes, RK_ERR_INVALID, "rk_fenrir_workspace_bytes: null argument");
    const size_t item = c->kalman_type == RK_KALMAN_SQRT ? fenrir_sqrt_item_doubles(c->n_bstate) : (size_t)FenrirItem(c->n_bstate).width;
    *bytes = sizeof(double) * (size_t)(c->n_steps + 1) * c->n_block * item * c->n_traj;
    return RK_OK;
}

// fenrir's solve_mv on the records of the blocked-tile forward pass (n_bstate 4 .. 8, rk_solve_filter without RK_FLAG_STORE_PRED |
// RK_FLAG_BATCH_MINOR): out->var_state holds the records [Sigma | mu] per (time, trajectory, block); the backward filter re-evaluates
// the predicted moments from them (fenrir_bwd_kernel<.., STORE, .., TILES>), the smoothing pass writes mean_out (N+1, d, p, B) and
// var_out (N+1, d, p, p, B), batch-minor.
int rk_fenrir_solve_mv_tiles(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out,
                             const double* obs, const double* obs_weight, const double* obs_var, const int32_t* obs_ind,
                             int32_t n_obs, int32_t n_bobs, void* workspace, double* mean_out, double* var_out) {
    RK_REQUIRE(h && c && in && out && obs && obs_weight && obs_var && obs_ind && workspace && mean_out && var_out, RK_ERR_INVALID,
               "rk_fenrir_solve_mv_tiles: null argument");
    const SolvePath fpath = !(c->flags & (RK_FLAG_STORE_PRED | RK_FLAG_BATCH_MINOR)) ? solve_path(c, RK_MODE_FILTER) : SolvePath::Small;
    RK_REQUIRE(fpath == SolvePath::Tile4 || fpath == SolvePath::TileN, RK_ERR_UNSUPPORTED,
               "rk_fenrir_solve_mv_tiles: a configuration of the blocked-tile forward pass (kalman_type standard, n_bstate 4..8, no "
               "RK_FLAG_STORE_PRED / RK_FLAG_BATCH_MINOR)");
    RK_REQUIRE(out->var_state && n_obs >= 0 && n_bobs >= 1 && n_bobs <= 3, RK_ERR_INVALID,
               "rk_fenrir_solve_mv_tiles: out->var_state (tile records) is null, or n_bobs outside 1..3");
    return fenrir_solve_mv_lanes<4, 8, true>(h, c, in, out, obs, obs_weight, obs_var, obs_ind, n_obs, n_bobs, workspace, mean_out, var_out);
}

int rk_fenrir_solve_mv(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out,
                       const double* obs, const double* obs_weight, const double* obs_var, const int32_t* obs_ind,
                       int32_t n_obs, int32_t n_bobs, void* workspace) {
    RK_REQUIRE(h && c && in && out && obs && obs_weight && obs_var && obs_ind && workspace, RK_ERR_INVALID,
               "rk_fenrir_solve_mv: null argument");
    if (c->kalman_type == RK_KALMAN_SQRT) {                          // fenrir.py:421-426 (fenrir_sqrt.hip)
        RK_REQUIRE(out->mean_state && out->var_state && n_obs >= 0, RK_ERR_INVALID,
                   "rk_fenrir_solve_mv (square-root): out->mean_state / var_state of rk_solve_filter are null");
        SolveArgs as;
        const int rcs = fenrir_begin(h, c, in, out, nullptr, as);
        if (rcs) return rcs;
        return fenrir_sqrt_launch(h, c, as, obs, obs_weight, obs_var, obs_ind, n_obs, n_bobs, nullptr, (double*)workspace);
    }
    RK_REQUIRE(c->kalman_type == RK_KALMAN_STANDARD, RK_ERR_UNSUPPORTED, "rk_fenrir_solve_mv: unknown kalman_type %d", c->kalman_type);
    RK_REQUIRE((c->flags & RK_FLAG_STORE_PRED) && (c->flags & RK_FLAG_BATCH_MINOR) && out->mean_state && out->var_state &&
               out->mean_pred && out->var_pred, RK_ERR_INVALID,
               "rk_fenrir_solve_mv needs the batch-minor filtered AND predicted moments of rk_solve_filter "
               "(RK_FLAG_STORE_PRED | RK_FLAG_BATCH_MINOR)");
    RK_REQUIRE(c->n_bstate >= 2 && c->n_bstate <= 6 && n_obs >= 0 && n_bobs >= 1 && n_bobs <= 3, RK_ERR_UNSUPPORTED,
               "rk_fenrir_solve_mv: n_bstate in 2..6, n_bobs in 1..3");
    return fenrir_solve_mv_lanes<2, 6, false>(h, c, in, out, obs, obs_weight, obs_var, obs_ind, n_obs, n_bobs, workspace, nullptr, nullptr);
}

}  // extern "C"
