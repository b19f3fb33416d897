// fenrir_grid_jvp / fenrir_grid_grad / fenrir_grad (an addition): host side of rk_fenrir_grid_jvp,
// directional derivatives of rk_fenrir_grid_loglik's value with respect to the ODE parameters and the initial state, and the
// backward kernel.  Two launches: fenrir_grid_jvp_fwd_kernel (fenrir_grad_kernels.hpp), one (trajectory, direction) item per
// lane, which stores the primal filtered records in the plan's batch-minor mean / var and every item's tangent records in the
// caller's workspace; then fenrir_grid_jvp_bwd_kernel (below), one lane per (block, item), the derivative of fenrir_grid's
// backward Markov chain; with more than one block, magi_sum_kernel twice (launch_block_sum).  Standard form, n_bmeas = 1,
// n_bobs = 1, built-in FitzHugh-Nagumo and Lorenz63, or a user right-hand side of the gradient kind (hiprtc, rhs_jit.hip's
// JIT_FENRIR_GRAD, the forward kernel only: the backward kernel has no right-hand side).  rk_fenrir_grid_jvp_hyper (section 7 (25))
// is the same entry with the log sigma / log observation variance directions, on the two hyper kernels (written out next to the
// plain ones: section 7 (26)).  The configuration check (grad_check, shared with dalton_grad.hip and worded "not
// built: ..."), the grid's staging, the test of the output pointers and the launch patterns are grid_entry.hpp's.
#include "common.hpp"
#include "rhs.hpp"
#include "kalman_small.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "grid_entry.hpp"
#include "grid_kernels.hpp"
#include "fenrir_kernels.hpp"
#include "records.hpp"
#include "fenrir_grad_kernels.hpp"

namespace rk {

// The tangent of fenrir_markov_step<P> along one direction: given filt[n] = (mf, Sf), pred[n + 1] = (mp, Sp) and their tangents,
// the carry (bm, bS) BEFORE the primal step overwrites it and its tangent (dbm, dbS), which is stepped in place.
//   T = Sigma_f Q^T, T. = Sigma._f Q^T ;  G = T (Sigma-)^-1, G. = (T. - G Sigma.-) (Sigma-)^-1  (a second LU solve on Sigma-, with
//   the transposed right-hand side as smooth_gain does; smooth_gain itself gives T and G)
//   b = mu_f - G mu-            b. = mu._f - G. mu- - G mu.-
//   C = Sigma_f - G T^T         C. = Sigma._f - G. T^T - G T.^T
//   m <- G m + b                m. <- G. m + G m. + b.
//   S <- G S G^T + C            S. <- G. S G^T + G S. G^T + G S G.^T + C.
template <int P>
__device__ __forceinline__ void jvp_markov_step(const double (&Q)[P][P], const double (&Sf)[P][P], const double (&mp)[P],
                                                const double (&Sp)[P][P], const double (&dmf)[P], const double (&dSf)[P][P],
                                                const double (&dmp)[P], const double (&dSp)[P][P], const double (&bm)[P],
                                                const double (&bS)[P][P], double (&dbm)[P], double (&dbS)[P][P]) {
    double T[P][P], G[P][P], dT[P][P], dG[P][P];
    smooth_gain<P>(Q, Sf, Sp, T, G);
    mm_nt<P, P, P>(dSf, Q, dT);
    {
        double GdS[P][P], A[P][P], X[P][P];
        mm<P, P, P>(G, dSp, GdS);
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int j = 0; j < P; ++j) {
                A[i][j] = Sp[i][j];
                X[i][j] = dT[j][i] - GdS[j][i];
            }
        lu_solve<P, P>(A, X);
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int j = 0; j < P; ++j) dG[i][j] = X[j][i];
    }
    double dGT[P][P], GdT[P][P], GS[P][P], dGS[P][P], GdbS[P][P], t1[P][P], t2[P][P], t3[P][P];
    mm_nt<P, P, P>(dG, T, dGT);                                         // G. T^T
    mm_nt<P, P, P>(G, dT, GdT);                                         // G T.^T
    mm<P, P, P>(G, bS, GS);
    mm<P, P, P>(dG, bS, dGS);
    mm<P, P, P>(G, dbS, GdbS);
    mm_nt<P, P, P>(dGS, G, t1);                                         // G. S G^T
    mm_nt<P, P, P>(GdbS, G, t2);                                        // G S. G^T
    mm_nt<P, P, P>(GS, dG, t3);                                         // G S G.^T
    double nm[P];
#pragma unroll
    for (int r = 0; r < P; ++r) {
        const double db = dmf[r] - dot<P>(dG[r], mp) - dot<P>(G[r], dmp);
        nm[r] = dot<P>(dG[r], bm) + dot<P>(G[r], dbm) + db;
#pragma unroll
        for (int c = 0; c < P; ++c) dbS[r][c] = t1[r][c] + t2[r][c] + t3[r][c] + (dSf[r][c] - dGT[r][c] - GdT[r][c]);
    }
#pragma unroll
    for (int r = 0; r < P; ++r) dbm[r] = nm[r];
}

// ---- backward filter and its tangent (n_bobs = 1) --------------------------------------------------------------------------------
// fenrir_grid_bwd_kernel<P, false, 1>'s recursion (fenrir_grid.hip), a sibling of it, not an edit: one lane per (block, item) on
// bwd_lane_geom(B K, D), item = b K + k.  The primal record is read at index b of the plan's batch-minor mean / var, the tangent
// record at index `item` of dmean / dvar (B K items wide), the pair by grid_load_pair.  The prefetch discipline is that kernel's:
// the records -- primal and tangent -- and the pair of step n - 1 are fetched before step n computes and rotated in behind it,
// the slot one step further ahead, everything issued before the loop is complete before the loop is entered, and the node of
// the next observation is held in a register.  Per step: predict_block / jvp_predict_block re-evaluate pred[n + 1] and its
// tangent from filt[n], jvp_markov_step runs on the carry before fenrir_markov_step overwrites it, and where node n is observed
// jvp_observe runs before fenrir_observe_scalar -- node 0 and node N like any other.  A y term the value drops (|w| <= 1e-8)
// adds nothing to the derivative (jvp_update's rule).
// No atomics: every lane writes its block's dacc to dpart[blk * B K + item], the k = 0 item writes acc to part[blk * B + b], and
// magi_sum_kernel adds them in block order; with one block part / dpart are value / dvalue themselves.
template <int P>
__global__ void __launch_bounds__(64) fenrir_grid_jvp_bwd_kernel(SolveArgs a, DaltonObs o, GridArgs g, int K,
                                                                 const double* __restrict__ dmean, const double* __restrict__ dvar,
                                                                 double* __restrict__ part, double* __restrict__ dpart) {
    const long long n_items = (long long)a.B * K;
    const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_items * a.D) return;
    const int blk = (int)(l / n_items), item = (int)(l - (long long)blk * n_items);
    const int b = item / K, k = item - b * K;
    const size_t B = (size_t)a.B, BK = (size_t)n_items;
    double bm[P], bS[P][P], dbm[P], dbS[P][P];
    load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, a.N, blk, b, bm, bS);       // terminal point (fenrir.py:186-188)
    load_moments<P, RK_LAYOUT_BATCH_MINOR>(dmean, dvar, BK, a.D, a.N, blk, item, dbm, dbS);
    double acc = 0.0, dacc = 0.0;
    int i = o.n_obs - 1;
    int obs_node = i >= 0 ? o.obs_ind[i] : -1;                              // node of observation i; -1: none left
    auto observe = [&]() {
        jvp_observe<P>(o, (size_t)i * a.D + blk, bm, bS, dbm, dbS, dacc);   // (before the primal update of the carry)
        fenrir_observe_scalar<P>(o, (size_t)i * a.D + blk, bm, bS, acc);
        --i;
        obs_node = i >= 0 ? o.obs_ind[i] : -1;
        asm volatile("" : "+v"(obs_node));                                  // waited for here, on the rare path, not behind a prefetch
    };
    if (obs_node >= a.N) observe();                                         // fenrir.py:189-209

    double mf[P], Sf[P][P], dmf[P], dSf[P][P], Q[P][P], R[P][P];
    load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, a.N - 1, blk, b, mf, Sf);
    load_moments<P, RK_LAYOUT_BATCH_MINOR>(dmean, dvar, BK, a.D, a.N - 1, blk, item, dmf, dSf);
    grid_load_pair<P>(g, a.B, a.D, grid_slot(g, a.N - 1), blk, b, Q, R);
    int s_next = a.N >= 2 ? g.slot[a.N - 2] : 0;              // slot of step n - 1 as the table has it: clamped where it is used
    // every load so far is complete before the loop is entered, so that no step waits for its own prefetch (grid_fwd_kernel)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    for (int n = a.N - 1; n >= 0; --n) {
        const bool more = n >= 1;
        double mfn[P], Sfn[P][P], dmfn[P], dSfn[P][P], Qn[P][P], Rn[P][P];
        int s_after = 0;
        if (more) {
            load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, n - 1, blk, b, mfn, Sfn);
            load_moments<P, RK_LAYOUT_BATCH_MINOR>(dmean, dvar, BK, a.D, n - 1, blk, item, dmfn, dSfn);
            grid_load_pair<P>(g, a.B, a.D, grid_clamp(g, s_next), blk, b, Qn, Rn);
            if (n >= 2) s_after = g.slot[n - 2];
        }
        double mp[P], Sp[P][P], dmp[P], dSp[P][P], G[P][P];
        predict_block<P>(Q, R, mf, Sf, mp, Sp);                             // pred[n + 1] from filt[n] and the pair of step n
        jvp_predict_block<P>(Q, dmf, dSf, dmp, dSp);
        jvp_markov_step<P>(Q, Sf, mp, Sp, dmf, dSf, dmp, dSp, bm, bS, dbm, dbS);              // (the carry is still step n + 1's)
        fenrir_markov_step<P>(Q, mf, Sf, mp, Sp, bm, bS, G);
        if (obs_node == n) observe();                                       // fenrir.py:155-170 (the same in every lane of the wave)
        if (more) {
            asm volatile("" : "+v"(s_after));                 // the fetched slot stays in a vector register until here (grid_fwd_kernel)
            s_next = s_after;
#pragma unroll
            for (int r = 0; r < P; ++r) {
                mf[r] = mfn[r];
                dmf[r] = dmfn[r];
#pragma unroll
                for (int c = 0; c < P; ++c) {
                    Sf[r][c] = Sfn[r][c];
                    dSf[r][c] = dSfn[r][c];
                    Q[r][c] = Qn[r][c];
                    R[r][c] = Rn[r][c];
                }
            }
        }
    }
    dpart[(size_t)blk * BK + item] = dacc;
    if (k == 0) part[(size_t)blk * B + b] = acc;
}

// The hyper form, a sibling of the kernel above with its lanes, prefetch discipline and exits,
// written out: as one `__device__ __forceinline__` body under `if constexpr (HYPER)` behind two one-line kernels the pair kept its
// registers (212 / 428 and 218 / 436), scratch 0 and fp64 instruction counts and ran 2.0 % (the kernel above) and 0.3 % (this one)
// slower than the parent's, whose three block medians lie within 0.2 % (profiles/grad_shared_times.txt, section 7 (26)).  The
// lane keeps its block's two rates, l. of log sigma and w. of the observation variances' log-scale; the re-evaluated pred[n + 1]
// has Sigma.- = Q Sigma._f Q^T + 2 l. R (jvp_predict_scale), and an observation has Omega. = w. Omega (jvp_observe_rate).
template <int P>
__global__ void __launch_bounds__(64) fenrir_grid_jvp_bwd_hyper_kernel(SolveArgs a, DaltonObs o, GridArgs g, int K, JvpHyper hy,
                                                                       const double* __restrict__ dmean,
                                                                       const double* __restrict__ dvar, double* __restrict__ part,
                                                                       double* __restrict__ dpart) {
    const long long n_items = (long long)a.B * K;
    const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_items * a.D) return;
    const int blk = (int)(l / n_items), item = (int)(l - (long long)blk * n_items);
    const int b = item / K, k = item - b * K;
    const size_t B = (size_t)a.B, BK = (size_t)n_items;
    const double dls = hyper_rate(hy.dlsig, hy.dlsig_b, a.D, k, blk, a.B, b);
    const double dlo = hyper_rate(hy.dlobs, hy.dlobs_b, a.D, k, blk, a.B, b);
    double bm[P], bS[P][P], dbm[P], dbS[P][P];
    load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, a.N, blk, b, bm, bS);       // terminal point (fenrir.py:186-188)
    load_moments<P, RK_LAYOUT_BATCH_MINOR>(dmean, dvar, BK, a.D, a.N, blk, item, dbm, dbS);
    double acc = 0.0, dacc = 0.0;
    int i = o.n_obs - 1;
    int obs_node = i >= 0 ? o.obs_ind[i] : -1;                              // node of observation i; -1: none left
    auto observe = [&]() {
        jvp_observe_rate<P>(o, (size_t)i * a.D + blk, dlo, bm, bS, dbm, dbS, dacc);           // (before the primal update of the carry)
        fenrir_observe_scalar<P>(o, (size_t)i * a.D + blk, bm, bS, acc);
        --i;
        obs_node = i >= 0 ? o.obs_ind[i] : -1;
        asm volatile("" : "+v"(obs_node));                                  // waited for here, on the rare path, not behind a prefetch
    };
    if (obs_node >= a.N) observe();                                         // fenrir.py:189-209

    double mf[P], Sf[P][P], dmf[P], dSf[P][P], Q[P][P], R[P][P];
    load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, a.N - 1, blk, b, mf, Sf);
    load_moments<P, RK_LAYOUT_BATCH_MINOR>(dmean, dvar, BK, a.D, a.N - 1, blk, item, dmf, dSf);
    grid_load_pair<P>(g, a.B, a.D, grid_slot(g, a.N - 1), blk, b, Q, R);
    int s_next = a.N >= 2 ? g.slot[a.N - 2] : 0;              // slot of step n - 1 as the table has it: clamped where it is used
    // every load so far is complete before the loop is entered, so that no step waits for its own prefetch (grid_fwd_kernel)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    for (int n = a.N - 1; n >= 0; --n) {
        const bool more = n >= 1;
        double mfn[P], Sfn[P][P], dmfn[P], dSfn[P][P], Qn[P][P], Rn[P][P];
        int s_after = 0;
        if (more) {
            load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, n - 1, blk, b, mfn, Sfn);
            load_moments<P, RK_LAYOUT_BATCH_MINOR>(dmean, dvar, BK, a.D, n - 1, blk, item, dmfn, dSfn);
            grid_load_pair<P>(g, a.B, a.D, grid_clamp(g, s_next), blk, b, Qn, Rn);
            if (n >= 2) s_after = g.slot[n - 2];
        }
        double mp[P], Sp[P][P], dmp[P], dSp[P][P], G[P][P];
        predict_block<P>(Q, R, mf, Sf, mp, Sp);                             // pred[n + 1] from filt[n] and the pair of step n
        jvp_predict_block<P>(Q, dmf, dSf, dmp, dSp);
        jvp_predict_scale<P>(R, dls, dSp);
        jvp_markov_step<P>(Q, Sf, mp, Sp, dmf, dSf, dmp, dSp, bm, bS, dbm, dbS);              // (the carry is still step n + 1's)
        fenrir_markov_step<P>(Q, mf, Sf, mp, Sp, bm, bS, G);
        if (obs_node == n) observe();                                       // fenrir.py:155-170 (the same in every lane of the wave)
        if (more) {
            asm volatile("" : "+v"(s_after));                 // the fetched slot stays in a vector register until here (grid_fwd_kernel)
            s_next = s_after;
#pragma unroll
            for (int r = 0; r < P; ++r) {
                mf[r] = mfn[r];
                dmf[r] = dmfn[r];
#pragma unroll
                for (int c = 0; c < P; ++c) {
                    Sf[r][c] = Sfn[r][c];
                    dSf[r][c] = dSfn[r][c];
                    Q[r][c] = Qn[r][c];
                    R[r][c] = Rn[r][c];
                }
            }
        }
    }
    dpart[(size_t)blk * BK + item] = dacc;
    if (k == 0) part[(size_t)blk * B + b] = acc;
}

// ---- dispatch ---------------------------------------------------------------------------------------------------
// The rule an instance ships by: the forward kernel uses no more scratch than grid_fwd_kernel<RHS, P,
// ITG>, the backward kernel no more than fenrir_grid_bwd_kernel<P, false, 1>.  profiles/fenrir_grad_code_objects.txt has every
// instance next to its yardstick (scripts/fenrir_grad_code_objects.py).  What is built is what jvp_interrogate's register set gave
// DALTON: n_bstate 2 and 3 of FitzHugh-Nagumo and Lorenz63 (D P^2 <= 27).
constexpr int FENRIR_GRAD_PMIN = GRAD_PMIN, FENRIR_GRAD_PMAX = 3;

// Is this call served?  grid_entry.hpp's grad_check with this entry's item count (the backward kernel has one lane per block and
// item), rule for a user right-hand side and range.
static int fenrir_grad_check(const rk_solve_cfg* c, int n_bobs, int n_dir) {
    return grad_check("fenrir_grid_jvp", c, n_bobs, n_dir, true, user_fenrir_grad_check, FENRIR_GRAD_PMAX);
}

// The hyper kernels ship by the same rule with their non-hyper siblings as yardsticks.  All fourteen
// pass without scratch (profiles/hyper_grad_code_objects.txt), so rk_fenrir_grid_jvp_hyper serves what rk_fenrir_grid_jvp serves.

// bytes of the tangent records of n_dir directions: dmean (N+1, D, P, B n_dir) then dvar (N+1, D, P, P, B n_dir)
static size_t fenrir_grad_ws_bytes(const rk_solve_cfg* c, int n_dir) {
    return sizeof(double) * (size_t)(c->n_steps + 1) * c->n_block * ((size_t)c->n_bstate + (size_t)c->n_bstate * c->n_bstate) *
           (size_t)c->n_traj * (size_t)n_dir;
}

// `hy`: null for rk_fenrir_grid_jvp, the hyper directions for rk_fenrir_grid_jvp_hyper (the hyper kernels)
static int fenrir_grid_jvp_forward(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& ga, const JvpDirs& dir,
                                   const JvpHyper* hy, double* dmean, double* dvar) {
    const auto user = [&] { return user_fenrir_grad(h, c, a, ga, dir, hy, a.B * dir.K, dmean, dvar); };
    return launch_by_rhs(c, a, user, [&](auto rhs) {
        using RHS = decltype(rhs);
        if constexpr (grad_has_rhs<RHS>()) {
            const LaunchGeom g = dalton_lane_geom(a.B * dir.K, false);      // 64 (trajectory, direction) items per wave
            if (hy)
                return launch_fwd_instance<FENRIR_GRAD_PMIN, FENRIR_GRAD_PMAX, RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(
                    h, c, "fenrir_grid_jvp_fwd_hyper_kernel", "fenrir_grid_jvp_hyper", [&](auto P, auto I) {
                        hipLaunchKernelGGL((fenrir_grid_jvp_fwd_hyper_kernel<RHS, P, I>), g.grid, g.block, 0, h->stream, a, ga, dir, *hy,
                                           dmean, dvar);
                    });
            return launch_fwd_instance<FENRIR_GRAD_PMIN, FENRIR_GRAD_PMAX, RK_INTERROGATE_RODEO, RK_INTERROGATE_KRAMER>(
                h, c, "fenrir_grid_jvp_fwd_kernel", "fenrir_grid_jvp", [&](auto P, auto I) {
                    hipLaunchKernelGGL((fenrir_grid_jvp_fwd_kernel<RHS, P, I>), g.grid, g.block, 0, h->stream, a, ga, dir, dmean, dvar);
                });
        } else {
            return (int)RK_ERR_UNSUPPORTED;                                 // (fenrir_grad_check has refused it)
        }
    });
}

static int fenrir_grid_jvp_backward(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, const GridArgs& ga,
                                    int K, const JvpHyper* hy, const double* dmean, const double* dvar, double* part, double* dpart) {
    const LaunchGeom g = bwd_lane_geom(a.B * K, a.D);
    LaunchTimer t(h, hy ? "fenrir_grid_jvp_bwd_hyper_kernel" : "fenrir_grid_jvp_bwd_kernel");
    const bool ok = dispatch_int<FENRIR_GRAD_PMIN, FENRIR_GRAD_PMAX>(c->n_bstate, [&](auto P) {
        if (hy)
            hipLaunchKernelGGL((fenrir_grid_jvp_bwd_hyper_kernel<P>), g.grid, g.block, 0, h->stream, a, o, ga, K, *hy, dmean, dvar, part,
                               dpart);
        else
            hipLaunchKernelGGL((fenrir_grid_jvp_bwd_kernel<P>), g.grid, g.block, 0, h->stream, a, o, ga, K, dmean, dvar, part, dpart);
    });
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "fenrir_grid_jvp: no backward kernel for n_bstate %d", c->n_bstate);
    t.stop();
    RK_HIP(hipGetLastError());
    return RK_OK;
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_fenrir_grid_jvp_workspace_bytes(const rk_solve_cfg* c, int32_t n_dir, size_t* bytes) {
    RK_REQUIRE(c && bytes, RK_ERR_INVALID, "rk_fenrir_grid_jvp_workspace_bytes: null argument");
    const int rc = grid_sizes_check("fenrir_grid_jvp", c);
    if (rc) return rc;
    RK_REQUIRE(n_dir >= 1, RK_ERR_INVALID, "fenrir_grid_jvp: n_dir must be at least 1, got %d", n_dir);
    *bytes = fenrir_grad_ws_bytes(c, n_dir);
    return RK_OK;
}

// the body of rk_fenrir_grid_jvp (hy null) and rk_fenrir_grid_jvp_hyper
static int fenrir_grid_jvp_run(const char* who, rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out,
                               const double* obs, const double* obs_weight, const double* obs_var, const int32_t* obs_node,
                               int32_t n_obs, int32_t n_bobs, const rk_grid_in* g, const JvpDirs& dir, const JvpHyper* hy,
                               void* workspace, double* value, double* dvalue) {
    const int n_dir = dir.K;
    RK_REQUIRE(c, RK_ERR_INVALID, "%s: null cfg", who);
    int rc = fenrir_grad_check(c, n_bobs, n_dir);                   // (the configuration alone, before anything else is looked at)
    if (rc) return rc;
    RK_REQUIRE(h && out && g && workspace && value && dvalue, RK_ERR_INVALID, "%s: null argument", who);
    GridArgs ga;
    rc = grid_args(who, g, ga);
    if (rc) return rc;
    rc = check_cfg(c, in);
    if (rc) return rc;
    RK_REQUIRE(n_obs >= 0 && (n_obs == 0 || (obs && obs_weight && obs_var && obs_node)), RK_ERR_INVALID,
               "%s: null observation array or n_obs < 0", who);
    rc = grid_out_check(who, out, RK_MODE_MV);
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    SolveArgs a;
    make_args(c, in, out, a);
    const DaltonObs o{obs, obs_weight, obs_var, obs_node, n_obs};
    const size_t BK = (size_t)a.B * (size_t)n_dir;
    double* dmean = (double*)workspace;
    double* dvar = dmean + (size_t)(a.N + 1) * a.D * c->n_bstate * BK;
    rc = fenrir_grid_jvp_forward(h, c, a, ga, dir, hy, dmean, dvar);
    if (rc) return rc;
    double *part = value, *dpart = dvalue;                          // one block: the lanes write value / dvalue themselves
    if (a.D > 1) {
        rc = lane_scratch(h, sizeof(double) * (size_t)a.D * ((size_t)a.B + BK), &part);
        if (rc) return rc;
        dpart = part + (size_t)a.D * a.B;
    }
    rc = fenrir_grid_jvp_backward(h, c, a, o, ga, n_dir, hy, dmean, dvar, part, dpart);
    if (rc || a.D == 1) return rc;
    rc = launch_block_sum(h, part, a.B, a.D, value);                // block order, B and then B K sums: two calls give the same bits
    if (rc) return rc;
    return launch_block_sum(h, dpart, (int)BK, a.D, dvalue);
}

int rk_fenrir_grid_jvp(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, const double* obs,
                       const double* obs_weight, const double* obs_var, const int32_t* obs_node, int32_t n_obs, int32_t n_bobs,
                       const rk_grid_in* g, int32_t n_dir, const double* dtheta, int32_t dtheta_batched, const double* dinit,
                       int32_t dinit_batched, void* workspace, double* value, double* dvalue) {
    const JvpDirs dir{dtheta, dinit, dtheta_batched != 0, dinit_batched != 0, n_dir};
    return fenrir_grid_jvp_run("rk_fenrir_grid_jvp (fenrir_grid_jvp)", h, c, in, out, obs, obs_weight, obs_var, obs_node, n_obs, n_bobs,
                               g, dir, nullptr, workspace, value, dvalue);
}

int rk_fenrir_grid_jvp_hyper(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, const double* obs,
                             const double* obs_weight, const double* obs_var, const int32_t* obs_node, int32_t n_obs, int32_t n_bobs,
                             const rk_grid_in* g, int32_t n_dir, const double* dtheta, int32_t dtheta_batched, const double* dinit,
                             int32_t dinit_batched, const double* dlog_sigma, int32_t dlog_sigma_batched, const double* dlog_obs_var,
                             int32_t dlog_obs_var_batched, void* workspace, double* value, double* dvalue) {
    const JvpDirs dir{dtheta, dinit, dtheta_batched != 0, dinit_batched != 0, n_dir};
    const JvpHyper hy{dlog_sigma, dlog_obs_var, dlog_sigma_batched != 0, dlog_obs_var_batched != 0};
    return fenrir_grid_jvp_run("rk_fenrir_grid_jvp_hyper (fenrir_grid_jvp)", h, c, in, out, obs, obs_weight, obs_var, obs_node, n_obs,
                               n_bobs, g, dir, &hy, workspace, value, dvalue);
}

}  // extern "C"
