// fenrir_grid / fenrir.solve_mv_grid (an addition): Fenrir on a non-uniform grid shared by the batch,
// every observation on a node -- the backward Markov-chain filter with every step's own prior pair, and the host side of
// rk_fenrir_grid_loglik / rk_fenrir_grid_solve_mv.  One route: the lanes on batch-minor records -- grid.hip's own forward launch
// (grid_fwd_kernel, one lane per trajectory; Fenrir's forward pass is free of data), then fenrir_grid_bwd_kernel, one lane per
// (block, trajectory), and for the solver fenrir.hip's own smoothing sweep (fenrir_smooth_kernel), which reads only the stored
// backward filter and knows nothing of step lengths.  Standard form, n_bmeas = 1.  Ahead-of-time code only: the backward pass
// has no right-hand side.  The pieces of the configuration check, the grid's staging and the test of the output pointers are
// grid_entry.hpp's.
#include "common.hpp"
#include "kalman_small.hpp"
#include "solve_args.hpp"
#include "solve_paths.hpp"
#include "grid_entry.hpp"
#include "grid_kernels.hpp"
#include "fenrir_kernels.hpp"
#include "records.hpp"

namespace rk {

// ---- backward filter (src/rodeo/inference/fenrir.py:86-259 with (Q_n, R_n) = (q, r)[slot[n]] in place of the one pair) ----
// fenrir_bwd_kernel's recursion (fenrir.hip) on the records grid_fwd_kernel wrote: the carry starts at filt[N]; for n = N-1 .. 0
// pred[n+1] is re-evaluated from filt[n] with the pair of step n (the forward pass stores no predictions), fenrir_markov_step
// runs with Q_n as the transition matrix, and the step conditions on y where node n is observed -- node 0 like any other.
// obs_ind holds the NODE of every observation, strictly increasing in 0 .. N.
//
// filt[n-1] and the pair of step n-1 are fetched before step n computes and rotated in behind it (bwd_walk, SlotPrior::fetch); the
// slot of step n-2 is fetched with them and first looked at (clamped) one step later, where its pair is fetched, so no step
// waits for a load that depends on another load.  A sibling of bwd_walk, not an edit of it: that walk stops at node 1, and its
// instances stay the code they are.  The node of the next observation is held in a register and fetched again only behind an
// observation: the steps between two observations issue no load besides the prefetches.
//
// No atomics: a lane writes its block's sum to part[blk * B + b] (with one block, part is logdens itself) and magi_sum_kernel
// adds a trajectory's sums in block order (launch_block_sum).  With STORE the backward filter's predicted and updated moments of every node and the Markov
// weights A_n go to `states`, one FenrirItem per (node, block), batch-minor: what fenrir_smooth_kernel reads.
template <int P, bool STORE, int MO>
__global__ void __launch_bounds__(64) fenrir_grid_bwd_kernel(SolveArgs a, DaltonObs o, GridArgs g, double* __restrict__ part,
                                                             double* __restrict__ states) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= a.B * a.D) return;
    int blk, b;
    record_lane<RK_LAYOUT_BATCH_MINOR>(l, a.B, a.D, blk, b);
    const size_t B = (size_t)a.B;
    double bm[P], bS[P][P];
    load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, a.N, blk, b, bm, bS);       // terminal point (fenrir.py:186-188)
    double acc = 0.0;
    int i = o.n_obs - 1;
    int obs_node = i >= 0 ? o.obs_ind[i] : -1;                              // node of observation i; -1: none left
    // conditioning on observation i: forecast (standard.py:333-335) + log-density + update (standard.py:93-102)
    auto observe = [&](double (&m)[P], double (&S)[P][P]) {
        if constexpr (MO == 1) fenrir_observe_scalar<P>(o, (size_t)i * a.D + blk, m, S, acc);
        else dalton_observe<P, MO>(o, (size_t)i * a.D + blk, m, S, acc);
        --i;
        obs_node = i >= 0 ? o.obs_ind[i] : -1;
        asm volatile("" : "+v"(obs_node));                                  // waited for here, on the rare path, not behind a prefetch
    };
    constexpr FenrirItem IT(P);
    auto keep = [&](int n, int off, const double (&m)[P], const double (&S)[P][P]) {
        double* q = states + (((size_t)n * a.D + blk) * IT.width + off) * B + b;
#pragma unroll
        for (int r = 0; r < P; ++r) {
            q[(size_t)r * B] = m[r];
#pragma unroll
            for (int c = 0; c < P; ++c) q[(size_t)(P + r * P + c) * B] = S[r][c];
        }
    };
    if constexpr (STORE) keep(a.N, IT.pred, bm, bS);                        // "prediction" at N = the terminal point
    if (obs_node >= a.N) observe(bm, bS);                                   // fenrir.py:189-209
    if constexpr (STORE) keep(a.N, IT.filt, bm, bS);

    double mf[P], Sf[P][P], Q[P][P], R[P][P];
    load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, a.N - 1, blk, b, mf, Sf);
    grid_load_pair<P>(g, a.B, a.D, grid_slot(g, a.N - 1), blk, b, Q, R);
    int s_next = a.N >= 2 ? g.slot[a.N - 2] : 0;              // slot of step n - 1 as the table has it: clamped where it is used
    // every load so far is complete before the loop is entered, so that no step waits for its own prefetch (grid_fwd_kernel)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    for (int n = a.N - 1; n >= 0; --n) {
        const bool more = n >= 1;
        double mfn[P], Sfn[P][P], Qn[P][P], Rn[P][P];
        int s_after = 0;
        if (more) {
            load_moments<P, RK_LAYOUT_BATCH_MINOR>(a.mean, a.var, B, a.D, n - 1, blk, b, mfn, Sfn);
            grid_load_pair<P>(g, a.B, a.D, grid_clamp(g, s_next), blk, b, Qn, Rn);
            if (n >= 2) s_after = g.slot[n - 2];
        }
        double mp[P], Sp[P][P], G[P][P];
        predict_block<P>(Q, R, mf, Sf, mp, Sp);                             // pred[n + 1] from filt[n] and the pair of step n
        fenrir_markov_step<P>(Q, mf, Sf, mp, Sp, bm, bS, G);
        if constexpr (STORE) {
            keep(n, IT.pred, bm, bS);
            double* q = states + (((size_t)n * a.D + blk) * IT.width + IT.A) * B + b;
#pragma unroll
            for (int r = 0; r < P; ++r)
#pragma unroll
                for (int c = 0; c < P; ++c) q[(size_t)(r * P + c) * B] = G[r][c];
        }
        if (obs_node == n) observe(bm, bS);                                 // fenrir.py:155-170 (the same in every lane of the wave)
        if constexpr (STORE) keep(n, IT.filt, bm, bS);
        if (more) {
            asm volatile("" : "+v"(s_after));                 // the fetched slot stays in a vector register until here (grid_fwd_kernel)
            s_next = s_after;
#pragma unroll
            for (int r = 0; r < P; ++r) {
                mf[r] = mfn[r];
#pragma unroll
                for (int c = 0; c < P; ++c) {
                    Sf[r][c] = Sfn[r][c];
                    Q[r][c] = Qn[r][c];
                    R[r][c] = Rn[r][c];
                }
            }
        }
    }
    if (part) part[(size_t)blk * B + b] = acc;
}

// ---- dispatch ---------------------------------------------------------------------------------------------------
// The rule an instance ships by (DESIGN.md section 7 (17), (16)'s rule): no more scratch than the larger of
// fenrir_bwd_kernel<P, STORE, MO> and grid_bwd_mv_kernel<P>.  profiles/fenrir_grid_code_objects.txt has all 30 instances next
// to the two (scripts/fenrir_grid_code_objects.py): all 30 keep the rule -- none up to n_bstate 4 uses scratch, at 5 and 6 they
// need less than grid_bwd_mv_kernel, which holds the same two pairs and two records -- so none is left out.

constexpr int FENRIR_GRID_PMIN = 2, FENRIR_GRID_PMAX = 6, FENRIR_GRID_PMAX_THREE_BLOCKS = 5;

// Is this call served?  Decided on the configuration and n_bobs alone: RK_OK, RK_ERR_INVALID or RK_ERR_UNSUPPORTED.
// grid_check's pattern (grid.hip; the pieces are grid_entry.hpp's) with fenrir's n_bobs.
static int fenrir_grid_check(const rk_solve_cfg* c, int n_bobs) {
    int rc = grid_sizes_check("fenrir_grid", c);
    if (rc) return rc;
    rc = grid_served_check({"fenrir_grid", GRID_RECORDS, RK_INTERROGATE_CHKREBTII, nullptr, FENRIR_GRID_PMIN, FENRIR_GRID_PMAX,
                            FENRIR_GRID_PMAX_THREE_BLOCKS}, c);
    if (rc) return rc;
    RK_REQUIRE(n_bobs >= 1 && n_bobs <= 3, RK_ERR_UNSUPPORTED, "fenrir_grid: n_bobs in 1..3, got %d", n_bobs);
    return grid_rhs_check("fenrir_grid", c, "grid");                // (the forward pass is the grid solver's: its rule, our name)
}

template <bool STORE>
static int launch_fenrir_grid_bwd(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, const GridArgs& ga,
                                  int n_bobs, double* part, double* states) {
    const LaunchGeom g = bwd_lane_geom(a.B, a.D);
    bool ok = false;
    LaunchTimer t(h, "fenrir_grid_bwd_kernel");
    dispatch_int<FENRIR_GRID_PMIN, FENRIR_GRID_PMAX>(c->n_bstate, [&](auto P) {
        dispatch_int<1, 3>(n_bobs, [&](auto M) {
            hipLaunchKernelGGL((fenrir_grid_bwd_kernel<P, STORE, M>), g.grid, g.block, 0, h->stream, a, o, ga, part, states);
            ok = true;
        });
    });
    RK_REQUIRE(ok, RK_ERR_UNSUPPORTED, "fenrir_grid: no backward kernel for n_bstate %d, n_bobs %d", c->n_bstate, n_bobs);
    t.stop();
    RK_HIP(hipGetLastError());
    return RK_OK;
}

// what both entries do once the configuration is accepted: the pointers of a served call (rk_solve_grid's rule for the grid and
// the records, dalton_grid's for the observations: an empty set needs no arrays), then the forward pass of rk_solve_grid
static int fenrir_grid_forward(const char* who, rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out,
                               const double* obs, const double* obs_weight, const double* obs_var, const int32_t* obs_node, int n_obs,
                               const rk_grid_in* g, SolveArgs& a, DaltonObs& o, GridArgs& ga) {
    int rc = grid_args(who, g, ga);
    if (rc) return rc;
    rc = check_cfg(c, in);
    if (rc) return rc;
    RK_REQUIRE(n_obs >= 0 && (n_obs == 0 || (obs && obs_weight && obs_var && obs_node)), RK_ERR_INVALID,
               "%s: null observation array or n_obs < 0", who);
    rc = grid_out_check(who, out, RK_MODE_MV);
    if (rc) return rc;
    rc = begin_solve(h);
    if (rc) return rc;
    make_args(c, in, out, a);
    o = DaltonObs{obs, obs_weight, obs_var, obs_node, n_obs};
    return launch_grid_forward(h, c, a, ga);
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_fenrir_grid_loglik(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, const double* obs,
                          const double* obs_weight, const double* obs_var, const int32_t* obs_node, int32_t n_obs, int32_t n_bobs,
                          const rk_grid_in* g, double* logdens) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_fenrir_grid_loglik (fenrir_grid): null cfg");
    int rc = fenrir_grid_check(c, n_bobs);                 // (the configuration alone, before anything else is looked at)
    if (rc) return rc;
    RK_REQUIRE(h && out && g && logdens, RK_ERR_INVALID, "rk_fenrir_grid_loglik (fenrir_grid): null argument");
    SolveArgs a;
    DaltonObs o;
    GridArgs ga;
    rc = fenrir_grid_forward("rk_fenrir_grid_loglik (fenrir_grid)", h, c, in, out, obs, obs_weight, obs_var, obs_node, n_obs, g, a, o, ga);
    if (rc) return rc;
    double* part = logdens;                                         // one block: the lanes write logdens themselves
    if (a.D > 1) {
        rc = lane_scratch(h, sizeof(double) * (size_t)a.B * (size_t)a.D, &part);
        if (rc) return rc;
    }
    rc = launch_fenrir_grid_bwd<false>(h, c, a, o, ga, n_bobs, part, nullptr);
    if (rc || a.D == 1) return rc;
    return launch_block_sum(h, part, a.B, a.D, logdens);
}

int rk_fenrir_grid_solve_mv(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, const double* obs,
                            const double* obs_weight, const double* obs_var, const int32_t* obs_node, int32_t n_obs, int32_t n_bobs,
                            const rk_grid_in* g, void* workspace) {
    RK_REQUIRE(c, RK_ERR_INVALID, "rk_fenrir_grid_solve_mv (fenrir_grid): null cfg");
    int rc = fenrir_grid_check(c, n_bobs);
    if (rc) return rc;
    RK_REQUIRE(h && out && g && workspace, RK_ERR_INVALID, "rk_fenrir_grid_solve_mv (fenrir_grid): null argument");
    SolveArgs a;
    DaltonObs o;
    GridArgs ga;
    rc = fenrir_grid_forward("rk_fenrir_grid_solve_mv (fenrir_grid)", h, c, in, out, obs, obs_weight, obs_var, obs_node, n_obs, g, a, o, ga);
    if (rc) return rc;
    rc = launch_fenrir_grid_bwd<true>(h, c, a, o, ga, n_bobs, nullptr, (double*)workspace);
    if (rc) return rc;
    return launch_fenrir_smooth_lanes(h, c, a, (const double*)workspace);
}

}  // extern "C"
