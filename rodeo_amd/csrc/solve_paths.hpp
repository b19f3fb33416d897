// Host-side solver API shared by the translation units of librodeo_kalman.so (host code only, not part of the hiprtc set):
// the functions one .hip file calls in another, the one rule that picks a configuration's device path, and the helpers
// that turn run-time sizes / ids into template instances at the launch sites.  What the entries on the non-uniform grid share on
// top of it -- the pieces of their configuration checks, the grid's staging, the launch patterns -- is in grid_entry.hpp.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include "common.hpp"
#include "rhs.hpp"
#include "solve_args.hpp"

namespace rk {

struct DenseItgArgs;
struct SimLogpost;
struct DaltonObs;
struct DaltonAt;
struct FenrirAt;
struct GridArgs;

// ---- lane-per-trajectory solver (solve_small.hip): helpers that DALTON (dalton.hip) and Fenrir (fenrir.hip) share ------
int check_cfg(const rk_solve_cfg* c, const rk_solve_in* in);
int make_args(const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, SolveArgs& a);
int begin_solve(rk_handle h);
int small_backward_pass(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, int mode);

// ---- dense large-block path (solve_dense.hip) ----------------------------------------------------------------------
bool dense_supported(const rk_solve_cfg* c, int mode);
int dense_check(const rk_solve_cfg* c, const rk_solve_in* in, int mode);
int dense_solve(rk_handle h, const rk_solve_cfg* c, const rk_solve_in* in, const rk_solve_out* out, int mode);
size_t dense_ws_bytes(const rk_solve_cfg* c, int mode);

// ---- user-supplied right-hand sides (rhs_jit.hip) ------------------------------------------------------------------
// Kernel kinds of the hiprtc builds: the row index of rhs_jit.hip's table and a field of its cache key.  Do not renumber.
enum JitKind : int {
    JIT_FWD = 0,              // fwd_kernel<.., false>
    JIT_FWD_STORE_PRED = 1,   // fwd_kernel<.., true>
    JIT_ITG = 2,              // interrogate_kernel
    JIT_TILE3 = 3,            // fwd_tile3_kernel
    JIT_TILE4 = 4,            // fwd_tile4_kernel
    JIT_TILEN = 5,            // fwd_tilen_kernel
    JIT_SQRT = 6,             // fwd_sqrt_kernel
    JIT_FWD_M = 7,            // fwd_kernel_m<.., false>   (n_bmeas > 1)
    JIT_FWD_M_STORE_PRED = 8, // fwd_kernel_m<.., true>
    JIT_DENSE_ITG = 9,        // dense_interrogate_kernel
    JIT_ITG_M = 10,           // interrogate_kernel_m     (n_bmeas > 1)
    JIT_DALTON = 11,          // dalton_fwd_kernel<.., false> (log-likelihood)
    JIT_DALTON_STORE = 12,    // dalton_fwd_kernel<.., true>  (joint filter's moments)
    JIT_DALTON_TILE3 = 13,    // dalton_fwd_tile3_kernel<.., false> (log-likelihood on the p = 3 tiles)
    JIT_DALTON_TILE3_STORE = 14,  // dalton_fwd_tile3_kernel<.., true> (RK_LAYOUT_TILE3 records)
    JIT_DALTONNG = 15,        // daltonng_fwd_kernel<.., false> (joint filter's moments)
    JIT_DALTONNG_BOTH = 16,   // daltonng_fwd_kernel<.., true>  (joint filter and the filter on Z alone)
    JIT_DALTONNG_OBS = 17,    // daltonng_obs_kernel (logy_x and the final sum; no right-hand side)
    JIT_DALTON_AT = 18,       // dalton_fwd_at_kernel (dalton_at's log-likelihood)
    JIT_DALTON_AT_TILE3 = 19, // dalton_fwd_at_tile3_kernel (dalton_at's log-likelihood on the p = 3 tiles)
    JIT_EVIDENCE = 20,        // evidence_kernel (solve_evidence, standard form on the lanes)
    JIT_EVIDENCE_TILE3 = 21,  // evidence_tile3_kernel (solve_evidence on the p = 3 tiles)
    JIT_EVIDENCE_SQRT = 22,   // evidence_sqrt_kernel (solve_evidence, square-root form)
    JIT_DYNAMIC = 23,         // dynamic_fwd_kernel (solve_mv_dynamic / solve_sim_dynamic, the forward lanes)
    JIT_GRID = 24,            // grid_fwd_kernel (solve_mv_grid / solve_sim_grid, the forward lanes)
    JIT_DALTON_GRID = 25,     // dalton_grid_fwd_kernel<.., false> (dalton_grid's log-likelihood)
    JIT_DALTON_GRID_STORE = 26,  // dalton_grid_fwd_kernel<.., true> (dalton.solve_mv_grid / solve_sim_grid, the joint filter's moments)
    JIT_GRID_EVIDENCE = 27,   // grid_evidence_kernel (solve_evidence_grid)
    JIT_GRID_DYNAMIC = 28,    // grid_dynamic_fwd_kernel (solve_mv_dynamic_grid / solve_sim_dynamic_grid, the forward lanes)
    JIT_DALTONNG_GRID = 29,   // daltonng_grid_fwd_kernel<.., false> (solve_mv_nn_grid, the joint filter's moments)
    JIT_DALTONNG_GRID_BOTH = 30,  // daltonng_grid_fwd_kernel<.., true> (daltonng_grid, the joint filter and the filter on Z alone)
    JIT_DALTON_GRAD = 31,     // dalton_grid_jvp_kernel (dalton_grid_jvp: value and directional derivatives; a gradient-kind source)
    JIT_FENRIR_GRAD = 32,     // fenrir_grid_jvp_fwd_kernel (fenrir_grid_jvp: the forward tangent filter; a gradient-kind source)
    JIT_DALTON_GRAD_HYPER = 33,  // dalton_grid_jvp_hyper_kernel (the same with log sigma / log observation variance directions)
    JIT_FENRIR_GRAD_HYPER = 34,  // fenrir_grid_jvp_fwd_hyper_kernel (the same with log sigma directions)
    JIT_N_KINDS
};
bool is_user_rhs(int rhs_id);
bool user_tile_available(const rk_solve_cfg* c, JitKind tile);
int user_forward_tile(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, double* tiles, JitKind tile);
int user_forward(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a);
int user_forward_sqrt(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a);
int user_rhs_check(const rk_solve_cfg* c);
int user_dalton(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, int n_bobs, bool store,
                bool tile, double* out);
int user_dalton_at(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, const DaltonAt& s, int n_bobs,
                   bool tile, double* out);
// the configuration against the registration of the lane families with an n_bstate range of their own (the square-root solver,
// solve_evidence, solve_mv_dynamic, the entries on the non-uniform grid): n_block, and n_bmeas = 1 on both sides; `who` names the entry
int user_lane_check(const rk_solve_cfg* c, const char* who);
// solve_evidence: whether the tile kernel builds, and the launch; route: 0 tiles, 1 lanes, 2 square-root lanes (evidence.hip's
// EvRoute)
bool user_evidence_tile_available(const rk_solve_cfg* c);
int user_evidence(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, int route, double* logdens, double* quad,
                  double* logdet);
// solve_mv_dynamic / solve_sim_dynamic: the forward launch (dynamic.hip)
int user_dynamic(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, double scale_min, double* scale, double* logdens);
// solve_mv_grid / solve_sim_grid: the forward launch (grid.hip)
int user_grid(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& g);
// the backward pass on the grid (grid.hip): grid_bwd_mv_kernel / grid_bwd_sim_kernel on the batch-minor filtered moments
int launch_grid_bwd(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, int mode, const GridArgs& ga);
// the forward pass on the grid (grid.hip): grid_fwd_kernel for a built-in or a user right-hand side
int launch_grid_forward(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& ga);
// solve_evidence_grid / solve_mv_dynamic_grid / solve_sim_dynamic_grid: the forward launches (grid_calib.hip)
int user_grid_evidence(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& g, double* logdens, double* quad,
                       double* logdet);
int user_grid_dynamic(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& g, double scale_min, double* scale,
                      double* logdens);
// dalton_grid's store form for rk_dalton_grid_sim_draws (grid_draws.hip; all three in dalton_grid.hip): is the instance of
// this configuration left out, the pointers of a served call, and the joint filter's batch-minor records into a.mean / a.var
bool dalton_grid_left_out(const rk_solve_cfg* c, int n_bobs, bool store);
int dalton_grid_inputs(const char* who, const rk_solve_cfg* c, const rk_solve_in* in, const double* obs, const double* obs_weight,
                       const double* obs_var, const int32_t* obs_ind, int n_obs, const rk_grid_in* g, DaltonObs& o, GridArgs& ga);
int dalton_grid_store_forward(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, const GridArgs& ga,
                              int n_bobs);
// dalton_grid: the forward launch (dalton_grid.hip)
int user_dalton_grid(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, const GridArgs& g, int n_bobs,
                     bool store, double* out);
// dalton_grid_jvp: the configuration against the registration and the launch (dalton_grad.hip); the right-hand side must be of
// the gradient kind (AutoJacG around a struct with rhs_generic: rodeo_amd.trace.trace_grad_source), else the build fails
struct JvpDirs;
struct JvpHyper;
// `hy`: null for rk_dalton_grid_jvp, the hyper directions of rk_dalton_grid_jvp_hyper (the same check, the hyper kernel)
int user_dalton_grad_check(const rk_solve_cfg* c);
int user_dalton_grad(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, const GridArgs& g, const JvpDirs& dir,
                     const JvpHyper* hy, int n_items, double* value, double* dvalue);
// fenrir_grid_jvp: the same for its forward kernel (fenrir_grad.hip); dmean / dvar are the tangent records of the n_items items
int user_fenrir_grad_check(const rk_solve_cfg* c);
int user_fenrir_grad(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& g, const JvpDirs& dir, const JvpHyper* hy,
                     int n_items, double* dmean, double* dvar);
int user_interrogate(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, double t, int step, const double* mp,
                     const double* vp, double* wm, double* mm_, double* vm);
// observation models of DALTON's non-Gaussian form (rk_register_obs_source) and the hiprtc kernels built around them
struct NgObs;
struct NgObsInfo { int n_block, n_bstate, n_ycols, n_theta, n_active; };
int ng_obs_info(int obs_id, NgObsInfo* info);
int ng_forward(rk_handle h, const rk_solve_cfg* c, int obs_id, const SolveArgs& a, const NgObs& o, bool both, double* zm,
               double* zv);
int ng_obs_eval(rk_handle h, const rk_solve_cfg* c, int obs_id, const SolveArgs& a, const NgObs& o, const double* sm,
                const double* part, double* out);
// the same forward filter(s) on rk_solve_grid's non-uniform grid (daltonng_grid_kernels.hpp): o.obs_ind holds nodes
int ng_grid_forward(rk_handle h, const rk_solve_cfg* c, int obs_id, const SolveArgs& a, const NgObs& o, const GridArgs& g, bool both,
                    double* zm, double* zv);
// what rk_daltonng_grid_* (daltonng_grid.hip) share with rk_daltonng_* (all three in daltonng.hip; `who` names the entry in the
// messages): is the configuration served and the observation model registered for it, the workspace of
// rk_daltonng_workspace_bytes carved into its parts (checked against workspace_bytes), and the launch of daltonng_chain_kernel
struct NgWs;
int ng_check(const char* who, const rk_solve_cfg* c, int obs_id);
int ng_workspace(const char* who, const rk_solve_cfg* c, int n_obs, void* workspace, size_t workspace_bytes, NgWs& w);
int ng_chain(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const NgWs& w, const NgObs& o);
bool user_dense_wanted(const rk_solve_cfg* c);
int user_dense_interrogate(rk_handle h, const rk_solve_cfg* c, const DenseItgArgs& a);

// ---- fused square-root solver (solve_sqrt.hip) and fenrir in the square-root form (fenrir_sqrt.hip, entered from fenrir.hip)
int sqrt_solve(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, int mode, double* ws, size_t ws_bytes);
size_t sqrt_ws_doubles(const rk_solve_cfg* c, int mode);
size_t fenrir_sqrt_item_doubles(int p);
int fenrir_sqrt_launch(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const double* obs, const double* obs_w,
                       const double* obs_v, const int32_t* obs_ind, int n_obs, int n_bobs, double* logdens, double* states);

// fenrir's smoothing sweep over a stored backward filter on the lanes, n_bstate 2 .. 6 (fenrir.hip: fenrir_smooth_kernel)
int launch_fenrir_smooth_lanes(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const double* states);

// ---- per-block sums without atomics (magi.hip) ------------------------------------------------------------------------
// the handle's grow-only device scratch, at least `need` bytes, and logdens[b] = sum over blocks of part[blk * B + b] in block
// order (magi_sum_kernel)
int lane_scratch(rk_handle h, size_t need, double** p);
int launch_block_sum(rk_handle h, const double* part, int B, int D, double* logdens);

// ---- MFMA-tile paths: n_bstate = 3 (solve_tile3.hip), 4 (solve_tile4.hip), blocked 4 .. 8 (solve_tilen.hip) ----------
bool tile3_supported(const rk_solve_cfg* c, int mode);
bool tile3_pack_route(const rk_solve_cfg* c, int mode);     // the tile3 route that packs its rows (solve_tile3.hip, tile3_pack.hpp)
int tile3_solve(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, double* tiles, int mode, const SimLogpost* lp = nullptr);
int tile3_backward(rk_handle h, const SolveArgs& a, double* tiles, int mode, const SimLogpost* lp = nullptr);
bool tile3_sim_logpost_supported(const rk_solve_cfg* c, int n_obs);
int tile3_solve_sim_logpost(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, double* tiles, const double* obs,
                            const int32_t* obs_ind, int n_obs, double noise_sd, const double* upars, int n_prior, double prior_sd,
                            double* logpost);
int tile3_fenrir_backward(rk_handle h, const SolveArgs& a, const double* tiles, const double* obs, const double* obs_w,
                          const double* obs_v, const int32_t* obs_ind, int n_obs, double* logdens);
int tile3_fenrir_backward_at(rk_handle h, const SolveArgs& a, const double* tiles, const FenrirAt& ob);
bool tile4_supported(const rk_solve_cfg* c, int mode);
int tile4_solve(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, double* tiles, int mode);
size_t tile4_doubles(const rk_solve_cfg* c);
bool tilen_supported(const rk_solve_cfg* c, int mode);
int tilen_solve(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, double* tiles, double* ws, size_t ws_bytes, int mode);
size_t tilen_tile_doubles(const rk_solve_cfg* c);
size_t tilen_ws_doubles(const rk_solve_cfg* c, int mode);

// ---- the posterior at arbitrary times (eval_at.hip; rk_eval_at and its refusals are in api.hip) ------------------------
// n_bstate served by eval_at_kernel: at 6 the lane kernel holds five 6 x 6 matrices through the pivoted LU and spills (4 to 14
// registers, 20 to 60 B of scratch per lane, with all 512 registers in use)
constexpr int EVAL_AT_PMIN = 3, EVAL_AT_PMAX = 5;
int eval_at_launch(rk_handle h, const rk_solve_cfg* c, int layout, const rk_solve_out* filt, const rk_solve_out* smooth,
                   const rk_eval_at_in* q, double* mean_out, double* var_out);

// ---- the device path of a configuration -----------------------------------------------------------------------------
enum class SolvePath { Dense, Sqrt, Tile3, Tile4, TileN, Small };

// The one routing rule of rk_solve_filter / _mv / _sim (and of every query about their outputs).  The tile predicates
// are disjoint and false for kalman_type = square-root; for a user right-hand side they consult (and fill) the hiprtc
// cache, so they are asked in this order only.
inline SolvePath solve_path(const rk_solve_cfg* c, int mode) {
    if (dense_supported(c, mode)) return SolvePath::Dense;
    if (tile4_supported(c, mode)) return SolvePath::Tile4;
    if (tile3_supported(c, mode)) return SolvePath::Tile3;
    if (tilen_supported(c, mode)) return SolvePath::TileN;
    return c->kalman_type == RK_KALMAN_SQRT ? SolvePath::Sqrt : SolvePath::Small;
}

// RK_LAYOUT_* of a path's outputs.  The blocked tiles at n_bstate = 4 write the RK_LAYOUT_TILE4 records; the p = 3 tiles pack
// the smoothed rows only where the caller asked for it (RK_FLAG_TILE3_PACKED_MV) and the route packs at all.
inline int path_layout(SolvePath p, const rk_solve_cfg* c, int mode) {
    switch (p) {
        case SolvePath::Dense: return RK_LAYOUT_TRAJ_MAJOR;
        case SolvePath::Tile3:
            return (c->flags & RK_FLAG_TILE3_PACKED_MV) && tile3_pack_route(c, mode) ? RK_LAYOUT_TILE3_PACKED : RK_LAYOUT_TILE3;
        case SolvePath::Tile4: return RK_LAYOUT_TILE4;
        case SolvePath::TileN: return c->n_bstate == 4 ? RK_LAYOUT_TILE4 : RK_LAYOUT_TILEP;
        default: return RK_LAYOUT_BATCH_MINOR;
    }
}

// ---- launch geometry --------------------------------------------------------------------------------------------------
// One function per kernel family, called by the launcher of its ahead-of-time instances and by the launcher of its
// hiprtc builds (rhs_jit.hip), so that the two cannot size a grid differently.
struct LaunchGeom { dim3 grid, block; };

// forward tile kernels: tiles per wave and waves per workgroup at n_block = D (Tpw<D> of mfma_tile.hpp and TileWaves<D> of
// solve_tile3_kernels.hpp; solve_tile3.hip asserts the equality for every D)
constexpr int tiles_per_wave(int D) { return D == 3 ? 3 : 4; }
constexpr int tile_waves(int D) { return D <= 4 ? 1 : (D + 3) / 4; }

// lane kernels with one trajectory per lane: fwd_kernel, fwd_kernel_m, interrogate_kernel(_m), daltonng_obs_kernel
inline LaunchGeom fwd_lane_geom(int B) { return {dim3(div_up(B, 64)), dim3(64)}; }
// fwd_sqrt_kernel: 64 / D trajectories per wave (solve_sqrt_kernels.hpp)
inline LaunchGeom fwd_sqrt_geom(int B, int D) { return {dim3(div_up(B, 64 / D)), dim3(64)}; }
// the backward lane kernels of lane_backward.hpp, one (block, trajectory) per lane (bwd_sim_draws_kernel adds grid.y)
inline LaunchGeom bwd_lane_geom(int B, int D) { return {dim3(div_up(B * D, 64)), dim3(64)}; }
// fwd_tile3_kernel, fwd_tile4_kernel, fwd_tilen_kernel: whole trajectories in one wave up to four blocks, beyond that one
// workgroup of tile_waves(D) waves per trajectory
inline LaunchGeom fwd_tile_geom(int B, int D) {
    const int nw = tile_waves(D);
    return {dim3(nw == 1 ? div_up(B * D, tiles_per_wave(D)) : B), dim3(64 * nw)};
}
// dalton_fwd_kernel, dalton_fwd_at_kernel, daltonng_fwd_kernel: the log-likelihood forms run two filters per trajectory
// in the two halves of a wave (pair: 32 trajectories per wave), the store forms one (64)
inline LaunchGeom dalton_lane_geom(int B, bool pair) { return {dim3(div_up(B, pair ? 32 : 64)), dim3(64)}; }
// dalton_fwd_tile3_kernel, dalton_fwd_at_tile3_kernel (n_block <= 4): 2 B (pair) or B filter instances of D tiles
inline LaunchGeom dalton_tile_geom(int B, int D, bool pair) {
    return {dim3(div_up((pair ? 2 * B : B) * D, tiles_per_wave(D))), dim3(64)};
}

// ---- draws per lane of the many-draws backward kernels (sim_draws.hip, grid_draws.hip) -------------------------------------
// most draws a lane carries down the chain: C * P doubles of carry on top of the one-draw kernel's registers (instances: C = 1,
// 2 and this; sim_draws_chunk picks one per call)
constexpr int SIM_DRAWS_CHUNK = 4;

// Draws per lane of this call: 1, 2 or SIM_DRAWS_CHUNK.  The chain of n_steps dependent steps bounds the kernel's time from
// below, and a draw more per lane lengthens every step, so sharing the gain work pays only once the waves no longer fit the
// machine side by side: the smallest chunk whose waves fit one per SIMD (four SIMDs per CU), else the largest.
// RK_SIM_DRAWS_CHUNK = 1, 2 or 4 (read per call) fixes it, for tests and measurements; the draws do not depend on it.
inline int sim_draws_chunk(rk_handle h, const rk_solve_cfg* c, int n_draws) {
    if (const char* fixed = getenv("RK_SIM_DRAWS_CHUNK")) {
        const int v = atoi(fixed);
        if (v == 1 || v == 2 || v == SIM_DRAWS_CHUNK) return v;
    }
    const long lanes_waves = div_up(c->n_traj * c->n_block, 64), simds = 4L * h->prop.multiProcessorCount;
    for (int chunk = 1; chunk < SIM_DRAWS_CHUNK; chunk *= 2)
        if (lanes_waves * div_up(n_draws, chunk) <= simds) return chunk;
    return SIM_DRAWS_CHUNK;
}

// ---- what the built-in instances of several families share ---------------------------------------------------------------
// largest n_bstate of DALTON's built-in lane instances (dalton, dalton_at): three blocks at n_bstate = 6 hold more state than
// a lane's registers (the store form spilled over 2 KiB per lane), so Lorenz63 stops at 5
template <class RHS>
constexpr int dalton_pmax() { return RHS::D >= 3 ? 5 : 6; }

// a built-in right-hand side reads RHS::NTHETA parameters: fewer given (with a parameter array at all) is refused
template <class RHS>
int check_n_theta(const rk_solve_cfg* c, const SolveArgs& a) {
    RK_REQUIRE(c->n_theta == 0 || c->n_theta >= RHS::NTHETA || !a.theta, RK_ERR_INVALID,
               "rhs %d needs %d parameters, got n_theta=%d", c->rhs_id, RHS::NTHETA, c->n_theta);
    return RK_OK;
}

// ---- compile-time dispatch ------------------------------------------------------------------------------------------
// f(std::integral_constant<int, v>{}) for v in [Lo, Hi]; false (f not called) outside.  Instantiates f for every value.
template <int Lo, int Hi, class F>
bool dispatch_int(int v, F&& f) {
    if constexpr (Lo > Hi) {
        return false;
    } else {
        if (v == Lo) {
            f(std::integral_constant<int, Lo>{});
            return true;
        }
        return dispatch_int<Lo + 1, Hi>(v, std::forward<F>(f));
    }
}

// f(RHS{}) for the built-in right-hand side rhs_id; false (f not called) for any other id.
template <class F>
bool with_builtin_rhs(int rhs_id, F&& f) {
    switch (rhs_id) {
        case RK_RHS_FITZHUGH_NAGUMO: f(FitzHughNagumo{}); return true;
        case RK_RHS_LORENZ63: f(Lorenz63{}); return true;
        case RK_RHS_HIGHER_ORDER: f(HigherOrder{}); return true;
    }
    return false;
}

// is rhs_id a built-in right-hand side with n_block blocks (RHS::D)?
inline bool builtin_has_n_block(int rhs_id, int n_block) {
    bool fits = false;
    with_builtin_rhs(rhs_id, [&](auto rhs) { fits = decltype(rhs)::D == n_block; });
    return fits;
}

}  // namespace rk
