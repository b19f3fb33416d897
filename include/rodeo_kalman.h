/*
 * rodeo_kalman.h -- C ABI of librodeo_kalman.so: MI355X (gfx950) implementation of rodeo's Kalman
 * filter / smoother time-stepping core, batched over independent trajectories.
 *
 * The reference (mlysy/rodeo v1.1.3) has no FFI: its boundaries are Python call conventions.  Each entry point
 * below cites the reference function whose work it performs (paths relative to the reference tree); the Python
 * package rodeo_amd/ binds these with ctypes and re-exposes rodeo's own names and keyword arguments
 * (INTEGRATION.md shows the binding).  Plain pointers and sizes only -- no torch / JAX types.
 *
 * Conventions
 * -----------
 *  - Every function returns an int status: RK_OK (0) or a negative RK_ERR_* code; rk_last_error() returns a
 *    thread-local message for the last failure.  The library never aborts.  Non-finite values propagate
 *    silently, as in the reference (no NaN checks anywhere in src/rodeo/).
 *  - The caller owns every buffer.  Device buffers come from rk_alloc / go to rk_free; the library keeps no
 *    pointer between calls.
 *  - One handle <-> one HIP device + one stream.  Calls on a handle are asynchronous w.r.t. the host unless
 *    stated otherwise; rk_sync(h) waits.  Calls on one handle must be serialised by the caller.
 *  - All arithmetic is IEEE fp64.
 *
 * Device data layout ("batch-minor")
 * ----------------------------------
 *  A per-trajectory array of logical shape S (e.g. (n_block, n_bstate, n_bstate)) for a batch of B trajectories
 *  is stored as the array of shape (S..., B): the element e of trajectory b sits at  ptr[e * B + b].
 *  Consecutive lanes of a wavefront therefore touch consecutive 8-byte words (512 B per wave per element).
 *  Time-indexed outputs have shape (n_steps + 1, S..., B).  Inputs flagged "shared" (batched == 0) have plain
 *  shape S and are broadcast to all trajectories.
 */
#ifndef RODEO_KALMAN_H
#define RODEO_KALMAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------------------------- */
#define RK_OK                 0
#define RK_ERR_INVALID       -1   /* null pointer / bad shape / inconsistent arguments                      */
#define RK_ERR_UNSUPPORTED   -2   /* combination of (rhs, n_block, n_bstate, n_bmeas, interrogate, kalman)  */
#define RK_ERR_HIP           -3   /* a HIP runtime call failed                                              */
#define RK_ERR_RCCL          -4   /* an RCCL call failed                                                    */
#define RK_ERR_NOMEM         -5

/* ---- enumerations ------------------------------------------------------------------------------------- */
/* kalman_type string of src/rodeo/solve.py:138-143 */
#define RK_KALMAN_STANDARD    0   /* "standard"    -> src/rodeo/kalmantv/standard.py    */
#define RK_KALMAN_SQRT        1   /* "square-root" -> src/rodeo/kalmantv/square_root.py */

/* interrogate callable of src/rodeo/solve.py:70-78, recognised by identity on the Python side */
#define RK_INTERROGATE_RODEO      0   /* src/rodeo/interrogate.py:87-115 */
#define RK_INTERROGATE_SCHOBER    1   /* src/rodeo/interrogate.py:50-62  */
#define RK_INTERROGATE_KRAMER     2   /* src/rodeo/interrogate.py:65-84  */
#define RK_INTERROGATE_CHKREBTII  3   /* src/rodeo/interrogate.py:13-47  */

/* built-in ODE right-hand sides (device code for the `ode_fun` callable of src/rodeo/solve.py:218) */
#define RK_RHS_FITZHUGH_NAGUMO  1   /* README.md:92-99; theta = (a, b, c); n_block = 2, n_bmeas = 1           */
#define RK_RHS_LORENZ63         2   /* docs/examples/lorenz.md:85-92; theta = (rho, sigma, beta); n_block = 3 */
#define RK_RHS_HIGHER_ORDER     3   /* docs/examples/higher_order.md:47-59; x'' = sin 2t - x; n_block = 1     */
#define RK_RHS_LINEAR_DENSE     4   /* x' = A x as one dense block (prior/indep_init.py); theta = A row-major */
#define RK_RHS_USER_BASE        1000 /* ids returned by rk_register_rhs_source start here                     */

/* flags for rk_solve_cfg.flags */
#define RK_FLAG_STORE_PRED   1    /* also write the predicted moments (solve.py:93-96 state_pred)            */
#define RK_FLAG_BATCH_MINOR  2    /* force the batch-minor kernels/layout even where the tile path exists    */
#define RK_FLAG_TILE3_PACKED_MV 4 /* rk_solve_mv may leave its smoothed n_bstate = 3 tile records packed
                                     (RK_LAYOUT_TILE3_PACKED); read by rk_solve_mv / rk_solve_layout(RK_MODE_MV)
                                     alone, ignored by every other entry and route.  Unset: today's bytes.      */

/* which call a layout query refers to */
#define RK_MODE_FILTER  0
#define RK_MODE_MV      1
#define RK_MODE_SIM     2

/* output layouts of the fused solvers (see rk_solve_layout) */
#define RK_LAYOUT_BATCH_MINOR  0  /* mean_state (N+1, d, p, B), var_state (N+1, d, p, p, B)                  */
#define RK_LAYOUT_TILE3        1  /* n_bstate = 3 only: var_state holds (N+1, B, d, 3, 4) doubles, row i of a
                                     block = [Sigma[i][0..2], mu[i]]; mean_state is not used (may be NULL)  */
#define RK_LAYOUT_TILE3_PACKED 5  /* RK_LAYOUT_TILE3 with the smoothed records of the time rows 1 .. N-1 packed in place:
                                     same buffer, same size (rk_solve_sizes), rows 0 and N natural.  Tiles come in
                                     tile-waves of four (tile = b * d + block; tile-wave tw = tile / 4 owns the 384-byte
                                     stripe at byte 384 tw of every time row).  With n_tiles = B * d and
                                     rk_tile3_packed_waves(N, n_tiles) = W, the records of steps 1 .. N-1 of the tiles
                                     < 4 W are 9 doubles [S00 S01 S02 S11 S12 S22 | mu0 mu1 mu2] (Sigma's upper triangle
                                     row-major, then the mean; Sigma is symmetric): the records of the steps 4k .. 4k+3
                                     of a tile-wave are 4 x 4 x 72 = 1152 contiguous bytes (step-major, then tile) laid
                                     over its stripe in the time rows 3k+1, 3k+2, 3k+3, i.e. slot s of (step n, tile)
                                     is byte ((n & 3) * 288 + (tile & 3) * 72 + 8 s) of group k = n / 4, byte x of a
                                     group being byte x % 384 of the stripe in time row 3k + 1 + x / 384.  Every other
                                     record (W = 0: N < 16 or an array of 2 GiB and more; the tiles of a ragged last
                                     tile-wave) is the natural RK_LAYOUT_TILE3 tile.  Bytes of the stripe rows that
                                     hold no record of a step 1 .. N-1 are unspecified.  Reported by rk_solve_layout for
                                     RK_MODE_MV only, with RK_FLAG_TILE3_PACKED_MV set, on the route that packs: a
                                     built-in right-hand side in tile form at n_block = 2, kalman_type standard, not
                                     chkrebtii, and the environment switch RK_TILE3_PACK not "0".  rk_solve_filter on
                                     the same buffer rewrites every row in the natural layout.                       */
#define RK_LAYOUT_TILE4        3  /* n_bstate = 4 only: var_state holds (N+1, B, d, 20) doubles per block:
                                     [Sigma row-major (16) | mu (4)]; mean_state is not used (may be NULL)   */
#define RK_LAYOUT_TILEP        4  /* blocked tile path, n_bstate = 5 .. 8: var_state holds (N+1, B, d, p*p + p) doubles per
                                     block: [Sigma row-major (p*p) | mu (p)]; mean_state is not used (may be NULL)
                                     (RK_LAYOUT_TILE4 is this format at p = 4)                                   */
#define RK_LAYOUT_TRAJ_MAJOR   2  /* dense large-block path: the reference's own layout with a leading batch
                                     axis, mean_state (B, N+1, d, p), var_state (B, N+1, d, p, p).  With
                                     kalman_type = RK_KALMAN_SQRT var_state (and var_pred) hold the LOWER factors
                                     L_n row-major, exact zeros above the diagonal (what src/rodeo/solve.py
                                     returns in that mode)                                                    */

typedef struct rk_handle_s* rk_handle;

/* ---- handle, memory, synchronisation ------------------------------------------------------------------ */
int         rk_create(int device_id, rk_handle* h);
int         rk_destroy(rk_handle h);
const char* rk_last_error(void);
const char* rk_version(void);
int         rk_device_count(int* n);
int         rk_device_name(rk_handle h, char* buf, size_t buflen);
int         rk_alloc(rk_handle h, size_t bytes, void** dptr);
int         rk_free(rk_handle h, void* dptr);
int         rk_memset(rk_handle h, void* dptr, int value, size_t bytes);
int         rk_h2d(rk_handle h, void* dst_dev, const void* src_host, size_t bytes);   /* synchronous */
int         rk_d2h(rk_handle h, void* dst_host, const void* src_dev, size_t bytes);   /* synchronous */
int         rk_d2d(rk_handle h, void* dst_dev, const void* src_dev, size_t bytes);    /* asynchronous, on the handle's stream */
int         rk_sync(rk_handle h);

/* HIP-event timing on the handle's stream (the stream every kernel of this library is launched on). */
int         rk_timer_start(rk_handle h);
int         rk_timer_stop(rk_handle h, double* elapsed_ms);     /* records, synchronises, returns elapsed   */
/* Per-kernel device time of the last rk_solve_* call on this handle, from HIP events bracketing each launch.
 * Enabled with rk_profile_enable(h, 1); names/ms arrays of capacity cap are filled, *n = number of launches.
 * rk_profile_enable(h, 2) keeps the entries of every call since it was enabled (rk_profile_last then returns all of
 * them, in launch order) instead of only those of the last solve; rk_profile_enable(h, 0) switches it off. */
int         rk_profile_enable(rk_handle h, int on);
int         rk_profile_last(rk_handle h, int cap, const char** names, double* ms, int* n);

/* ---- user-supplied ODE right-hand sides ------------------------------------------------------------------------
 * The `ode_fun(X, t, **params)` callable of src/rodeo/solve.py:218 (and its jax.jacfwd, src/rodeo/interrogate.py:76)
 * for an ODE that is not built in: HIP source defining, inside namespace rk, a struct with the interface of
 * rodeo_amd/csrc/rhs.hpp (D, NTHETA, NDEP, f<P>, fjac<P>) -- or a scalar-generic `rhs<T, P>` used through
 * "AutoJac<Name>" (forward-mode duals, rodeo_amd/csrc/dual.hpp).  type_name is that C++ type.  The kernels are
 * compiled with hiprtc on first use per (n_bstate, interrogation); n_bmeas = 1, kalman_type = standard.
 * rk_rhs_compile_check compiles without loading (needs no GPU) and reports compiler errors via rk_last_error().   */
int rk_register_rhs_source(const char* type_name, const char* source, int32_t n_block, int32_t n_theta,
                           int32_t* rhs_id);
/* the same for a right-hand side with n_bmeas > 1 measurements per block (src/rodeo/solve.py:48-51: ode_weight (n_block,
 * n_bmeas, n_bstate)), e.g. the reference's "non-block" form of a small system (prior/indep_init.py, examples/solve_nb.py):
 * `type_name` then names a type with the interface of csrc/solve_small_m_kernels.hpp (rk::AutoJacM<...> around a
 * scalar-generic rhs writing out[D][M]); such right-hand sides run on the lane-per-trajectory kernels (n_bstate <= 9,
 * n_bmeas <= 4) or, for ONE block beyond that (n_bmeas up to 256, n_bstate up to 768), on the dense MFMA path with its
 * interrogation kernel built around them (csrc/solve_dense_itg_kernels.hpp; standard filter, all solvers and interrogations). */
int rk_register_rhs_source_m(const char* type_name, const char* source, int32_t n_block, int32_t n_bmeas, int32_t n_theta,
                             int32_t* rhs_id);
int rk_rhs_compile_check(int32_t rhs_id, int32_t n_bstate, int32_t interrogate);

/* ---- whole-solve boundary ---------------------------------------------------------------------------------
 * Mirrors  solve_mv / solve_sim (key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate,
 *                                prior_pars, kalman_type, **params)         src/rodeo/solve.py:125-129,208-212 */
typedef struct {
    int32_t  n_traj;        /* B: trajectories held by THIS handle/rank                                     */
    int32_t  n_steps;       /* N (solve.py:223)                                                             */
    int32_t  n_block;       /* d = ode_weight.shape[0]                                                      */
    int32_t  n_bstate;      /* p = ode_weight.shape[2]                                                      */
    int32_t  n_bmeas;       /* m = ode_weight.shape[1]                                                      */
    int32_t  rhs_id;        /* RK_RHS_*                                                                     */
    int32_t  interrogate;   /* RK_INTERROGATE_*                                                             */
    int32_t  kalman_type;   /* RK_KALMAN_*                                                                  */
    int32_t  n_theta;       /* doubles of ODE parameters per trajectory                                     */
    int32_t  flags;         /* RK_FLAG_*                                                                    */
    double   t_min, t_max;  /* solve.py:221-222; step n is interrogated at t_min + (t_max-t_min)(n+1)/N     */
    uint64_t seed;          /* Philox key (stands in for the jax PRNG `key`; see oracle/counter_rng.py)     */
    uint64_t traj_offset;   /* global index of local trajectory 0: makes draws independent of the sharding  */
} rk_solve_cfg;

typedef struct {
    const double* ode_weight;    int32_t ode_weight_batched;    /* W  (d, m, p [,B])   solve.py:219         */
    const double* ode_init;      int32_t ode_init_batched;      /* x0 (d, p [,B])      solve.py:220         */
    const double* prior_weight;  int32_t prior_weight_batched;  /* Q  (d, p, p [,B])   prior_pars[0]        */
    const double* prior_var;     int32_t prior_var_batched;     /* R  (d, p, p [,B])   prior_pars[1]        */
    const double* theta;         int32_t theta_batched;         /* (n_theta [,B])      **params, packed     */
} rk_solve_in;

typedef struct {
    /* filtered moments; after rk_solve_mv they hold the SMOOTHED moments (smoothing is done in place)      */
    double* mean_state;     /* (N+1, d, p, B)                                                               */
    double* var_state;      /* (N+1, d, p, p, B)                                                            */
    /* predicted moments, only written when RK_FLAG_STORE_PRED is set (may be NULL otherwise); with          */
    /* RK_LAYOUT_TRAJ_MAJOR (the dense path) they are trajectory-major like the state: (B, N+1, p[, p])     */
    double* mean_pred;      /* (N+1, d, p, B)                                                               */
    double* var_pred;       /* (N+1, d, p, p, B)                                                            */
    /* rk_solve_sim: the sample path; mean_state / var_state are then the filter workspace                  */
    double* x_state;        /* (N+1, d, p, B)                                                               */
    /* scratch for the dense large-block path: rk_solve_workspace_bytes() bytes (NULL if that returns 0)     */
    void*   workspace;
    /* size of `workspace` in bytes: a call whose configuration needs more is refused (RK_ERR_INVALID) before */
    /* any kernel is launched                                                                                */
    size_t  workspace_bytes;
} rk_solve_out;

/* Output layout the fused kernels use for this configuration and call (RK_MODE_*).  The MFMA-tile kernels
 * (n_bstate = 3 or 4, n_bmeas = 1, solve_mv / filter, kramer | schober | rodeo) write RK_LAYOUT_TILE3 / _TILE4, the dense
 * path RK_LAYOUT_TRAJ_MAJOR; everything else
 * RK_LAYOUT_BATCH_MINOR.  The caller sizes and interprets out->mean_state / var_state accordingly.             */
int rk_solve_layout(const rk_solve_cfg* cfg, int32_t mode, int32_t* layout);
/* bytes of the output arrays for a configuration in the given layout (any pointer may be NULL);
 * RK_LAYOUT_TILE3: *mean_bytes = 0, *var_bytes = ((N+1) * B * d * 12 + 128 * ceil(B * d / 8)) * 8 -- the buffer MUST
 * have this size: behind the tiles sits a scratch tail (64 doubles per wave) that lanes without an output slot use.
 * RK_LAYOUT_TILE4 likewise (20 doubles per tile + 128 per wave); always size tile buffers with this function.   */
int rk_solve_sizes(const rk_solve_cfg* cfg, int32_t layout, size_t* mean_bytes, size_t* var_bytes);
/* RK_LAYOUT_TILE3_PACKED: the number W of leading tile-waves (four tiles each) whose records of the steps 1 .. N-1 are packed,
 * for n_steps = N and n_tiles = B * d: n_tiles / 4 when N >= 16 and the tile array (N+1) * n_tiles * 96 bytes stays below
 * 0x7fff0000, else 0.  The one size rule of the kernels that write and read the layout; needs no handle and no GPU.   */
int rk_tile3_packed_waves(int32_t n_steps, int32_t n_tiles);

/* bytes of device scratch (rk_solve_out.workspace) the configuration needs; 0 for the standard small-block kernels.  Dense path
 * with RK_KALMAN_SQRT and mode != RK_MODE_FILTER: per-trajectory scratch PLUS the predicted factors of every step,
 * (B, N+1, p, p) doubles (src/rodeo/kalmantv/square_root.py:170-175 solves with them in the backward pass), unless
 * RK_FLAG_STORE_PRED hands the caller's var_pred to the library for that purpose.
 * Blocked tile path (n_bstate 4..8): the hand-off records of the two-kernel backward passes (solve_sim; solve_mv only with
 * RK_TILEN_BWD=split -- the default one-kernel solve_mv needs none of it, the size is still reported for that switch).
 * Small blocks with RK_KALMAN_SQRT, rk_solve_mv / rk_solve_sim: (N, d, 3p^2 + p | p^2 + 2p, B) doubles of records for the two-kernel backward pass;
 * OPTIONAL -- with workspace = NULL (or too small) the one-kernel backward pass runs, same results, about twice the time. */
int rk_solve_workspace_bytes(const rk_solve_cfg* cfg, int32_t mode, size_t* bytes);

/* forward pass only: src/rodeo/solve.py:31-122 (_solve_filter).  out->mean_state/var_state <- filtered. */
int rk_solve_filter(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out);
/* forward + backward mean/variance smoother: src/rodeo/solve.py:208-302 (solve_mv).                     */
int rk_solve_mv(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out);
/* forward + backward sampler: src/rodeo/solve.py:125-205 (solve_sim).  out->x_state <- one draw per traj. */
int rk_solve_sim(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out);

/* The solver's posterior at arbitrary times (an addition: the reference returns its posterior on the grid only).  `filt`
 * holds the records of rk_solve_filter and `smooth` those of rk_solve_mv for the SAME cfg / in / seed, both in `layout` =
 * rk_solve_layout(cfg, RK_MODE_FILTER) = rk_solve_layout(cfg, RK_MODE_MV) (two buffers: rk_solve_mv smooths in place) -- or
 * `layout` = RK_LAYOUT_TILE3_PACKED, where that is what rk_solve_layout(cfg, RK_MODE_MV) reported for `smooth` (`filt` is then
 * RK_LAYOUT_TILE3).  Smoothed n_bstate = 3 tile records are read with Sigma's lower triangle taken from the upper one.  Only
 * var_state (and mean_state in RK_LAYOUT_BATCH_MINOR) of the two are read.  Per query k the device array `query` (T, 3) holds
 * the node n, an on-node flag and the slot of its prior quadruple: with the flag set the smoothed record n is copied (the
 * bits of rk_solve_mv); without it the time lies in (t_n, t_{n+1}), n < N, and by the prior's Markov property
 *     (mu_t, Sigma_t) = predict(filt[n]; Q1, R1),  (mu', Sigma') = predict((mu_t, Sigma_t); Q2, R2)   standard.py:57-59
 *     G = Sigma_t Q2^T Sigma'^{-1}                                                                     standard.py:175-176
 *     mu = mu_t + G (mu^s[n+1] - mu'),  Sigma = Sigma_t + G (Sigma^s[n+1] - Sigma') G^T                 standard.py:213-216
 * with (Q1, R1) / (Q2, R2) the prior over t - t_n / t_{n+1} - t: trans (n_quad, 2, d, p, p [,B]) = (Q1, Q2) and noise
 * likewise = (R1, R2) per slot, batch-minor where batched.  Indices are clamped to the buffers.  Results in the reference's
 * layout with the batch axis first: mean_out (B, T, d, p), var_out (B, T, d, p, p).  One lane per (query, trajectory,
 * block), no time loop.  Served: kalman_type = RK_KALMAN_STANDARD, n_bstate 3..5 (at 6 the lane kernel spills), every
 * layout but RK_LAYOUT_TRAJ_MAJOR (RK_ERR_UNSUPPORTED otherwise, before the handle is looked at).                       */
typedef struct {
    int32_t        n_query;                              /* T                                                    */
    int32_t        n_quad;                               /* quadruple slots (at least 1, also when none is used)  */
    const int32_t* query;                                /* (T, 3) on the device: node, on-node flag, slot        */
    const double*  trans;   int32_t trans_batched;       /* (n_quad, 2, d, p, p [,B]): Q1, Q2                     */
    const double*  noise;   int32_t noise_batched;       /* (n_quad, 2, d, p, p [,B]): R1, R2                     */
} rk_eval_at_in;
int rk_eval_at(rk_handle h, const rk_solve_cfg* cfg, int32_t layout, const rk_solve_out* filt, const rk_solve_out* smooth,
               const rk_eval_at_in* q, double* mean_out, double* var_out);

/* Gather x[obs_ind[k], :, 0] and reduce the Gaussian observation log-likelihood + N(0, prior_sd^2) log-prior
 * per trajectory: the tail of the user log-posterior of docs/examples/parameter.md:188-210,331-354 (and of
 * src/rodeo/inference/basic.py:47-62 with a Gaussian obs_loglik).
 *   state: the solver output holding the path -- layout RK_LAYOUT_BATCH_MINOR: x_state / mean_state (N+1, d, p, B);
 *          layout RK_LAYOUT_TILE3 / RK_LAYOUT_TILE3_PACKED / RK_LAYOUT_TILE4: the tile buffer (the mean is column 3 / slots
 *          6..8 of a packed record / entries 16..19);
 *   obs (n_obs, d) row-major on device; obs_ind (n_obs) int32 on device (clamped to [0, N]), any order; with
 *   n_obs = 0 (prior only, or zeros without upars) neither is read and both may be NULL -- here and below;
 *   upars (n_prior, B) batch-minor or NULL (no prior term); out logpost (B).                              */
int rk_gauss_obs_logpost(rk_handle h, int32_t n_traj, int32_t n_steps, int32_t n_block, int32_t n_bstate,
                         int32_t layout, const double* state, const double* obs, const int32_t* obs_ind,
                         int32_t n_obs, double noise_sd, const double* upars, int32_t n_prior, double prior_sd,
                         double* logpost);

/* rk_solve_sim followed by rk_gauss_obs_logpost on its sample path, as ONE call: the body of the user-level log-posterior of
 * docs/examples/parameter.md:331-354 (constrain -> solve_sim with interrogate_chkrebtii -> Gaussian observation
 * log-likelihood at searchsorted indices + normal log-prior), what a pseudo-marginal sampler evaluates once per proposal
 * (src/rodeo/inference/pseudo_marginal.py:135-149).  On the n_bstate = 3 tile path with n_block in {1, 2, 4} the backward
 * sampler reduces the log-posterior itself (no second launch) and out->x_state may be NULL: then no path is stored at
 * all and logpost (B) is the only result.  Any other configuration runs the two kernels back to back and needs x_state.
 * upars / obs / obs_ind must be on the device BEFORE the call (upload them before launching, not between the launches).
 * obs_ind is REQUIRED to be ascending (equal neighbours allowed) on the fused route: the sampler walks the indices from the
 * end and waits for its step index to meet the next one, so an index that is larger than its successor is never met --
 * its terms and those of every observation before it are left out of logpost, and no error is returned (the indices live
 * on the device; checking them would cost a download per evaluation).  Sort them, rows of obs along, before the upload
 * (rodeo_amd.inference.logpost.check_obs does).  The two-kernel route and rk_gauss_obs_logpost accept any order.        */
int rk_solve_sim_logpost(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out,
                         const double* obs, const int32_t* obs_ind, int32_t n_obs, double noise_sd,
                         const double* upars, int32_t n_prior, double prior_sd, double* logpost);

/* Fenrir's backward pass (src/rodeo/inference/fenrir.py:86-259; the forward pass is rk_solve_filter with the same
 * cfg / in, fenrir.py:304-313): log p(y_{0:M} | Z_{1:N}) per trajectory from the filter's output in `out` -- either
 * the RK_LAYOUT_TILE3 tiles (no flags; predicted moments are re-evaluated on the fly; n_bobs = 1) or the RK_LAYOUT_TILE4 /
 * RK_LAYOUT_TILEP records (no flags; n_bstate 4..8, any n_bobs) when rk_solve_layout reports that layout for
 * RK_MODE_FILTER, or the batch-minor filtered and predicted moments of a call with
 * RK_FLAG_STORE_PRED | RK_FLAG_BATCH_MINOR (n_bstate 2..6; required at n_bstate = 3 when n_bobs > 1).  Observations (fenrir.py:106-122), n_bobs = 1..3
 * per block: obs (n_obs, d, n_bobs), obs_weight (n_obs, d, n_bobs, p), obs_var (n_obs, d, n_bobs, n_bobs) row-major on
 * device, shared by all trajectories; obs_ind (n_obs) = searchsorted(sim_times, obs_times), ascending.  logdens (B) is
 * overwritten.  The log-density follows src/rodeo/utils.py:60-78 (eigendecomposition of the forecast variance;
 * eigenvalues with |w| <= 1e-8 contribute nothing).
 * kalman_type = RK_KALMAN_SQRT (fenrir.py:292-296): `out` holds the batch-minor filtered means and FACTORS of the
 * square-root rk_solve_filter (no predictions needed: they are re-evaluated), prior_var and obs_var are lower
 * factors; square_root.forecast squares its factor (square_root.py:343-344), so the value is the same log-likelihood.    */
int rk_fenrir_backward(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out,
                       const double* obs, const double* obs_weight, const double* obs_var, const int32_t* obs_ind,
                       int32_t n_obs, int32_t n_bobs, double* logdens);

/* Fenrir's data-adaptive solver (src/rodeo/inference/fenrir.py:333-457 `_smooth_mv`, `solve_mv`): mean and variance of
 * p(X_{0:N} | Z_{1:N}, Y_{0:M}).  Input as for rk_fenrir_backward with RK_FLAG_STORE_PRED | RK_FLAG_BATCH_MINOR; the
 * backward filter's moments are kept in `workspace` (rk_fenrir_workspace_bytes), the smoothing pass overwrites
 * out->mean_state / out->var_state (batch-minor (N+1, d, p [,p], B)) with the result.  RK_KALMAN_SQRT (fenrir.py:421-426):
 * input as for the square-root rk_fenrir_backward, the result's var_state holds factors.                              */
int rk_fenrir_workspace_bytes(const rk_solve_cfg* cfg, size_t* bytes);
int rk_fenrir_solve_mv(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out,
                       const double* obs, const double* obs_weight, const double* obs_var, const int32_t* obs_ind,
                       int32_t n_obs, int32_t n_bobs, void* workspace);

/* DALTON for Gaussian observations (src/rodeo/inference/dalton.py:39-545, kalman_type = standard).  Observations as for
 * rk_fenrir_backward (n_bobs = 1..3), obs_ind strictly increasing up to n_steps; an observation at grid index 0 enters the
 * joint density only, indices above n_steps never match.  Served: n_bmeas = 1, n_bstate 2..6 (2..5 with three or more
 * blocks), interrogate rodeo / schober / kramer, any built-in right-hand side or a user one with n_bmeas = 1.  Routes: the
 * p = 3 MFMA tiles (n_bobs = 1, n_block 1..4, a configuration of the tile solver; dalton_tile3_kernels.hpp) unless
 * RK_DALTON_LANES=1, else the lane-per-trajectory kernels (dalton_kernels.hpp).
 * rk_dalton_layout: the layout that rk_dalton_solve writes for this cfg / mode / n_bobs (RK_LAYOUT_TILE3 on the tiles,
 * RK_LAYOUT_BATCH_MINOR on the lanes; the cfg's flags do not enter), or RK_ERR_UNSUPPORTED (+ message) if not served.
 * rk_dalton_loglik: log p(Y | Z = 0) = logdens_joint - logdens_marg per trajectory into logdens (B); both filters of all B
 * trajectories run in one launch and nothing else is written (`out` is not needed).
 * rk_dalton_solve: the joint filter (RK_MODE_FILTER), + the smoothing pass (RK_MODE_MV) or + the sampler (RK_MODE_SIM) of
 * rk_solve_mv / rk_solve_sim into `out`, in exactly the layout rk_solve_layout(cfg, mode) reports -- refused unless that
 * equals rk_dalton_layout (set RK_FLAG_BATCH_MINOR where they differ).  RK_FLAG_STORE_PRED (lanes) also writes the
 * predictions.  On the tiles out->var_state holds the records (rk_solve_sizes) and out->mean_state is not used.            */
int rk_dalton_layout(const rk_solve_cfg* cfg, int32_t mode, int32_t n_bobs, int32_t* layout);
int rk_dalton_loglik(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in,
                     const double* obs, const double* obs_weight, const double* obs_var, const int32_t* obs_ind,
                     int32_t n_obs, int32_t n_bobs, double* logdens);
int rk_dalton_solve(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out, int32_t mode,
                    const double* obs, const double* obs_weight, const double* obs_var, const int32_t* obs_ind,
                    int32_t n_obs, int32_t n_bobs);

/* solve_evidence (an addition): the solver's own marginal likelihood log p(Z_{1:N} = 0), the evidence of the interrogations
 * under the prior, with its per-block parts quad_b = sum_n z_{n,b}^2 / s_{n,b} and logdet_b = sum_n log s_{n,b} (z the
 * innovation, s its forecast variance):  logdens = -1/2 sum_b (quad_b + logdet_b) - n_block n_steps log(2 pi) / 2, the
 * blocks summed in block order.  The density is the plain Gaussian one, without the 1e-8 threshold of utils.py:60-78 (so it
 * is not rk_dalton_loglik's marginal term wherever that rule drops a step); a zero, negative or non-finite s gives inf or
 * NaN.  Under prior_var_b -> c_b prior_var_b (the factor times sqrt(c_b) in the square-root form) quad_b becomes
 * quad_b / c_b and logdet_b becomes logdet_b + n_steps log c_b, so c_b = quad_b / n_steps maximises the evidence.
 * Served: n_bmeas = 1, interrogate rodeo / schober / kramer (not chkrebtii: it draws from the predicted variance), any
 * built-in right-hand side or a user one with n_bmeas = 1; kalman_type standard with n_bstate 2..6 (2..5 with three or more
 * blocks) or square-root with n_bstate 2..8.  Routes: the p = 3 MFMA tiles (standard, n_block 1..4, what the tile solver
 * accepts in filter mode; evidence_tile3_kernels.hpp) unless RK_EVIDENCE_LANES=1 (read per call), else the lane kernels
 * (evidence_kernels.hpp).  What is not served is refused on cfg alone -- RK_ERR_INVALID (a non-positive size) or
 * RK_ERR_UNSUPPORTED -- before the handle or any pointer is looked at.
 * Outputs (device, overwritten; each element has one writer, no atomics): logdens (n_traj); quad and logdet
 * (n_block, n_traj) batch-minor, block b of trajectory t at [b * n_traj + t].  No per-step state is written anywhere.    */
int rk_solve_evidence(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, double* logdens, double* quad,
                      double* logdet);

/* solve_mv_dynamic / solve_sim_dynamic (an addition): the solver with a per-step calibrated prior scale.  At step n -> n + 1
 * block b predicts mu- = Q mu and P = Q Sigma Q^T, interrogates at mu- (W~ = ode_weight + wgt_meas, a = mean_meas), forms the
 * innovation z = 0 - (W~ mu- + a) and r = W~ prior_var W~^T and takes c = max(z^2 / r, scale_min) as the scale of prior_var for
 * this step: Sigma- = P + c prior_var, var_meas from this Sigma- (rodeo), then the usual update with forecast variance s.
 * mode = RK_MODE_MV smooths with these predictions into out->mean_state / var_state, RK_MODE_SIM samples into out->x_state
 * (draws as in rk_solve_sim; mean_state / var_state then hold the filtered moments).  All records are RK_LAYOUT_BATCH_MINOR.
 * Further outputs (device, overwritten; each element has one writer, no atomics, no workspace): scale (n_steps, n_block,
 * n_traj), block b of step n of trajectory t at [(n * n_block + b) * n_traj + t]; logdens (n_traj), the log-evidence
 * -1/2 sum_b sum_n (z^2 / s + log s) - n_block n_steps log(2 pi) / 2 of rk_solve_evidence under the scaled prior.
 * With scale_min = 0 a step whose z is exactly 0 has c = 0 and s = 0: inf / NaN as the arithmetic produces them.
 * Served: kalman_type standard, n_bmeas = 1, n_bstate 2..5 (2..4 with three or more blocks), interrogate rodeo / schober /
 * kramer (not chkrebtii: its point is drawn from the predicted variance, which here depends on the point), any built-in
 * right-hand side or a user one with n_bmeas = 1; one lane per trajectory forward, one per (trajectory, block) backward.  What is not served is refused on cfg,
 * mode and scale_min alone -- RK_ERR_INVALID (a non-positive size, another mode, a negative or non-finite scale_min) or
 * RK_ERR_UNSUPPORTED -- before the handle or any pointer is looked at.                                                      */
int rk_solve_dynamic(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out, int32_t mode,
                     double scale_min, double* scale, double* logdens);

/* solve_mv_grid / solve_sim_grid (an addition): rk_solve_mv / rk_solve_sim on a non-uniform grid that the whole batch shares.
 * Node n sits at t[n] (n = 0..n_steps, strictly increasing; cfg->t_min / t_max are not read), step n -> n + 1 takes the prior
 * pair (q, r)[slot[n]] in place of in->prior_weight / prior_var -- steps of one length share a slot -- and interrogates at
 * t[n+1].  The smoothing gain of step n is formed with that step's q.  Pairs are (n_slots, d, p, p) row-major, or
 * (n_slots, d, p, p, B) batch-minor where q_batched / r_batched say so; slots are clamped to 0..n_slots-1.  in->prior_weight /
 * prior_var must still be given (slot 0's, by convention) but are not read by the kernels.
 * mode = RK_MODE_MV smooths into out->mean_state / var_state, RK_MODE_SIM samples into out->x_state (Philox keys as in
 * rk_solve_sim; mean_state / var_state then hold the filtered moments).  All records are RK_LAYOUT_BATCH_MINOR and cfg->flags
 * must carry RK_FLAG_BATCH_MINOR.  No workspace.
 * Served: kalman_type standard, n_bmeas = 1, n_bstate 2..6 (2..5 with three or more blocks), the four interrogations, any
 * built-in right-hand side or a user one with n_bmeas = 1; one lane per trajectory forward (grid_kernels.hpp), one per
 * (trajectory, block) backward (grid.hip).  What is not served is refused on cfg and mode alone -- RK_ERR_INVALID (a
 * non-positive size, another mode, RK_FLAG_BATCH_MINOR missing) or RK_ERR_UNSUPPORTED -- before the handle or any pointer is
 * looked at.                                                                                                               */
typedef struct {
    const double*  t;                                    /* (n_steps + 1) node times on the device                */
    const int32_t* slot;                                 /* (n_steps) slot of every step on the device            */
    const double  *q, *r;                                /* (n_slots, d, p, p [,B]): Q, R of every slot            */
    int32_t        q_batched, r_batched;
    int32_t        n_slots;
} rk_grid_in;
int rk_solve_grid(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out, int32_t mode,
                  const rk_grid_in* g);

/* solve_evidence_grid / solve_mv_dynamic_grid / solve_sim_dynamic_grid (an addition): rk_solve_evidence and rk_solve_dynamic on
 * rk_solve_grid's non-uniform grid, i.e. the calibration of the prior scale on the grid the solver runs on.  Step n -> n + 1
 * takes the pair (q, r)[slot[n]] in place of in->prior_weight / prior_var and interrogates at t[n+1]; cfg->t_min / t_max are
 * not read.
 * rk_solve_evidence_grid: rk_solve_evidence's sums with every step's own pair -- quad_b = sum_n z^2 / s, logdet_b = sum_n log s
 * (the plain Gaussian density, no threshold on s) and logdens = -1/2 sum_b (quad_b + logdet_b) - n_block n_steps log(2 pi) / 2.
 * The scale law holds when every r of block b becomes c_b r.  Outputs as rk_solve_evidence's: logdens (n_traj); quad, logdet
 * (n_block, n_traj) batch-minor.  One kernel (grid_evidence_kernel), nothing stored per step.
 * rk_solve_dynamic_grid: rk_solve_dynamic's step with the step's own pair -- mu- = q mu, P = q Sigma q^T,
 * c = max(z^2 / (W~ r W~^T), scale_min), Sigma- = P + c r, var_meas from this Sigma- (rodeo) -- and its backward passes with
 * Sigma-_{n+1} re-evaluated as q_n Sigma_f[n] q_n^T + scale[n] r_n and the gain from q_n; mode, out, scale (n_steps, n_block,
 * n_traj) and logdens (n_traj) as for rk_solve_dynamic (Philox keys as in rk_solve_sim).  scale[n] multiplies r_n, which
 * already carries the step's length.
 * Both: all records are RK_LAYOUT_BATCH_MINOR and cfg->flags must carry RK_FLAG_BATCH_MINOR; each output element has one
 * writer, no atomics, no workspace.  Served: kalman_type standard, n_bmeas = 1, interrogate rodeo / schober / kramer, any
 * built-in right-hand side or a user one with n_bmeas = 1; n_bstate 2..6 (2..5 with three or more blocks) for the evidence and
 * 2..5 (2..4) for the dynamic solver.  What is not served is refused on cfg (and mode, scale_min) alone -- RK_ERR_INVALID (a
 * non-positive size, another mode, a negative or non-finite scale_min, RK_FLAG_BATCH_MINOR missing) or RK_ERR_UNSUPPORTED --
 * before the handle or any pointer is looked at.                                                                           */
int rk_solve_evidence_grid(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_grid_in* g, double* logdens,
                           double* quad, double* logdet);
int rk_solve_dynamic_grid(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out, int32_t mode,
                          const rk_grid_in* g, double scale_min, double* scale, double* logdens);

/* dalton_grid (an addition): rk_dalton_loglik / rk_dalton_solve on rk_solve_grid's non-uniform grid, every observation on a node.
 * obs / obs_weight / obs_var as for rk_dalton_loglik (n_bobs = 1..3); obs_ind (n_obs) holds the NODE of every observation,
 * strictly increasing in 0..n_steps: node 0 enters the joint density only and does not update x_0, a node above n_steps never
 * matches.  Step n -> n + 1 of the joint filter: the prediction with (q, r)[slot[n]], the interrogation at t[n+1], the z forecast
 * log-density and update, then -- if node n + 1 is observed -- the conditioning on y, per block (z first, y second, as
 * rk_dalton_loglik).  The marginal filter is the same without the conditioning.
 * rk_dalton_grid_loglik: logdens (B, overwritten, one writer per element) = joint - marginal.
 * rk_dalton_grid_solve: the joint filter's moments into out->mean_state / var_state (RK_LAYOUT_BATCH_MINOR), then rk_solve_grid's
 * backward pass: mode = RK_MODE_MV smooths in place, RK_MODE_SIM samples into out->x_state (Philox keys as in rk_solve_sim).
 * One route, the lanes (dalton_grid_kernels.hpp; no tile route, RK_DALTON_LANES is not read); no workspace.
 * Served: kalman_type standard, n_bmeas = 1, n_bstate 2..6 (2..5 with three or more blocks), interrogate rodeo / schober /
 * kramer, any built-in right-hand side or a user one with n_bmeas = 1; cfg->flags must carry RK_FLAG_BATCH_MINOR.  What is not
 * served is refused on cfg, mode and n_bobs alone -- RK_ERR_INVALID (a non-positive size, another mode, RK_FLAG_BATCH_MINOR
 * missing) or RK_ERR_UNSUPPORTED -- before the handle or any pointer is looked at.                                       */
int rk_dalton_grid_loglik(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const double* obs, const double* obs_weight,
                          const double* obs_var, const int32_t* obs_ind, int32_t n_obs, int32_t n_bobs, const rk_grid_in* g,
                          double* logdens);
int rk_dalton_grid_solve(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out, int32_t mode,
                         const double* obs, const double* obs_weight, const double* obs_var, const int32_t* obs_ind,
                         int32_t n_obs, int32_t n_bobs, const rk_grid_in* g);

/* dalton_grid_jvp (an addition): rk_dalton_grid_loglik's value and its directional derivatives, forward mode, with respect to
 * the ODE parameters and the initial state.  The first ten arguments are rk_dalton_grid_loglik's.  n_dir >= 1 directions:
 * dtheta (n_dir, n_theta), or (n_dir, n_theta, n_traj) batch-minor with dtheta_batched; dinit (n_dir, n_block, n_bstate), or
 * (n_dir, n_block, n_bstate, n_traj) with dinit_batched; a NULL array is a zero direction in that argument.
 * value (n_traj) = joint - marginal; dvalue (n_traj, n_dir), trajectory-major: dvalue[b n_dir + k] is the derivative of value[b]
 * along direction k.  Both are overwritten, one writer per element, no atomics: two calls give the same bits.  It is the exact
 * derivative of the filters' formulas as computed; a forecast term the value drops (|s| <= 1e-8) contributes nothing.
 * One kernel (dalton_grid_jvp_kernel, dalton_grad_kernels.hpp): a (trajectory, direction) pair per lane pair; no workspace.
 * Served: kalman_type standard, n_bmeas = 1, n_bobs = 1, interrogate rodeo / schober / kramer, fitzhugh_nagumo and lorenz63 at
 * n_bstate 2..3, and a user right-hand side of the gradient kind (hiprtc, JIT_DALTON_GRAD) with n_block n_bstate^2 <= 27; cfg->flags must carry RK_FLAG_BATCH_MINOR.  What is not served is refused on cfg, n_bobs and n_dir
 * alone -- RK_ERR_INVALID (a non-positive size, n_dir < 1, RK_FLAG_BATCH_MINOR missing) or RK_ERR_UNSUPPORTED ("not built") --
 * before the handle or any pointer is looked at.                                                                          */
int rk_dalton_grid_jvp(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const double* obs, const double* obs_weight,
                       const double* obs_var, const int32_t* obs_ind, int32_t n_obs, int32_t n_bobs, const rk_grid_in* g,
                       int32_t n_dir, const double* dtheta, int32_t dtheta_batched, const double* dinit, int32_t dinit_batched,
                       double* value, double* dvalue);
/* Build rk_dalton_grid_jvp's kernel for a registered right-hand side of the gradient kind (rodeo_amd.trace.trace_grad_source,
 * registered as AutoJacG<struct>) without a device; RK_ERR_INVALID with the compiler's log otherwise.                    */
int rk_dalton_grad_compile_check(int32_t rhs_id, int32_t n_bstate, int32_t interrogate);

/* fenrir_grid (an addition): rk_fenrir_backward / rk_fenrir_solve_mv on rk_solve_grid's non-uniform grid, every observation on a
 * node.  Both entries run the forward pass of rk_solve_grid themselves (grid_fwd_kernel: out->mean_state / var_state receive
 * the batch-minor filtered moments; Fenrir's forward pass is free of data), then the backward Markov-chain filter with every
 * step's own pair (fenrir_grid.hip): the carry starts at filt[N]; for n = N-1 .. 0 the prediction of node n + 1 is re-evaluated
 * from filt[n] with (q, r)[slot[n]], the chain steps with that q as its transition matrix, and the step conditions on y where
 * node n is observed -- node 0 like any other.  obs / obs_weight / obs_var as for rk_fenrir_backward (n_bobs = 1..3); obs_node
 * (n_obs) holds the NODE of every observation, strictly increasing in 0..n_steps; n_obs = 0 needs no observation arrays.
 * rk_fenrir_grid_loglik: logdens (B, overwritten) = log p(Y | Z).  No atomics: with several blocks every lane writes its block's
 * sum to the handle's scratch and a trajectory's sums are added in block order, so two calls give the same bits.
 * rk_fenrir_grid_solve_mv: the backward filter's moments go to `workspace` (rk_fenrir_workspace_bytes, the same item), then
 * rk_fenrir_solve_mv's smoothing sweep overwrites out->mean_state / var_state with mean and variance of p(X | Z, Y).
 * Served: kalman_type standard, n_bmeas = 1, n_bstate 2..6 (2..5 with three or more blocks), the four interrogations, any
 * built-in right-hand side or a user one with n_bmeas = 1; cfg->flags must carry RK_FLAG_BATCH_MINOR and not RK_FLAG_STORE_PRED.
 * What is not served is refused on cfg and n_bobs alone -- RK_ERR_INVALID (a non-positive size, RK_FLAG_BATCH_MINOR missing) or
 * RK_ERR_UNSUPPORTED -- before the handle or any pointer is looked at.                                                      */
int rk_fenrir_grid_loglik(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out, const double* obs,
                          const double* obs_weight, const double* obs_var, const int32_t* obs_node, int32_t n_obs, int32_t n_bobs,
                          const rk_grid_in* g, double* logdens);
int rk_fenrir_grid_solve_mv(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out, const double* obs,
                            const double* obs_weight, const double* obs_var, const int32_t* obs_node, int32_t n_obs, int32_t n_bobs,
                            const rk_grid_in* g, void* workspace);

/* fenrir_grid_jvp (an addition): rk_fenrir_grid_loglik's value and its directional derivatives, forward mode, with respect to the
 * ODE parameters and the initial state.  The first eleven arguments are rk_fenrir_grid_loglik's (out->mean_state / var_state
 * receive the batch-minor filtered moments), the directions rk_dalton_grid_jvp's: dtheta (n_dir, n_theta), or (n_dir, n_theta,
 * n_traj) batch-minor with dtheta_batched; dinit (n_dir, n_block, n_bstate), or (n_dir, n_block, n_bstate, n_traj) with
 * dinit_batched; a NULL array is a zero direction in that argument.  value (n_traj) = log p(Y | Z); dvalue (n_traj, n_dir),
 * trajectory-major: dvalue[b n_dir + k] is the derivative of value[b] along direction k.  Both are overwritten, one writer per
 * element, no atomics (with several blocks the block sums are added in block order): two calls give the same bits.  It is the
 * exact derivative of the filters' formulas as computed; a y term the value drops (|w| <= 1e-8) contributes nothing.
 * Two kernels: fenrir_grid_jvp_fwd_kernel (fenrir_grad_kernels.hpp), a (trajectory, direction) item per lane, writes every item's
 * tangent records to `workspace` -- rk_fenrir_grid_jvp_workspace_bytes: (n_steps + 1) n_block (n_bstate + n_bstate^2) n_traj
 * n_dir doubles, item-minor -- and fenrir_grid_jvp_bwd_kernel (fenrir_grad.hip), a lane per (block, item), reads them.  The
 * directions are independent: a caller short of memory runs them in chunks.
 * Served: kalman_type standard, n_bmeas = 1, n_bobs = 1, interrogate rodeo / schober / kramer, fitzhugh_nagumo and lorenz63 at
 * n_bstate 2..3, and a user right-hand side of the gradient kind (hiprtc, JIT_FENRIR_GRAD) with n_block n_bstate^2 <= 27;
 * cfg->flags must carry RK_FLAG_BATCH_MINOR.  What is not served is refused on cfg, n_bobs and n_dir alone -- RK_ERR_INVALID (a
 * non-positive size, n_dir < 1, RK_FLAG_BATCH_MINOR missing) or RK_ERR_UNSUPPORTED ("not built") -- before the handle or any
 * pointer is looked at.                                                                                                      */
int rk_fenrir_grid_jvp_workspace_bytes(const rk_solve_cfg* cfg, int32_t n_dir, size_t* bytes);
int rk_fenrir_grid_jvp(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out, const double* obs,
                       const double* obs_weight, const double* obs_var, const int32_t* obs_node, int32_t n_obs, int32_t n_bobs,
                       const rk_grid_in* g, int32_t n_dir, const double* dtheta, int32_t dtheta_batched, const double* dinit,
                       int32_t dinit_batched, void* workspace, double* value, double* dvalue);
/* Build rk_fenrir_grid_jvp's forward kernel for a registered right-hand side of the gradient kind without a device, as
 * rk_dalton_grad_compile_check does for rk_dalton_grid_jvp's, or around a built-in right-hand side (its id); RK_ERR_INVALID
 * with the compiler's log otherwise.                                                                                        */
int rk_fenrir_grad_compile_check(int32_t rhs_id, int32_t n_bstate, int32_t interrogate);

/* The hyper forms of the two (an addition): rk_dalton_grid_jvp / rk_fenrir_grid_jvp with two more directions per block, the argument
 * lists of those entries followed by dlog_sigma, dlog_sigma_batched, dlog_obs_var, dlog_obs_var_batched (rk_fenrir_grid_jvp_hyper:
 * in front of workspace).  dlog_sigma (n_dir, n_block), or (n_dir, n_block, n_traj) batch-minor with its flag: entry b is the rate
 * of log sigma_b, the prior scale of block b, under the scale law r_b ~ sigma_b^2 with q free of sigma -- every step's own r as
 * loaded gets the tangent 2 rate r, q none, and the initial variance is not scaled.  dlog_obs_var likewise: entry b is the rate of
 * a common log-scale of block b's observation variances, obs_var. = rate obs_var at every observation, node 0 and node n_steps
 * included.  A NULL array is a zero direction; with both NULL the result has rk_dalton_grid_jvp's / rk_fenrir_grid_jvp's bits.
 * Kernels of their own (dalton_grid_jvp_hyper_kernel; fenrir_grid_jvp_fwd_hyper_kernel, fenrir_grid_jvp_bwd_hyper_kernel), the
 * plain entries launch what they launched; the workspace is rk_fenrir_grid_jvp_workspace_bytes'.  Served and refused as the plain
 * entries, on cfg, n_bobs and n_dir alone; an instance whose hyper kernel would need more scratch than its yardstick is
 * RK_ERR_UNSUPPORTED ("not built").  The two compile checks build the hiprtc kinds (JIT_DALTON_GRAD_HYPER, JIT_FENRIR_GRAD_HYPER)
 * without a device, as the plain ones do.                                                                                    */
int rk_dalton_grid_jvp_hyper(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const double* obs, const double* obs_weight,
                             const double* obs_var, const int32_t* obs_ind, int32_t n_obs, int32_t n_bobs, const rk_grid_in* g,
                             int32_t n_dir, const double* dtheta, int32_t dtheta_batched, const double* dinit, int32_t dinit_batched,
                             const double* dlog_sigma, int32_t dlog_sigma_batched, const double* dlog_obs_var,
                             int32_t dlog_obs_var_batched, double* value, double* dvalue);
int rk_fenrir_grid_jvp_hyper(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out, const double* obs,
                             const double* obs_weight, const double* obs_var, const int32_t* obs_node, int32_t n_obs, int32_t n_bobs,
                             const rk_grid_in* g, int32_t n_dir, const double* dtheta, int32_t dtheta_batched, const double* dinit,
                             int32_t dinit_batched, const double* dlog_sigma, int32_t dlog_sigma_batched, const double* dlog_obs_var,
                             int32_t dlog_obs_var_batched, void* workspace, double* value, double* dvalue);
int rk_dalton_grad_hyper_compile_check(int32_t rhs_id, int32_t n_bstate, int32_t interrogate);
int rk_fenrir_grad_hyper_compile_check(int32_t rhs_id, int32_t n_bstate, int32_t interrogate);

/* solve_sim_draws (an addition): n_draws sample paths per trajectory from one forward filter.  Runs the forward pass of
 * rk_solve_filter (cfg must carry RK_FLAG_BATCH_MINOR; out->mean_state / var_state hold the filtered moments afterwards), then
 * one backward kernel, one lane per (chunk of draws, block, trajectory), which does the work that no draw changes -- the
 * record's load, the prediction, the smoothing gain, Sigma_f - G T^T and its factor -- once per step for its chunk.  A chunk is
 * 1, 2 or rk_sim_draws_chunk() = 4 draws: the smallest whose waves fit the device one per SIMD, else the largest.
 * THE SEED LAW: draw s is the path rk_solve_sim writes under the seed cfg->seed + s (mod 2^64) -- Philox is keyed with
 * (seed + s, traj_offset + trajectory, step, block, smoothing purpose) -- up to rounding.
 * keep: NULL for every node (K = n_steps + 1), else a device array of n_keep = K grid indices in 0..n_steps, strictly
 * increasing; only those nodes are written (node 0 is ode_init).  An array that breaks the rule loses rows but never writes
 * outside x_draws.  x_draws (device, overwritten, each element has one writer): (n_draws, K, n_block, n_bstate, n_traj)
 * batch-minor, element i of (draw s, kept row k, block b, trajectory t) at [(((s * K + k) * n_block + b) * n_bstate + i) *
 * n_traj + t].  No workspace; out->x_state is not used.
 * Served: kalman_type standard, n_bmeas = 1, n_bstate 2..6, any n_block, interrogate rodeo / schober / kramer (not
 * chkrebtii: its forward pass depends on the key, so the draws cannot share one filter), any built-in right-hand side or a
 * user one with n_bmeas = 1; n_draws 1..65535.  What is not served is refused on cfg alone -- RK_ERR_INVALID (a
 * non-positive size, RK_FLAG_BATCH_MINOR missing) or RK_ERR_UNSUPPORTED -- before the handle or any pointer is looked at;
 * then n_draws and n_keep (RK_ERR_INVALID).  RK_SIM_DRAWS_CHUNK = 1, 2 or 4 (read per call) fixes the chunk, for tests and
 * measurements; the draws do not depend on it.                                                                            */
int rk_solve_sim_draws(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out, int32_t n_draws,
                       const int32_t* keep, int32_t n_keep, double* x_draws);
int rk_sim_draws_chunk(void);

/* solve_sim_draws_grid / dalton.solve_sim_draws_grid (an addition): rk_solve_sim_draws on rk_solve_grid's non-uniform grid, from
 * the solver's forward filter (p(X | Z)) or from dalton_grid's joint filter (p(X | Z, Y)).
 * rk_solve_sim_draws_grid runs the forward pass of rk_solve_grid (grid_fwd_kernel), rk_dalton_grid_sim_draws the store form of
 * rk_dalton_grid_solve's joint filter (obs .. n_bobs as there: obs_ind holds the NODE of every observation); out->mean_state /
 * var_state hold the filtered moments afterwards.  Then one backward kernel (grid_bwd_sim_draws_kernel), one lane per (chunk of
 * draws, block, trajectory): rk_solve_sim_draws's, with the pair (q, r)[slot[n]] of step n in the prediction and in the
 * smoothing gain.  The chunk is rk_solve_sim_draws's (RK_SIM_DRAWS_CHUNK included); the draws do not depend on it.
 * THE SEED LAW: draw s is the path that rk_solve_grid / rk_dalton_grid_solve write in RK_MODE_SIM under the seed cfg->seed + s
 * (mod 2^64) -- Philox is keyed with (seed + s, traj_offset + trajectory, step, block, smoothing purpose).
 * keep, n_keep and x_draws (n_draws, K, n_block, n_bstate, n_traj) are rk_solve_sim_draws's, with node indices of t in
 * 0..n_steps: an array that breaks the rule loses rows but never writes outside x_draws.  No workspace; out->x_state is not used.
 * Served: kalman_type standard, n_bmeas = 1, n_bstate 2..6 (2..5 with three or more blocks), interrogate rodeo / schober /
 * kramer, n_bobs 1..3, any built-in right-hand side or a user one with n_bmeas = 1; cfg->flags must carry RK_FLAG_BATCH_MINOR.
 * What is not served is refused on cfg (and n_bobs) alone -- RK_ERR_INVALID (a non-positive size, RK_FLAG_BATCH_MINOR missing)
 * or RK_ERR_UNSUPPORTED -- before the handle or any pointer is looked at; then n_draws (1..65535) and n_keep (RK_ERR_INVALID). */
int rk_solve_sim_draws_grid(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out,
                            const rk_grid_in* g, int32_t n_draws, const int32_t* keep, int32_t n_keep, double* x_draws);
int rk_dalton_grid_sim_draws(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out,
                             const double* obs, const double* obs_weight, const double* obs_var, const int32_t* obs_ind,
                             int32_t n_obs, int32_t n_bobs, const rk_grid_in* g, int32_t n_draws, const int32_t* keep,
                             int32_t n_keep, double* x_draws);

/* dalton_at: rk_dalton_loglik for observations whose times need not be grid nodes (an addition: the reference places every
 * observation by searchsorted on the grid).  obs / obs_weight / obs_var as for rk_dalton_loglik, in time order.  The device
 * array `table` (n_obs, 4) holds per observation: node, off-grid flag, pre slot, post slot or -1.  With the flag clear the
 * observation sits on grid node `node` (0..n_steps) and is handled as by rk_dalton_loglik (node 0: the joint density only).
 * With it set the time lies in (t_node, t_node+1): the joint filter predicts over the gap since the previous event (node or
 * observation) with the prior pair (pre_trans, pre_noise)[pre slot], conditions on y, and after the interval's last
 * observation -- the one whose fourth entry is not -1 -- predicts on to t_node+1 with (post_trans, post_noise)[post slot];
 * the interrogation and the z update at node + 1 follow as always.  The marginal filter takes the same split predictions
 * without the conditioning.  Entries must be ordered in time, the off-grid ones of an interval adjacent.  Pairs are
 * (n, d, p, p) row-major, or (n, d, p, p, B) batch-minor with prior_batched; n_pre and n_post are at least 1 (also when
 * no slot is used) and slots are clamped to them.  Served range, routes and RK_DALTON_LANES as for rk_dalton_loglik
 * (kernels: dalton_at_tile3_kernels.hpp / dalton_at_kernels.hpp); logdens (B) is overwritten.                           */
typedef struct {
    const int32_t* table;                                /* (n_obs, 4) on the device                              */
    int32_t        n_pre, n_post;                        /* pairs in pre_* / post_* (each at least 1)             */
    const double  *pre_trans, *pre_noise;                /* (n_pre, d, p, p [,B]): Q, R over the gap before an observation   */
    const double  *post_trans, *post_noise;              /* (n_post, d, p, p [,B]): Q, R from the last observation to the node */
    int32_t        prior_batched;
} rk_dalton_at_in;
int rk_dalton_loglik_at(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in,
                        const double* obs, const double* obs_weight, const double* obs_var, const rk_dalton_at_in* at,
                        int32_t n_obs, int32_t n_bobs, double* logdens);

/* fenrir_at: rk_fenrir_backward for observations whose times need not be grid nodes (an addition), after rk_solve_filter with the
 * same cfg / in.  obs / obs_weight / obs_var as for rk_fenrir_backward, in time order; `at` is rk_dalton_loglik_at's table and
 * prior pairs.  Fenrir's forward pass is free of data, so an observation in (t_node, t_node+1) adds hops to the backward Markov
 * chain: with the interval's observations 1..k, the forward moments at their times are predictions from filt[node] over the
 * pre pairs, hop j (over pre pair j+1, or the post pair for j = k) is the smooth_cond map (standard.py:366-370) between two
 * neighbouring events, and the chain runs from node+1 down to node through the hops k..0, conditioning on y_j after hop j >= 1.
 * The hop records are evaluated time-parallel into `workspace` first (rk_fenrir_at_workspace_bytes with n_records = n_pre +
 * n_post; released by the caller after the call).  Served: kalman_type standard; the RK_LAYOUT_TILE3 records (no flags,
 * n_bstate = 3, n_bobs = 1) or the batch-minor filtered and predicted moments (RK_FLAG_STORE_PRED | RK_FLAG_BATCH_MINOR, n_bstate
 * 2..6, n_bobs 1..3).  Everything else -- the square-root form, n_bstate 7 and 8, the blocked-tile records -- is refused with
 * RK_ERR_UNSUPPORTED on the configuration alone, before the handle or any pointer is looked at.  logdens (B) is overwritten.  */
typedef rk_dalton_at_in rk_fenrir_at_in;
int rk_fenrir_at_workspace_bytes(const rk_solve_cfg* cfg, int32_t n_bobs, int32_t n_records, size_t* bytes);
int rk_fenrir_backward_at(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out,
                          const double* obs, const double* obs_weight, const double* obs_var, const rk_fenrir_at_in* at,
                          int32_t n_obs, int32_t n_bobs, void* workspace, double* logdens);

/* DALTON for non-Gaussian observations (src/rodeo/inference/dalton.py:547-1039, kalman_type = standard, n_bmeas = 1,
 * n_bstate 2..6 (2..5 with three or more blocks), interrogate rodeo / schober / kramer, any built-in or user right-hand side
 * with n_bmeas = 1).  The observation log-likelihood is HIP source, like a user right-hand side:
 * rk_register_obs_source: `source` defines, inside namespace rk, a struct `type_name` with constants D, P, NY, NTHETA, MO,
 * NACT[D], ACT[D][3] (the state components of each block that the log-likelihood reads, at most n_active = MO <= 3 per
 * block) and `template <class T> static T loglik(const double (&y)[D][NY], const T (&X)[D][P], double ind, const double
 * (&th)[NTHETA])` (rodeo_amd.trace.trace_obs_source writes it from a Python function); returns obs_id.  n_theta is the
 * solver's cfg.n_theta: the log-likelihood reads the same packed parameters as the right-hand side.  Every call registers a
 * new model, kept with its compiled kernels for the life of the process (nothing is pruned or compared): register a source
 * once and reuse its obs_id (the Python wrapper keys its models by a hash of the source).
 * Observations: obs (n_obs, n_block, n_ycols) and obs_ind (n_obs) on the device, grid indices strictly increasing and at
 * most n_steps; an observation at grid index 0 enters the log-likelihood term only.
 * rk_daltonng_loglik: logy_x + logx_z - logx_yhat per trajectory into logdens (B); needs a device workspace of
 * rk_daltonng_workspace_bytes (two filters' moments, the gain records, the smoothed means at the observations); a point
 * where the log-likelihood is not concave in a block's active components yields NaN, not an error.
 * rk_daltonng_solve: the joint filter (RK_MODE_FILTER) + the smoothing pass of rk_solve_mv (RK_MODE_MV) into `out` in the
 * batch-minor layout (refused unless rk_solve_layout reports it: set RK_FLAG_BATCH_MINOR).                               */
int rk_register_obs_source(const char* type_name, const char* source, int32_t n_block, int32_t n_bstate, int32_t n_ycols,
                           int32_t n_theta, int32_t n_active, int32_t* obs_id);
/* compiles the three kernels around obs_id (both forward forms for this right-hand side and interrogation, and the
 * observation kernel) without loading them (needs no GPU); compiler errors via rk_last_error() */
int rk_obs_compile_check(int32_t obs_id, int32_t rhs_id, int32_t interrogate);
int rk_daltonng_workspace_bytes(const rk_solve_cfg* cfg, int32_t n_obs, size_t* bytes);
int rk_daltonng_loglik(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, int32_t obs_id, const double* obs,
                       const int32_t* obs_ind, int32_t n_obs, void* workspace, size_t workspace_bytes, double* logdens);
int rk_daltonng_solve(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out, int32_t mode,
                      int32_t obs_id, const double* obs, const int32_t* obs_ind, int32_t n_obs);
/* daltonng_grid (an addition): rk_daltonng_loglik / rk_daltonng_solve on rk_solve_grid's non-uniform grid, every observation on a
 * node.  obs_id and obs as for rk_daltonng_loglik; obs_node (n_obs) holds the NODE of every observation, strictly increasing in
 * 0..n_steps: node 0 enters the log-likelihood term only, a node above n_steps never matches.  Step n -> n + 1 of the joint
 * filter: the prediction with (q, r)[slot[n]], the interrogation at t[n+1], the z update, then -- if node n + 1 is observed -- the
 * conditioning on the pseudo-observation expanded at the predicted mean (z first, yhat second, as rk_daltonng_loglik).  The two
 * backward conditionals at node n re-evaluate the prediction and the gain from filt[n] with (q, r)[slot[n]].
 * rk_daltonng_grid_loglik: logy_x + logx_z - logx_yhat per trajectory into logdens (B); `workspace` is rk_daltonng_workspace_bytes's,
 * the same layout, checked before any launch.  A non-concave point yields NaN, not an error.
 * rk_daltonng_grid_solve: the joint filter's moments into out->mean_state / var_state (mode = RK_MODE_FILTER), then rk_solve_grid's
 * smoothing pass (RK_MODE_MV); RK_LAYOUT_BATCH_MINOR.
 * Served: what rk_daltonng_loglik serves; cfg->flags must carry RK_FLAG_BATCH_MINOR and not RK_FLAG_STORE_PRED.  What is not served
 * is refused on cfg, mode and the registered model alone -- RK_ERR_INVALID (a non-positive size, another mode,
 * RK_FLAG_BATCH_MINOR missing, a model registered for another configuration) or RK_ERR_UNSUPPORTED -- before the handle or any
 * pointer is looked at.
 * rk_obs_grid_compile_check: compiles the two forward forms of the grid filter around obs_id for this right-hand side and
 * interrogation without loading them (needs no GPU; RK_JIT_VERBOSE prints each build's registers, scratch and LDS).            */
int rk_obs_grid_compile_check(int32_t obs_id, int32_t rhs_id, int32_t interrogate);
int rk_daltonng_grid_loglik(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, int32_t obs_id, const double* obs,
                            const int32_t* obs_node, int32_t n_obs, const rk_grid_in* g, void* workspace, size_t workspace_bytes,
                            double* logdens);
int rk_daltonng_grid_solve(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out, int32_t mode,
                           int32_t obs_id, const double* obs, const int32_t* obs_node, int32_t n_obs, const rk_grid_in* g);
/* The same on the records of the blocked-tile forward pass (kalman_type standard, n_bstate 4 .. 8, rk_solve_filter WITHOUT
 * RK_FLAG_STORE_PRED | RK_FLAG_BATCH_MINOR: out->var_state = the records): predicted moments are re-evaluated, nothing but the
 * filtered records is read; the result goes to mean_out (N+1, d, p, B) and var_out (N+1, d, p, p, B), batch-minor.
 * Replaces the same reference lines as rk_fenrir_solve_mv (src/rodeo/inference/fenrir.py:333-457).                        */
int rk_fenrir_solve_mv_tiles(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, const rk_solve_out* out,
                             const double* obs, const double* obs_weight, const double* obs_var, const int32_t* obs_ind,
                             int32_t n_obs, int32_t n_bobs, void* workspace, double* mean_out, double* var_out);

/* MAGI log-density (src/rodeo/inference/magi.py:6-99): the Kalman filter of the prior X_n = Q X_{n-1} + N(0, R) per block,
 * started from the known state x_0 = ode_state[0], that measures the first n_active components of every X_n exactly
 * (W = eye(n_active, p), no measurement offset or noise); logdens[b] = the sum over steps and blocks of the forecast's
 * Gaussian log-density (Cholesky form, not the eigenvalue rule of rk_fenrir_backward) at x_meas.  No right-hand side, no
 * interrogation: the caller supplies the data.  kalman_type = RK_KALMAN_STANDARD (LU gain of standard.py:93-102) or
 * RK_KALMAN_SQRT (square_root.py:30-101, 317-345: prior_var holds lower factors).  Served: n_bstate 2..6 (standard) or
 * 2..7 (square-root; beyond, the lane kernel spills), n_active 1..n_bstate, any n_block; n_steps = 0 gives 0.  One lane per
 * (trajectory, block); with n_block > 1 the block sums go to the handle's grow-only device scratch (n_block * B doubles,
 * allocated when it grows) and a second kernel adds them in block order (no atomics): the result is the same bits from
 * run to run.  logdens (B) is overwritten.  With n_active >= 2 and a coupled prior_weight (IBM priors included) the
 * standard form's covariance loses its symmetry by amplified rounding, as in the reference: RK_KALMAN_SQRT is the form
 * to use there.                                                                                                        */
typedef struct {
    int32_t n_traj;       /* B                                                                             */
    int32_t n_steps;      /* N: ode_state has N + 1 time points                                            */
    int32_t n_block;      /* d = n_vars                                                                    */
    int32_t n_bstate;     /* p = n_deriv                                                                   */
    int32_t n_active;     /* measured components per block, 1 .. p                                         */
    int32_t kalman_type;  /* RK_KALMAN_*                                                                   */
} rk_magi_cfg;

typedef struct {
    const double* x0;            int32_t x0_batched;            /* ode_state[0]  (d, p [,B])                   */
    const double* x_meas;        int32_t x_meas_batched;        /* ode_state[1:, :, :n_active]  (N, d, n_active [,B]) */
    const double* prior_weight;  int32_t prior_weight_batched;  /* Q  (d, p, p [,B])   prior_pars[0]            */
    const double* prior_var;     int32_t prior_var_batched;     /* R or its lower factor (d, p, p [,B])         */
} rk_magi_in;

int rk_magi_logdens(rk_handle h, const rk_magi_cfg* cfg, const rk_magi_in* in, double* logdens);

/* Laplace approximation of a k-parameter log-posterior by central differences (rodeo_amd/inference/laplace.py replaces
 * jax.grad / jax.hessian of docs/examples/parameter.md:239-275).  Device arrays, row-major, centre axis first; k <= 12
 * (RK_ERR_UNSUPPORTED beyond).  S = 2 k^2 + 1 stencil points per centre, in this order:
 *     s = 0                        u
 *     s = 1 + 2 i,  2 + 2 i        u + h_i e_i,  u - h_i e_i                                 i = 0 .. k-1
 *     s = 1 + 2 k + 4 q + 0 .. 3   u + h_i e_i + h_j e_j, u + h_i e_i - h_j e_j, u - h_i e_i + h_j e_j, u - h_i e_i - h_j e_j
 *                                  for the pairs i < j in row-major order (0,1), (0,2), .., (k-2,k-1), q = 0, 1, ..
 * rk_fd_stencil writes the points: u (C, k), step (k) -> out (C, S, k).
 * rk_fd_grad_hess turns the values vals (C, S) of the log-posterior at those points into grad (C, k) =
 * (f(+i) - f(-i)) / (2 h_i) and hess (C, k, k): diagonal ((f(+i) - f(0)) + (f(-i) - f(0))) / h_i^2, off the diagonal
 * ((f(++) - f(+-)) - (f(-+) - f(--))) / (4 h_i h_j), both triangles from the same expression.  Each entry is one fixed
 * expression (no atomics): identical bits from call to call.  n_bad (C) counts the centre's non-finite values; where it is
 * not 0 the centre's grad and hess are NaN.
 * rk_newton_step: per centre the Cholesky factor of -hess + damping[c] I, delta (C, k) = (-hess + damping I)^{-1} grad,
 * logdet (C) = log det(-hess + damping I), ok (C) = 1; a pivot that is not positive gives ok = 0 and NaN in delta and
 * logdet.  The three kernels are latency-bound and not tuned.                                                        */
int rk_fd_stencil(rk_handle h, int32_t n_centre, int32_t k, const double* u, const double* step, double* out);
int rk_fd_grad_hess(rk_handle h, int32_t n_centre, int32_t k, const double* vals, const double* step, double* grad,
                    double* hess, int32_t* n_bad);
int rk_newton_step(rk_handle h, int32_t n_centre, int32_t k, const double* grad, const double* hess, const double* damping,
                   double* delta, double* logdet, int32_t* ok);

/* The gradient mode of the same driver (laplace_grad): the caller supplies value AND exact gradient of the log-posterior,
 * the Hessian is a first central difference of gradients.  S' = 2 k + 1 points per centre: the leading S' points of
 * rk_fd_stencil (u, then u + h_i e_i, u - h_i e_i), in its order and with its arithmetic, so the rows are its rows bit for
 * bit.  Refusals as above (n_centre < 1 or k < 1: RK_ERR_INVALID; k > 12: RK_ERR_UNSUPPORTED).
 * rk_fd_grad_stencil writes the points: u (C, k), step (k) -> out (C, S', k).
 * rk_fd_hess_from_grad: vals (C, S'), grads (C, S', k) with G[s] the gradient at point s ->
 *     grad (C, k)     = G[0]
 *     hess (C, k, k):   diagonal (G[1+2i][i] - G[2+2i][i]) / (2 h_i); off the diagonal, a = min(i, j), b = max(i, j),
 *                       0.5 ((G[1+2a][b] - G[2+2a][b]) / (2 h_a) + (G[1+2b][a] - G[2+2b][a]) / (2 h_b)),
 *                       both triangles from the same expression
 *     grad_fd (C, k)  = (vals[1+2i] - vals[2+2i]) / (2 h_i), the difference quotient the driver checks G[0] against
 *     n_bad (C)       the count of non-finite entries of vals and grads of the centre; where it is not 0 the centre's
 *                     grad, hess and grad_fd are NaN.
 * One fixed expression per entry (no atomics): identical bits from call to call.  Latency-bound, not tuned.          */
int rk_fd_grad_stencil(rk_handle h, int32_t n_centre, int32_t k, const double* u, const double* step, double* out);
int rk_fd_hess_from_grad(rk_handle h, int32_t n_centre, int32_t k, const double* vals, const double* grads,
                         const double* step, double* grad, double* hess, double* grad_fd, int32_t* n_bad);

/* ---- per-step operator boundary -------------------------------------------------------------------------
 * Batched versions of the nine functions of src/rodeo/kalmantv/standard.py (kalman_type = RK_KALMAN_STANDARD)
 * and src/rodeo/kalmantv/square_root.py (RK_KALMAN_SQRT).  n = batch size (the reference's vmap axis);
 * every array is batch-minor: vectors (n_state, n), matrices (rows, cols, n).  A NULL optional input means 0.
 * Names of the arguments are the reference's keyword names.  Any n_state up to 768: one lane per item up to 16, one
 * 512-thread workgroup per item on the dense solver's GEMM / LU / QR blocks beyond (the reference's operators are
 * size-agnostic, standard.py:31-60); the large-block path keeps a grow-only device scratch on the handle.              */
typedef struct {
    int32_t n;            /* batch                                                                         */
    int32_t n_state;
    int32_t n_meas;
    int32_t kalman_type;
} rk_op_cfg;

/* standard.py:31-60 / square_root.py:30-58 */
int rk_kalman_predict_batched(rk_handle h, const rk_op_cfg* c,
        const double* mean_state_past, const double* var_state_past, const double* mean_state,
        const double* wgt_state, const double* var_state,
        double* mean_state_pred, double* var_state_pred);
/* standard.py:63-103 / square_root.py:61-101 */
int rk_kalman_update_batched(rk_handle h, const rk_op_cfg* c,
        const double* mean_state_pred, const double* var_state_pred, const double* x_meas,
        const double* mean_meas, const double* wgt_meas, const double* var_meas,
        double* mean_state_filt, double* var_state_filt);
/* standard.py:106-157 / square_root.py:104-155 */
int rk_kalman_filter_batched(rk_handle h, const rk_op_cfg* c,
        const double* mean_state_past, const double* var_state_past, const double* mean_state,
        const double* wgt_state, const double* var_state, const double* x_meas,
        const double* mean_meas, const double* wgt_meas, const double* var_meas,
        double* mean_state_pred, double* var_state_pred, double* mean_state_filt, double* var_state_filt);
/* standard.py:180-217 / square_root.py:178-219 (var_state = R factor is required for RK_KALMAN_SQRT) */
int rk_kalman_smooth_mv_batched(rk_handle h, const rk_op_cfg* c,
        const double* mean_state_next, const double* var_state_next,
        const double* mean_state_filt, const double* var_state_filt,
        const double* mean_state_pred, const double* var_state_pred,
        const double* wgt_state, const double* var_state,
        double* mean_state_smooth, double* var_state_smooth);
/* standard.py:220-255 / square_root.py:222-261 */
int rk_kalman_smooth_sim_batched(rk_handle h, const rk_op_cfg* c,
        const double* x_state_next,
        const double* mean_state_filt, const double* var_state_filt,
        const double* mean_state_pred, const double* var_state_pred,
        const double* wgt_state, const double* var_state,
        double* mean_state_sim, double* var_state_sim);
/* standard.py:258-305 / square_root.py:264-314 */
int rk_kalman_smooth_batched(rk_handle h, const rk_op_cfg* c,
        const double* x_state_next, const double* mean_state_next, const double* var_state_next,
        const double* mean_state_filt, const double* var_state_filt,
        const double* mean_state_pred, const double* var_state_pred,
        const double* wgt_state, const double* var_state,
        double* mean_state_sim, double* var_state_sim, double* mean_state_smooth, double* var_state_smooth);
/* standard.py:308-336 / square_root.py:317-345 */
int rk_kalman_forecast_batched(rk_handle h, const rk_op_cfg* c,
        const double* mean_state_pred, const double* var_state_pred,
        const double* mean_meas, const double* wgt_meas, const double* var_meas,
        double* mean_fore, double* var_fore);
/* standard.py:339-371 / square_root.py:348-385 */
int rk_kalman_smooth_cond_batched(rk_handle h, const rk_op_cfg* c,
        const double* mean_state_filt, const double* var_state_filt,
        const double* mean_state_pred, const double* var_state_pred,
        const double* wgt_state, const double* var_state,
        double* wgt_state_cond, double* mean_state_cond, double* var_state_cond);

/* ---- interrogation boundary ------------------------------------------------------------------------------
 * One interrogation for a batch of predicted states: src/rodeo/interrogate.py (all four variants; the variant,
 * rhs, dims, seed and traj_offset are taken from cfg; `step` addresses the Philox stream for chkrebtii).
 *   mean_state_pred (d, p, B), var_state_pred (d, p, p, B), ode_weight/theta as in rk_solve_in;
 *   outputs wgt_meas (d, m, p, B), mean_meas (d, m, B), var_meas (d, m, m, B); any n_bmeas m for a registered
 *   right-hand side.  cfg->kalman_type = RK_KALMAN_SQRT matters to chkrebtii only (interrogate.py:35-42, m = 1):
 *   var_state_pred is then the factor L-, var_meas = W L- has shape (d, 1, p, B) and the draw is mu- + (W L-) z.  */
int rk_interrogate_batched(rk_handle h, const rk_solve_cfg* cfg, const rk_solve_in* in, double t, int32_t step,
        const double* mean_state_pred, const double* var_state_pred,
        double* wgt_meas, double* mean_meas, double* var_meas);

/* ---- multi-GPU: batch sharding over RCCL / xGMI --------------------------------------------------------------
 * The path shards by independent trajectories (no data-path collective).  The only exchange is the all-gather of
 * per-trajectory scalars (e.g. log-posteriors).  uid is an opaque 128-byte ncclUniqueId made on rank 0 and
 * distributed by the host launcher.                                                                           */
#define RK_COMM_UID_BYTES 128
int rk_comm_uid(void* uid128);
int rk_comm_init(rk_handle h, int rank, int nranks, const void* uid128);
int rk_comm_destroy(rk_handle h);
int rk_allgather_f64(rk_handle h, const double* send_dev, double* recv_dev, size_t count_per_rank);
int rk_allreduce_max_f64(rk_handle h, const double* send_dev, double* recv_dev, size_t count);
int rk_comm_barrier(rk_handle h);

#ifdef __cplusplus
}
#endif
#endif /* RODEO_KALMAN_H */
