"""
Gaussian observation log-likelihood (+ optional normal log-prior) per trajectory, reduced on the device from a solver
output that is still resident in HBM -- the tail of rodeo's user-level log-posteriors:

    obs_ind  = searchsorted(sim_times, obs_times)                          docs/examples/parameter.md:149
    loglik   = sum norm.logpdf(obs, loc = Xt[obs_ind, :, 0], scale = noise_sd)    parameter.md:197-210
    logprior = sum norm.logpdf(upars[:n_prior], 0, prior_sd)               parameter.md:188-194

Only B doubles leave the GPU instead of the (B, N+1, d, p) path.
"""
import ctypes as C
import numpy as np
from .. import _lib
from ..solve import TILE_LAYOUTS


def obs_index(t_min, t_max, n_steps, obs_times):
    """Indices of the solver grid closest-from-the-right to the observation times (``jnp.searchsorted``)."""
    sim_times = np.linspace(t_min, t_max, n_steps + 1)
    return np.searchsorted(sim_times, np.asarray(obs_times, dtype=np.float64)).astype(np.int32)


def check_obs(obs_data, obs_ind, d, n_steps):
    """
    The observations as the kernels read them: ``(obs (n_obs, d) float64, ind (n_obs,) int32)``, both C-contiguous, with
    ``ind`` ASCENDING.  Raises ``ValueError`` for a shape other than (n_obs, d) / (n_obs,) or an index outside [0, n_steps].
    Indices may come in any order (the reference's ``Xt[obs_ind]`` takes any): where they descend somewhere they are sorted
    -- a stable sort, so repeated indices keep their order -- with the rows of ``obs`` carried along.  The sampler that
    reduces the log-posterior itself (bwd_sim_tile3_kernel<true>) walks the indices from the end and needs them ascending.
    """
    obs = np.ascontiguousarray(obs_data, dtype=np.float64)
    ind = np.ascontiguousarray(obs_ind, dtype=np.int32)
    if ind.ndim != 1 or obs.shape != (ind.shape[0], d):
        raise ValueError(f"obs_data must have shape (n_obs, {d}) and obs_ind (n_obs,)")
    if ind.size and (ind.min() < 0 or ind.max() > n_steps):
        raise ValueError("obs_ind outside the solver grid")
    if np.any(np.diff(ind) < 0):
        order = np.argsort(ind, kind="stable")
        obs, ind = np.ascontiguousarray(obs[order]), np.ascontiguousarray(ind[order])
    return obs, ind


def gauss_obs_logpost(plan, obs_data, obs_ind, noise_sd, upars=None, prior_sd=10.0, n_prior=None, which="auto",
                      reuse_out=False):
    """
    ``plan``: a ``SolvePlan`` whose ``mv()`` / ``sim()`` has been launched.  ``obs_data`` (n_obs, d), ``obs_ind``
    (n_obs,) int; ``upars`` (B, k) optional unconstrained parameters whose first ``n_prior`` entries get a
    N(0, prior_sd^2) prior.  Returns a DeviceArray of shape (B,) (call ``.to_host()``): a fresh one, or -- with
    ``reuse_out=True`` -- one of four buffers owned by the plan that later calls overwrite in turn.  ``obs_ind`` may come in
    any order (``check_obs``).  ``which``: "x" reduces over the path of the last sampler launch and raises ``RuntimeError``
    when that launch stored none (a path-less ``sim_logpost``), "mean" over the moments of the last filter() / mv(), "auto"
    picks "x" after a sampler launch.
    """
    dev = plan.dev
    obs, ind = check_obs(obs_data, obs_ind, plan.d, plan.N)
    if which == "auto":                  # (after a path-less sim_logpost it is "x" too, and raises: no stale path, no filter mean)
        which = "x" if plan.last_mode == _lib.MODE_SIM else "mean"
    if which == "x":
        plan._require_path()
        state, layout = plan.x_state, _lib.LAYOUT_BATCH_MINOR
    else:
        layout = plan.records_layout                 # (RK_LAYOUT_TILE3_PACKED after a packing mv(): the kernel reads both forms)
        state = plan.var_state if plan.layout in TILE_LAYOUTS else plan.mean_state
    # per call one upload (upars) and one kernel
    d_obs, d_ind, d_up, k = _staged(plan, obs, ind, upars, n_prior)
    # The result is a fresh device array unless the caller opts into `reuse_out`: then it comes from the plan's ring of four
    # (``SolvePlan.result_ring``) -- for callers that read the result at once (FitzLogPosterior, basic).
    out = plan.result_ring() if reuse_out else dev.empty((plan.B,))
    _lib.check(dev.lib.rk_gauss_obs_logpost(dev.h, plan.B, plan.N, plan.d, plan.p, layout, state.ptr, d_obs.ptr,
                                            d_ind.ptr, ind.shape[0], float(noise_sd),
                                            d_up.ptr if d_up is not None else None, k, float(prior_sd), out.ptr))
    return out


def _staged(plan, obs, ind, upars, n_prior):
    """Device copies of the checked observations / indices (``SolvePlan.staged``: a pseudo-marginal chain calls once per step
    with the same data) and of the transposed parameters: ``(d_obs, d_ind, d_upars or None, n_prior)``."""
    d_obs, d_ind = plan.staged("logpost", obs, ind)
    d_up, k = None, 0
    if upars is not None:           # (a DeviceArray (n_prior, B) from stage_upars() is already staged)
        d_up = upars if hasattr(upars, "ptr") else stage_upars(plan, upars, n_prior)
        k = int(d_up.shape[0])
    return d_obs, d_ind, d_up, k


def stage_upars(plan, upars, n_prior=None):
    """The first ``n_prior`` unconstrained parameters of every trajectory as a device array (n_prior, B), batch-minor: what the
    reduction reads.  Upload it together with the plan's other inputs (``SolvePlan.update``), BEFORE the kernels are launched."""
    up = np.asarray(upars, dtype=np.float64)
    k = up.shape[1] if n_prior is None else int(n_prior)
    upt = np.ascontiguousarray(up[:, :k].T)
    if plan.upars_dev is None or tuple(plan.upars_dev.shape) != upt.shape:
        plan.upars_dev = plan.dev.to_device(upt)
    else:
        plan.upars_dev.upload(upt)                    # (they change with every call: one buffer, overwritten in place)
    return plan.upars_dev


def sim_logpost(plan, key, obs_data, obs_ind, noise_sd, upars=None, prior_sd=10.0, n_prior=None, keep_path=False):
    """
    ``plan.sim(key)`` followed by ``gauss_obs_logpost`` on its path as ONE device call (``rk_solve_sim_logpost``): the body of
    the log-posterior of docs/examples/parameter.md:331-354.  Everything the kernels read is uploaded BEFORE the launch (an
    upload between sampler and reduction left the GPU idle for 30 of C4's 275 us per evaluation); on the n_bstate = 3 tile
    path the backward sampler reduces the log-posterior itself and, unless ``keep_path``, stores no path at all.
    Returns a DeviceArray (B,) from a ring of four buffers owned by the plan (overwritten by the fourth call after this one).

    ``obs_ind`` may come in any order, as in the reference's ``Xt[obs_ind]``: unsorted indices are sorted here (stably, rows of
    ``obs_data`` carried along, ``check_obs``) before they are cached and uploaded, because the fused sampler needs them
    ascending -- the C entry ``rk_solve_sim_logpost`` REQUIRES ascending indices on that route (include/rodeo_kalman.h).
    A path-less call (the fused route without ``keep_path``) invalidates ``plan.x_state``: the path an earlier ``plan.sim``
    left there is not this draw's, so ``plan.x_host()`` and ``gauss_obs_logpost(plan, ..., which="x" / "auto")`` raise
    ``RuntimeError`` until a ``plan.sim`` or a ``sim_logpost(..., keep_path=True)`` has written a path again.
    """
    obs, ind = check_obs(obs_data, obs_ind, plan.d, plan.N)
    d_obs, d_ind, d_up, k = _staged(plan, obs, ind, upars, n_prior)
    n_obs, out = ind.shape[0], plan.result_ring()
    # the fused sampler stores no path unless asked to: the launch then neither allocates nor writes x_state
    plan.launch(plan.dev.lib.rk_solve_sim_logpost, key, _lib.MODE_SIM, d_obs.ptr, d_ind.ptr, n_obs, float(noise_sd),
                d_up.ptr if d_up is not None else None, k, float(prior_sd), out.ptr,
                path=keep_path or not _fused_supported(plan, n_obs))
    return out


def _fused_supported(plan, n_obs):
    """Mirror of tile3_sim_logpost_supported (csrc/solve_tile3.hip): the configurations whose sampler reduces the log-posterior."""
    lay = C.c_int32(0)
    _lib.check(plan.dev.lib.rk_solve_layout(C.byref(plan.cfg), _lib.MODE_SIM, C.byref(lay)))
    return lay.value == _lib.LAYOUT_TILE3 and plan.d in (1, 2, 4) and n_obs <= 512 and n_obs * plan.d <= 1024
