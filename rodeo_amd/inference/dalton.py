"""
``rodeo.inference.dalton`` for Gaussian observations (src/rodeo/inference/dalton.py:39-545):
  * ``dalton``: the DALTON approximate log-likelihood log p(Y_{0:M} | Z_{1:N}) = logdens_joint - logdens_marg, the log-density
    of a filter that conditions on the ODE residuals Z and the observations Y minus that of a filter on Z alone (:39-235);
  * ``solve_mv``: the data-adaptive solver, mean and variance of p(X_{0:N} | Z_{1:N}, Y_{0:M}) -- the joint filter followed by
    the solver's own smoothing pass (:374-460);
  * ``solve_sim``: the same filter followed by the solver's sampler (:463-545).
All of it runs on the device (``rk_dalton_loglik`` / ``rk_dalton_solve``): both filters of every parameter set in one
kernel launch for ``dalton`` (only B doubles come back), the joint filter's moments and the solver's own backward kernels
for ``solve_mv`` / ``solve_sim``.  At n_bstate = 3 with one observation per block and up to four blocks the filters run
on the MFMA tiles (``dalton_tile3_kernels.hpp``, RK_LAYOUT_TILE3 records), elsewhere on lane-per-trajectory kernels
(``dalton_kernels.hpp``, batch-minor moments); ``RK_DALTON_LANES=1`` forces the lanes.

Same signatures as the reference.  Extension as in ``fenrir``: a leading batch axis on ``ode_init`` / ``prior_pars`` /
``**params`` (observations are shared) returns an array (B,) or batched states.  Observations per block: n_bobs = 1 .. 3
(``obs_data`` (n_obs, n_block, n_bobs), ``obs_weight`` (n_obs, n_block, n_bobs, n_bstate), ``obs_var`` (n_obs, n_block, n_bobs,
n_bobs)).  Served: kalman_type "standard", n_bmeas = 1, n_bstate 2 .. 6 (2 .. 5 with three or more blocks), interrogate rodeo /
schober / kramer.  What the arguments' shapes and the interrogation decide is refused before any device work; what depends on
the right-hand side (its block count, the n_bstate limit of three or more blocks) is refused by the library once the plan is
built.  Divergences from the reference:
  * the grid indices of the observations on the grid (index <= n_steps) must be strictly increasing (ValueError): the
    reference silently drops every observation after a repeated or unsorted index;
  * y is conditioned on after z within a step instead of on the stacked measurement: the same value up to rounding unless a
    forecast variance lies within utils.py:60-78's 1e-8 threshold.
"""
import ctypes as C
import os
import numpy as np
from .. import _lib
from ..solve import cached_plan, _interrogate_id, _seed
from .fenrir import _check_obs
from .logpost import obs_index


def _refusals(ode_weight, interrogate, kalman_type, obs_data, obs_weight, obs_var, t_min, t_max, n_steps, obs_times):
    """Everything this build does not serve, raised before any device work; returns (obs, D, Omega, n_bobs, obs_ind)."""
    if kalman_type == "square-root":
        raise NotImplementedError("dalton: the square-root form is not built on the device (kalman_type='standard' only)")
    if kalman_type != "standard":
        raise NotImplementedError                                   # dalton.py:83-88
    itg, _ = _interrogate_id(interrogate)
    if itg == _lib.INTERROGATE_CHKREBTII:
        raise NotImplementedError("dalton: interrogate_chkrebtii is not supported (rodeo, schober, kramer)")
    W = np.shape(ode_weight)
    if len(W) not in (3, 4):
        raise ValueError("ode_weight must have shape (n_block, n_bmeas, n_bstate) [+ a leading batch axis]")
    if W[-2] != 1:
        raise NotImplementedError("dalton on the device: n_bmeas = 1 only (the dense / indep_init form is not served)")
    if not 2 <= W[-1] <= 6:
        raise NotImplementedError("dalton on the device: n_bstate in 2..6")
    obs, D, Om, n_bobs = _check_obs(obs_data, obs_weight, obs_var)
    if D.shape[1:] != (W[-3], n_bobs, W[-1]):
        raise ValueError(f"obs_weight must have shape (n_obs, {W[-3]}, n_bobs, {W[-1]})")
    ind = obs_index(t_min, t_max, n_steps, obs_times)
    on_grid = ind[ind <= int(n_steps)]                              # (later times never match, here or in the reference)
    if np.any(np.diff(ind) < 0) or np.any(np.diff(on_grid) == 0):
        raise ValueError("dalton: the observations' grid indices must be strictly increasing (one observation per grid "
                         "point, in time order)")
    return obs, D, Om, n_bobs, ind


def _obs_on_device(plan, obs, D, Om, ind):
    """The observations uploaded once per plan and reused while they do not change (a sampler calls dalton in a loop)."""
    cache = plan.__dict__.setdefault("_dalton_obs", {})
    sig = (obs.tobytes(), D.tobytes(), Om.tobytes(), ind.tobytes())
    if cache.get("sig") != sig:
        cache["sig"] = sig
        cache["dev"] = tuple(plan.dev.to_device(np.ascontiguousarray(a)) for a in (obs, D, Om, ind.astype(np.int32)))
    return cache["dev"]


def _plan(args, params, mode, n_bobs):
    """The cached plan whose output layout is the one rk_dalton_solve writes: without flags where the tile route may serve
    (n_bstate = 3, one observation per block), else with RK_FLAG_BATCH_MINOR; checked against rk_dalton_layout."""
    p, d = int(np.shape(args[1])[-1]), int(np.shape(args[1])[-3])
    tiles = p == 3 and n_bobs == 1 and d <= 4 and os.environ.get("RK_DALTON_LANES", "0") in ("", "0")
    plan = cached_plan(*args, batch_minor=not tiles, **params)
    want, lay = C.c_int32(0), C.c_int32(0)
    _lib.check(plan.dev.lib.rk_dalton_layout(C.byref(plan.cfg), mode, n_bobs, C.byref(want)))
    _lib.check(plan.dev.lib.rk_solve_layout(C.byref(plan.cfg), mode, C.byref(lay)))
    if lay.value != want.value:                                     # (e.g. a user right-hand side without a tile form)
        plan = cached_plan(*args, batch_minor=True, **params)
    return plan


def dalton(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
           obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", **params):
    """log p(Y_{0:M} | Z_{1:N}) (dalton.py:39-235): a float, or an array (B,) for batched inputs."""
    obs, D, Om, n_bobs, ind = _refusals(ode_weight, interrogate, kalman_type, obs_data, obs_weight, obs_var, t_min, t_max,
                                        n_steps, obs_times)
    plan = _plan((ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type), params,
                 _lib.MODE_FILTER, n_bobs)
    d_obs, d_w, d_v, d_ind = _obs_on_device(plan, obs, D, Om, ind)
    plan.cfg.seed = _seed(key)
    out = plan.dev.empty((plan.B,))
    _lib.check(plan.dev.lib.rk_dalton_loglik(plan.dev.h, C.byref(plan.cfg), C.byref(plan.inp), d_obs.ptr, d_w.ptr, d_v.ptr,
                                             d_ind.ptr, int(ind.shape[0]), n_bobs, out.ptr))
    ll = out.to_host()
    return ll if plan.batched else float(ll[0])


def _solve(mode, key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
           obs_data, obs_times, obs_weight, obs_var, kalman_type, params):
    """The joint filter + the solver's backward pass for `mode`, on a cached plan whose layout is the one rk_dalton_solve
    writes; the launch goes through the plan's own bookkeeping (generation, layout, last_mode)."""
    obs, D, Om, n_bobs, ind = _refusals(ode_weight, interrogate, kalman_type, obs_data, obs_weight, obs_var, t_min, t_max,
                                        n_steps, obs_times)
    plan = _plan((ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type), params, mode,
                 n_bobs)
    d_obs, d_w, d_v, d_ind = _obs_on_device(plan, obs, D, Om, ind)
    plan.generation += 1               # whatever is in the output buffers now belongs to an earlier call
    plan._prepare_out(mode)
    plan.last_mode = mode
    plan.cfg.seed = _seed(key)
    _lib.check(plan.dev.lib.rk_dalton_solve(plan.dev.h, C.byref(plan.cfg), C.byref(plan.inp), C.byref(plan._out), mode,
                                            d_obs.ptr, d_w.ptr, d_v.ptr, d_ind.ptr, int(ind.shape[0]), n_bobs))
    return plan


def solve_mv(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
             obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", **params):
    """Mean and variance of p(X_{0:N} | Y_{0:M}, Z_{1:N}) (dalton.py:374-460): ``(mean (N+1, d, p), var (N+1, d, p, p))``
    with a leading batch axis for batched inputs."""
    plan = _solve(_lib.MODE_MV, key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                  obs_data, obs_times, obs_weight, obs_var, kalman_type, params)
    return plan.state_host()


def solve_sim(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
              obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", **params):
    """One draw from p(X_{0:N} | Y_{0:M}, Z_{1:N}) (dalton.py:463-545): ``x (N+1, d, p)`` [+ a leading batch axis].  ``key``
    is an integer seed of the solver's Philox stream (the draws of ``rodeo_amd.solve_sim``)."""
    plan = _solve(_lib.MODE_SIM, key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                  obs_data, obs_times, obs_weight, obs_var, kalman_type, params)
    return plan.x_host()
