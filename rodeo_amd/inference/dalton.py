"""
``rodeo.inference.dalton`` for Gaussian observations (src/rodeo/inference/dalton.py:39-545):
  * ``dalton``: the DALTON approximate log-likelihood log p(Y_{0:M} | Z_{1:N}) = logdens_joint - logdens_marg, the log-density
    of a filter that conditions on the ODE residuals Z and the observations Y minus that of a filter on Z alone (:39-235);
  * ``solve_mv``: the data-adaptive solver, mean and variance of p(X_{0:N} | Z_{1:N}, Y_{0:M}) -- the joint filter followed by
    the solver's own smoothing pass (:374-460);
  * ``solve_sim``: the same filter followed by the solver's sampler (:463-545).
  * ``dalton_at``: ``dalton`` with the observations at their own times, between grid nodes where they fall there (an
    addition; imported from this module, not re-exported by ``rodeo_amd.inference``).
  * ``dalton_grid`` / ``solve_mv_grid`` / ``solve_sim_grid``: the three on a non-uniform grid shared by the batch, every observation
    on a node (an addition, imported from this module like ``dalton_at``; ``rk_dalton_grid_loglik`` / ``rk_dalton_grid_solve``).
  * ``dalton_grid_jvp`` / ``dalton_grid_grad`` / ``dalton_grad``: ``dalton_grid``'s value with its derivatives in the ODE parameters
    and the initial state, forward mode, on the device (an addition, imported from this module; ``rk_dalton_grid_jvp``), and in
    the two log-scales ``"log_sigma"`` / ``"log_obs_var"`` (``rk_dalton_grid_jvp_hyper``).
  * ``daltonng`` / ``solve_mv_nn`` for non-Gaussian observations (:547-1039) and ``daltonng_grid`` / ``solve_mv_nn_grid``, the two
    on that non-uniform grid (an addition; ``rk_daltonng_grid_loglik`` / ``rk_daltonng_grid_solve``); imported from this module.
All of it runs on the device (``rk_dalton_loglik`` / ``rk_dalton_loglik_at`` / ``rk_dalton_solve``): both filters of every parameter set in one
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
import collections
import ctypes as C
import hashlib
import os
import numpy as np
from .. import _lib
from ..solve import cached_plan, _shape_rule
from ._grad import (_GRAD_BSTATE, _GRAD_HYPER, _GRAD_NOT_WRT, _GRAD_STATE_MAX, _direction, _grad_config, _grad_of,  # noqa: F401
                    _grad_ode, _split_hyper, _stage_directions, _stage_hyper, _unit_directions, _wrt_directions)
from ._obs import (_at_inputs, _at_layout, _grid_plan, _obs_nodes, _refuse_config, _served, _stack_pairs,  # noqa: F401
                   _stage_at)                                       # (noqa: the names that were reached through this module still are)
from .logpost import obs_index

_BMEAS = " (the dense / indep_init form is not served)"             # what dalton / dalton_at add to "n_bmeas = 1 only"


def _refusals(ode_weight, interrogate, kalman_type, obs_data, obs_weight, obs_var, t_min, t_max, n_steps, obs_times):
    """Everything this build does not serve, raised before any device work; returns (obs, D, Omega, n_bobs, obs_ind)."""
    obs, D, Om, n_bobs = _served("dalton", ode_weight, kalman_type, obs_data, obs_weight, obs_var, interrogate=interrogate,
                                 bmeas=_BMEAS)
    ind = obs_index(t_min, t_max, n_steps, obs_times)
    on_grid = ind[ind <= int(n_steps)]                              # (later times never match, here or in the reference)
    if np.any(np.diff(ind) < 0) or np.any(np.diff(on_grid) == 0):
        raise ValueError("dalton: the observations' grid indices must be strictly increasing (one observation per grid "
                         "point, in time order)")
    return obs, D, Om, n_bobs, ind


def _plan(args, params, mode, n_bobs):
    """The cached plan whose output layout is the one rk_dalton_solve writes: without flags where the tile route may serve
    (n_bstate = 3, one observation per block), else with RK_FLAG_BATCH_MINOR; checked against rk_dalton_layout."""
    p, d = int(np.shape(args[1])[-1]), int(np.shape(args[1])[-3])
    tiles = p == 3 and n_bobs == 1 and d <= 4 and os.environ.get("RK_DALTON_LANES", "0") in ("", "0")
    plan = cached_plan(*args, batch_minor=not tiles, **params)
    want = C.c_int32(0)
    _lib.check(plan.dev.lib.rk_dalton_layout(C.byref(plan.cfg), mode, n_bobs, C.byref(want)))
    if plan.solve_layout(mode) != want.value:                                     # (e.g. a user right-hand side without a tile form)
        plan = cached_plan(*args, batch_minor=True, **params)
    return plan


def dalton(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
           obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", **params):
    """log p(Y_{0:M} | Z_{1:N}) (dalton.py:39-235): a float, or an array (B,) for batched inputs."""
    obs, D, Om, n_bobs, ind = _refusals(ode_weight, interrogate, kalman_type, obs_data, obs_weight, obs_var, t_min, t_max,
                                        n_steps, obs_times)
    plan = _plan((ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type), params,
                 _lib.MODE_FILTER, n_bobs)
    return _loglik_on_grid(plan, key, obs, D, Om, n_bobs, ind)


def _loglik_on_grid(plan, key, obs, D, Om, n_bobs, ind):
    """rk_dalton_loglik on `plan` with the observations at the grid indices `ind`."""
    d_obs, d_w, d_v, d_ind = plan.staged("dalton", obs, D, Om, ind)
    plan.set_seed(key)
    out = plan.dev.empty((plan.B,))
    _lib.check(plan.dev.lib.rk_dalton_loglik(plan.dev.h, C.byref(plan.cfg), C.byref(plan.inp), d_obs.ptr, d_w.ptr, d_v.ptr,
                                             d_ind.ptr, int(ind.shape[0]), n_bobs, out.ptr))
    return plan.per_traj(out)


def _solve(mode, key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
           obs_data, obs_times, obs_weight, obs_var, kalman_type, params):
    """The joint filter + the solver's backward pass for `mode`, on a cached plan whose layout is the one rk_dalton_solve
    writes; the launch goes through the plan's own bookkeeping (``SolvePlan.launch``)."""
    obs, D, Om, n_bobs, ind = _refusals(ode_weight, interrogate, kalman_type, obs_data, obs_weight, obs_var, t_min, t_max,
                                        n_steps, obs_times)
    plan = _plan((ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type), params, mode,
                 n_bobs)
    d_obs, d_w, d_v, d_ind = plan.staged("dalton", obs, D, Om, ind)
    plan.launch(plan.dev.lib.rk_dalton_solve, key, mode, mode, d_obs.ptr, d_w.ptr, d_v.ptr, d_ind.ptr, int(ind.shape[0]), n_bobs)
    return plan


def solve_mv(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
             obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", **params):
    """Mean and variance of p(X_{0:N} | Y_{0:M}, Z_{1:N}) (dalton.py:374-460): ``(mean (N+1, d, p), var (N+1, d, p, p))``
    with a leading batch axis for batched inputs."""
    plan = _solve(_lib.MODE_MV, key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                  obs_data, obs_times, obs_weight, obs_var, kalman_type, params)
    return plan.state_host()


# --- observations between grid nodes (an addition) -----------------------------------------------

def dalton_at(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
              obs_data, obs_times, obs_weight, obs_var, prior_at, kalman_type="standard", **params):
    """
    ``dalton`` with the observations at their own times (an addition: ``dalton`` snaps every time to the next grid node):
    log p(Y | Z) = joint - marginal, a float, or an array (B,) for batched inputs.  The first thirteen arguments and the
    batching rules are ``dalton``'s; ``prior_at(dt)`` is ``solve_mv_at``'s, the prior ``(wgt_state, var_state)`` over a step of
    length dt (``lambda h: ibm_init(h, n_deriv, sigma)``).

    ``obs_times`` must be strictly increasing, finite and in [t_min, t_max] (ValueError; a time past t_max is an error here).
    A time within ``EVAL_AT_NODE_TOL`` of a step from a node is that node and is handled as ``dalton`` handles it; when every
    time is a node, ``prior_at`` is never called and the value is ``dalton``'s bit for bit (the same kernels run).  An
    observation at t in (t_n, t_n+1) splits step n of both filters: predict over the gap since the previous event (node or
    observation) with ``prior_at(gap)``, condition the joint filter on y, and after the interval's last observation predict up
    to t_n+1; the interrogation and the z update at node n + 1 follow.  Nothing is interrogated between nodes.  The sub-step
    priors of every such interval must compose to ``prior_pars`` (``check_prior_at``'s 1e-10 bar).  Served and refused as
    ``dalton``; all refusals come before any device work.
    """
    obs, D, Om, n_bobs = _served("dalton_at", ode_weight, kalman_type, obs_data, obs_weight, obs_var, interrogate=interrogate,
                                 bmeas=_BMEAS)
    table, stacked, batched = _at_inputs("dalton_at", ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, prior_pars,
                                         obs.shape[0], obs_times, prior_at, params)
    plan = _plan((ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type), params,
                 _lib.MODE_FILTER, n_bobs)
    if stacked is None:                                             # every time is a node: dalton itself, on those nodes
        return _loglik_on_grid(plan, key, obs, D, Om, n_bobs, table[:, 0])
    d_obs, d_w, d_v, at = _stage_at(plan, "dalton_at", obs, D, Om, table, stacked, batched)
    plan.set_seed(key)
    out = plan.dev.empty((plan.B,))
    _lib.check(plan.dev.lib.rk_dalton_loglik_at(plan.dev.h, C.byref(plan.cfg), C.byref(plan.inp), d_obs.ptr, d_w.ptr, d_v.ptr,
                                                C.byref(at), int(table.shape[0]), n_bobs, out.ptr))
    return plan.per_traj(out)


# --- DALTON on a non-uniform grid (an addition) ---------------------------------------------------

def _on_grid(who, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_times, obs_weight, obs_var,
             kalman_type, params):
    """
    What the three grid calls do before their launch: ``dalton``'s refusals of the configuration and the observations
    (``_served``), the observation times against the nodes, ``rodeo_amd.solve_mv_grid``'s refusals of the grid and ``prior_at``
    (called once per slot) -- all before any device work -- then the cached batch-minor plan with the grid and the observations
    staged on it.  Returns ``(plan, g, observation pointers and counts)``; the pointers are None for an empty observation set.
    """
    from .. import grid
    obs, D, Om, n_bobs = _served(who, ode_weight, kalman_type, obs_data, obs_weight, obs_var, interrogate=interrogate, bmeas=_BMEAS)
    node = _obs_nodes(who, grid._grid(t_grid), obs_times, obs.shape[0])
    ode, t, slot, pairs = grid._refusals(who, ode_fun, ode_weight, ode_init, t_grid, prior_at, kalman_type, params)
    return _grid_plan("dalton_grid", ode, ode_weight, ode_init, t, slot, pairs, interrogate, kalman_type, params, obs, D, Om, node,
                      n_bobs)


def dalton_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", **params):
    """
    ``dalton`` on a non-uniform grid shared by the batch (an addition): log p(Y | Z) = joint - marginal, a float, or an array
    (B,) for batched inputs.  ``t_grid`` (N+1,), ``prior_at(dt)`` (called once per slot of ``grid_slots(t_grid)``) and the batching
    of what it returns are ``rodeo_amd.solve_mv_grid``'s; the observation arguments, n_bobs = 1 .. 3 and what is served
    (kalman_type "standard", n_bmeas = 1, n_bstate 2 .. 6, 2 .. 5 with three or more blocks, rodeo / schober / kramer) are
    ``dalton``'s.

    EVERY OBSERVATION TIME MUST BE A NODE: time tau belongs to node k when |tau - t[k]| <= ``EVAL_AT_NODE_TOL`` times the shorter
    adjacent step.  ``rodeo_amd.grid_with_times(t_grid, obs_times)`` returns the grid with the times put in.  Unlike
    ``dalton_at``, the solver then interrogates the ODE at the observation times as well.  ValueError before any device work: a
    time that is no node, times not strictly increasing, two times on one node, a non-finite time, a time outside
    [t[0], t[-1]], and what ``solve_mv_grid`` and ``dalton`` refuse.

    Step n -> n + 1 of the joint filter: the prediction with the step's own prior pair, the interrogation at t[n+1], the z
    forecast log-density and update, then the conditioning on y if node n + 1 is observed (z first, y second, like ``dalton``);
    the marginal filter is the same without y.  An observation on node 0 adds log p(y_0 | x_0) to the joint density and does not
    update x_0.  An empty observation set gives 0.0.

    THE 1e-8 RULE.  Like ``dalton`` (utils.py:60-78 of the reference), a forecast whose variance s has |s| <= 1e-8 adds nothing
    to the log-density.  On a non-uniform grid the forecast variances of one run can lie on both sides of it, and a step can be
    kept in one filter and dropped in the other: the value then jumps.  With short steps and a small prior scale (n_bstate >= 4
    in particular) look at the scale of sigma before trusting a value.
    """
    if (getattr(ode_fun, "rhs_id", None) == _lib.RHS_FITZHUGH_NAGUMO and np.shape(ode_weight)[-1:] == (4,)
            and np.shape(obs_weight)[2:3] == (3,)):                 # (dalton_grid.hip: dalton_grid_ships)
        raise NotImplementedError("dalton_grid on the device: fitzhugh_nagumo at n_bstate = 4 with n_bobs = 3 is left out (its "
                                  "kernel needs more scratch than dalton's and solve_mv_grid's); the two grid solvers serve it")
    plan, g, (p_obs, p_w, p_v, p_ind, n_obs, n_bobs) = _on_grid(
        "dalton_grid", ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_times, obs_weight, obs_var,
        kalman_type, params)
    plan.set_seed(key)
    out = plan.dev.empty((plan.B,))
    _lib.check(plan.dev.lib.rk_dalton_grid_loglik(plan.dev.h, C.byref(plan.cfg), C.byref(plan.inp), p_obs, p_w, p_v, p_ind, n_obs,
                                                  n_bobs, C.byref(g), out.ptr))
    return plan.per_traj(out)


# --- DALTON gradients on the device (an addition) --------------------------------------------------

DaltonGrad = collections.namedtuple("DaltonGrad", ["value", "grad"])


# (Here, not in _grad.py: tests/test_hyper_grad_host.py records what is staged by patching this module's _stage_directions, for
# Fenrir's calls as well; fenrir.py imports this function.)
def _stage_all(who, ode, tangents, params, B, batched, d, p):
    """``_stage_directions`` on the parameters' and ode_init's directions and ``_stage_hyper`` on the reserved names': ``(K, dtheta,
    dtheta_batched, dinit, dinit_batched, hyper)`` with hyper None without a reserved name, else ``_stage_hyper``'s four."""
    plain, hyper = _split_hyper(tangents, params)
    if not hyper:
        return _stage_directions(who, ode, plain, B, batched, d, p) + (None,)
    staged = _stage_directions(who, ode, plain, B, batched, d, p) if plain else (None, None, 0, None, 0)
    hy = _stage_hyper(who, hyper, B, batched, d, staged[0])
    return (hy[0],) + staged[1:] + (hy[1:],)


def _jvp(who, key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_times, obs_weight, obs_var, tangents,
         kalman_type, params):
    """``dalton_grid_jvp``'s body: every refusal, then -- unless the observation set is empty -- the cached plan with the grid,
    the observations and the directions staged on it and one rk_dalton_grid_jvp.  Returns (value (B,), dvalue (B, K), batched)."""
    from .. import grid
    if not isinstance(tangents, dict):
        raise ValueError(f"{who}: tangents must be a dict name -> directions")
    ode_fun = _grad_config(who, ode_fun, ode_weight, interrogate, kalman_type, obs_weight, list(tangents), params)
    obs, D, Om, n_bobs = _served(who, ode_weight, kalman_type, obs_data, obs_weight, obs_var, interrogate=interrogate, bmeas=_BMEAS)
    node = _obs_nodes(who, grid._grid(t_grid), obs_times, obs.shape[0])
    ode, t, slot, pairs = grid._refusals(who, ode_fun, ode_weight, ode_init, t_grid, prior_at, kalman_type, params)
    sizes = _shape_rule(ode, ode_weight, ode_init, pairs[0], params)[-1]
    B, batched = (sizes[0], True) if sizes else (1, False)
    d, p = int(np.shape(ode_weight)[-3]), int(np.shape(ode_weight)[-1])
    K, dtheta, dtheta_b, dinit, dinit_b, hyper = _stage_all(who, ode, tangents, params, B, batched, d, p)
    if len(node) == 0:                                              # joint = marginal: nothing to launch
        return np.zeros(B), np.zeros((B, K)), batched
    plan, g, (p_obs, p_w, p_v, p_ind, n_obs, n_bobs) = _grid_plan("dalton_grid", ode, ode_weight, ode_init, t, slot, pairs, interrogate,
                                                                  kalman_type, params, obs, D, Om, node, n_bobs)
    d_th, d_x0 = plan.staged("dalton_grad", np.zeros(1) if dtheta is None else dtheta, np.zeros(1) if dinit is None else dinit)
    plan.set_seed(key)
    value, dvalue = plan.dev.empty((plan.B,)), plan.dev.empty((plan.B, K))
    head = (plan.dev.h, C.byref(plan.cfg), C.byref(plan.inp), p_obs, p_w, p_v, p_ind, n_obs, n_bobs, C.byref(g), K,
            None if dtheta is None else d_th.ptr, dtheta_b, None if dinit is None else d_x0.ptr, dinit_b)
    if hyper is None:                                               # (the kernel of every call without a reserved name)
        _lib.check(plan.dev.lib.rk_dalton_grid_jvp(*head, value.ptr, dvalue.ptr))
    else:
        dls, dls_b, dlo, dlo_b = hyper
        d_ls, d_lo = plan.staged("dalton_grad_hyper", np.zeros(1) if dls is None else dls, np.zeros(1) if dlo is None else dlo)
        _lib.check(plan.dev.lib.rk_dalton_grid_jvp_hyper(*head, None if dls is None else d_ls.ptr, dls_b,
                                                         None if dlo is None else d_lo.ptr, dlo_b, value.ptr, dvalue.ptr))
    return value.to_host(), dvalue.to_host(), batched


def dalton_grid_jvp(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                    obs_data, obs_times, obs_weight, obs_var, tangents, kalman_type="standard", **params):
    """
    ``dalton_grid`` and its directional derivatives (an addition; forward mode, on the device): ``(value, dvalue)``.  The first
    eleven arguments, ``kalman_type`` and ``**params`` are ``dalton_grid``'s.  ``tangents`` is a dict that holds K directions: its
    keys are names of ``params`` and / or ``"ode_init"``; a parameter direction has shape (K, size), or (B, K, size) when it
    differs per trajectory, an ``"ode_init"`` direction (K, d, p) or (B, K, d, p); a missing key is a zero direction.  ``value`` is
    ``dalton_grid``'s result, a float or (B,); ``dvalue`` is (K,) or (B, K): entry k is the derivative of ``value`` along direction
    k of (params, ode_init).  One launch (``rk_dalton_grid_jvp``): a (trajectory, direction) pair per lane, no atomics -- two calls
    give the same bits.

    It is the exact derivative of the filters' formulas as the kernels compute them (``dalton_grid``: predict, interrogate, z
    first, y second; an observation on node 0 is differentiated in x_0 and updates nothing).

    THE 1e-8 RULE (see ``dalton_grid``'s warning).  A forecast term that ``dalton_grid`` drops (|s| <= 1e-8) contributes nothing
    to the derivative either: where the value jumps, the derivative is that of the side the parameters are on.

    THE TWO LOG-SCALES.  Two reserved names are directions too, unless ``params`` has a parameter of
    that name (which then wins).  ``"log_sigma"``, shape (K, d) or (B, K, d): entry b is the rate of log sigma_b, the prior scale
    of block b, under the scale law ``evidence_scale`` relies on -- every step's prior variance R_b is proportional to sigma_b^2
    and Q does not depend on it, which is what ``prior_at = lambda h: ibm_init(h, p, sigma)`` satisfies; the initial variance is
    not scaled.  A ``prior_at`` that is no such scale family gets the derivative of (Q, e^{2c} R) in c, and nothing else.
    ``"log_obs_var"``, shape (K, d) or (B, K, d): entry b is the rate of a common log-scale of block b's observation variances,
    at every observation, node 0 and node N included.  They mix with the other names in one call, with one K; a call that holds
    one of them runs kernels of its own (``rk_dalton_grid_jvp_hyper``), every other call the kernels it ran before.

    Served: kalman_type "standard", n_bmeas = 1, n_bobs = 1, rodeo / schober / kramer, n_bstate 2 and 3 with n_block n_bstate^2
    <= 27; ``rodeo_amd.ode.fitzhugh_nagumo``, ``lorenz63`` and plain Python right-hand sides (a function, or ``ode.from_python``'s
    result: traced once more with generic parameters, ``rodeo_amd.trace.grad_from_python``, and built with hiprtc).
    NotImplementedError ("not built") before any device work: interrogate_chkrebtii, the square-root form, n_bobs > 1,
    n_bmeas > 1, another size or right-hand side, and a direction in the prior ("sigma", "prior_pars": use "log_sigma"),
    ``ode_weight`` or the data ("obs_var": use "log_obs_var").  ValueError before any device work: an unknown name in ``tangents``, a direction of the wrong
    shape or non-finite, K = 0, and whatever ``dalton_grid`` refuses.  An empty observation set returns (0.0, zeros) without a
    launch.
    """
    value, dvalue, batched = _jvp("dalton_grid_jvp", key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data,
                                  obs_times, obs_weight, obs_var, tangents, kalman_type, params)
    return (value, dvalue) if batched else (float(value[0]), dvalue[0])


def dalton_grid_grad(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                     obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", wrt=("theta",), init_jac=None, **params):
    """
    ``dalton_grid`` and its gradient (an addition): ``DaltonGrad(value, grad)`` with ``grad`` a dict name -> (size,), or (B, size)
    for batched inputs, for every name in ``wrt`` -- names of ``params`` and / or ``"ode_init"``, whose gradient has shape (d, p) or
    (B, d, p).  This is ``dalton_grid_jvp`` with the unit directions, in ONE launch; the direction count is the sum of the sizes.
    ``init_jac`` (optional): a dict name -> d ode_init / d param, shape (d, p, size) or (B, d, p, size); it is added into that
    parameter's ``ode_init`` direction, and the returned gradient is then the total derivative for an initial state that depends
    on the parameters (the quick start's ``init(v0, t, theta)``).  ``wrt`` may hold ``"log_sigma"`` and ``"log_obs_var"``
    (``dalton_grid_jvp``'s two log-scales, d unit directions each): ``grad["log_sigma"]`` and ``grad["log_obs_var"]`` are (d,) or
    (B, d); ``init_jac`` for either is a ValueError.  Served, refused and the 1e-8 rule as ``dalton_grid_jvp``;
    ValueError as well for a name in ``init_jac`` that is no parameter in ``wrt`` and for a Jacobian of the wrong shape.
    """
    who = "dalton_grid_grad"
    tangents, layout = _wrt_directions(who, "dalton_grid", ode_fun, ode_weight, ode_init, interrogate, kalman_type, obs_weight, wrt,
                                       init_jac, params)
    value, dvalue, batched = _jvp(who, key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_times,
                                  obs_weight, obs_var, tangents, kalman_type, params)
    return DaltonGrad(value if batched else float(value[0]), _grad_of(dvalue, layout, batched))


def dalton_grad(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", wrt=("theta",), init_jac=None, **params):
    """
    ``dalton`` and its gradient on the uniform grid (an addition): ``dalton_grid_grad`` on ``np.linspace(t_min, t_max, n_steps + 1)``
    with ``prior_at = lambda dt: prior_pars``; the observation times are mapped to nodes by ``dalton``'s own rule (the next grid
    index; an observation past t_max never matches and is left out).  The first thirteen arguments are ``dalton``'s, ``wrt`` and
    ``init_jac`` ``dalton_grid_grad``'s; returns ``DaltonGrad(value, grad)``.

    The value agrees with ``dalton``'s to 1e-9 relative, NOT bit for bit: the time of node n is the table's ``linspace`` entry
    here and ``t_min + (t_max - t_min) (n + 1) / n_steps`` there, which may differ by an ulp (and ``dalton`` may run on the tiles).
    Served, refused and the 1e-8 rule as ``dalton_grid_jvp``; ``wrt`` may hold ``"log_sigma"`` (with ``prior_pars =
    ibm_init(dt, p, sigma)``: the derivative in log sigma) and ``"log_obs_var"`` as in ``dalton_grid_grad``.
    """
    _grad_config("dalton_grad", ode_fun, ode_weight, interrogate, kalman_type, obs_weight, (wrt,) if isinstance(wrt, str) else tuple(wrt),
                 params)
    obs, D, Om, n_bobs, ind = _refusals(ode_weight, interrogate, kalman_type, obs_data, obs_weight, obs_var, t_min, t_max, n_steps,
                                        obs_times)
    on = ind <= int(n_steps)
    t = np.linspace(float(t_min), float(t_max), int(n_steps) + 1)
    return dalton_grid_grad(key, ode_fun, ode_weight, ode_init, t, interrogate, lambda dt: prior_pars, obs[on], t[ind[on]], D[on],
                            Om[on], kalman_type=kalman_type, wrt=wrt, init_jac=init_jac, **params)


def _solve_grid(who, mode, key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_times, obs_weight,
                obs_var, kalman_type, params):
    """The joint filter on the grid + ``rk_solve_grid``'s backward pass for `mode`; with no observations the plain grid solver."""
    plan, g, (p_obs, p_w, p_v, p_ind, n_obs, n_bobs) = _on_grid(
        who, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_times, obs_weight, obs_var, kalman_type,
        params)
    if n_obs == 0:                                                  # p(X | Z): rodeo_amd.solve_mv_grid / solve_sim_grid itself
        plan.launch(plan.dev.lib.rk_solve_grid, key, mode, mode, C.byref(g))
    else:
        plan.launch(plan.dev.lib.rk_dalton_grid_solve, key, mode, mode, p_obs, p_w, p_v, p_ind, n_obs, n_bobs, C.byref(g))
    if plan.layout != _lib.LAYOUT_BATCH_MINOR:
        raise RuntimeError(f"{who}: the plan reports layout {plan.layout}, not the batch-minor records")
    return plan


def solve_mv_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                  obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", **params):
    """Mean and variance of p(X | Z, Y) on the nodes ``t_grid`` (an addition): ``(mean (N+1, d, p), var (N+1, d, p, p))`` with a
    leading batch axis for batched inputs -- ``dalton_grid``'s joint filter, then ``rodeo_amd.solve_mv_grid``'s smoothing pass
    with every step's own prior pair.  Arguments, the node rule and the refusals are ``dalton_grid``'s; with an empty
    observation set the result is ``rodeo_amd.solve_mv_grid``'s."""
    return _solve_grid("dalton.solve_mv_grid", _lib.MODE_MV, key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                       obs_data, obs_times, obs_weight, obs_var, kalman_type, params).state_host()


def solve_sim_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                   obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", **params):
    """One draw from p(X | Z, Y) on the nodes ``t_grid`` (an addition): ``x (N+1, d, p)`` [+ a leading batch axis];
    ``dalton_grid``'s joint filter, then ``rodeo_amd.solve_sim_grid``'s sampler (``key`` seeds ``solve_sim``'s Philox stream,
    keyed by trajectory, step and block; ``x[0]`` is ``ode_init``).  Arguments and refusals are ``dalton_grid``'s."""
    return _solve_grid("dalton.solve_sim_grid", _lib.MODE_SIM, key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                       obs_data, obs_times, obs_weight, obs_var, kalman_type, params).x_host()


def solve_sim_draws_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                         obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", n_draws=1, keep=None, **params):
    """``n_draws`` draws from p(X | Z, Y) on the nodes ``t_grid`` from one joint filter (an addition):
    ``x`` (n_draws, K, d, p), or (B, n_draws, K, d, p) for batched inputs -- ``dalton_grid``'s joint filter (its store form), then
    ``rodeo_amd.solve_sim_draws_grid``'s backward kernel.  Arguments, the node rule and the refusals are ``dalton_grid``'s;
    ``n_draws`` and ``keep`` (node indices of ``t_grid``, ``None`` for every node) and their refusals are
    ``rodeo_amd.solve_sim_draws``'s, raised before any device work.  The law: draw ``s`` is ``solve_sim_grid``'s path (this
    module's) for the integer seed ``rodeo_amd.draws.draw_seed(key, s)``, restricted to ``keep``; node 0 is ``ode_init``.  With an
    empty observation set the result is ``rodeo_amd.solve_sim_draws_grid``'s."""
    from .. import grid
    from ..draws import _draw_rules, _launch_draws
    who = "dalton.solve_sim_draws_grid"
    n_draws, keep = _draw_rules(who, interrogate, n_draws, keep, len(grid._grid(t_grid)) - 1)
    plan, g, (p_obs, p_w, p_v, p_ind, n_obs, n_bobs) = _on_grid(
        who, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_times, obs_weight, obs_var, kalman_type,
        params)
    if n_obs == 0:                                                  # p(X | Z): rodeo_amd.solve_sim_draws_grid itself
        return _launch_draws(who, plan, key, plan.dev.lib.rk_solve_sim_draws_grid, n_draws, keep, C.byref(g))
    return _launch_draws(who, plan, key, plan.dev.lib.rk_dalton_grid_sim_draws, n_draws, keep, p_obs, p_w, p_v, p_ind, n_obs, n_bobs,
                         C.byref(g))


# --- non-Gaussian observations (src/rodeo/inference/dalton.py:547-1039) -------------------------------------------------
#
# ``daltonng`` and ``solve_mv_nn`` take an ordinary Python ``obs_loglik_i(obs_data_i, ode_data_i, ind, **params)`` written with
# NumPy (``rodeo_amd.trace.gammaln`` for log-factorials); it is traced once into scalar-generic device code
# (``trace.trace_obs_source``), differentiated twice by forward-mode duals (csrc/dual2.hpp) inside the forward filter and
# evaluated on plain doubles for logy_x.  What is built where the reference's text cannot be taken literally, and the other
# divergences, are listed in DESIGN.md section 7 (the selector of a block's active components as the weight; the block index
# where the reference has the observation index; NaN at a non-concave point; strictly increasing grid indices; no observation
# beyond t_max).  Neither name is re-exported from ``rodeo_amd.inference``: import them from this module.
#
# The function is run once per call, on symbols (plain Python, no device work; a function with side effects shows them once
# a call), and the traced models are kept by the hash of the generated source: a lambda or closure built anew per call finds
# its compiled kernels again, and nothing is registered twice.  Python values the function closes over (or reads from globals) are constants of the generated code -- a changed value
# is a different source, hence another model and another hiprtc build; what should vary between calls without a rebuild goes
# through ``**params``.

_obs_models = {}
_NG_PLACEHOLDER = "TracedObs_0000000000"                            # the struct's name until the source's hash is known


def _ng_param_spec(ode_fun, params):
    """How **params are packed: the right-hand side's own rule (the log-likelihood reads the same vector)."""
    spec = getattr(ode_fun, "param_spec", None)
    if spec is None:                                                # a Python right-hand side: SolvePlan's rule
        spec = tuple((k, int(np.shape(v)[-1]) if np.ndim(v) >= 1 else 1) for k, v in params.items())
    return tuple(spec)


def _ng_config(who, ode_fun, ode_weight, interrogate, kalman_type, obs_data, obs_loglik_i):
    """The configurations ``who`` (daltonng, or daltonng_grid) does not serve and the shapes of its observation arguments, raised
    before any device work; returns obs (n_obs, d, n_ycols) as contiguous float64."""
    _refuse_config(who, ode_weight, kalman_type, interrogate=interrogate, bmeas="")
    d, p = int(np.shape(ode_weight)[-3]), int(np.shape(ode_weight)[-1])
    if d >= 3 and p > 5:                                            # (daltonng.hip ng_check: the lane kernel spills)
        raise NotImplementedError(f"{who} on the device: n_bstate up to 5 with three or more blocks")
    rid = getattr(ode_fun, "rhs_id", None)
    if rid is not None and rid < _lib.RHS_USER_BASE:                # a built-in right-hand side: the hiprtc unit has to name it
        if rid not in (_lib.RHS_FITZHUGH_NAGUMO, _lib.RHS_LORENZ63, _lib.RHS_HIGHER_ORDER):
            raise NotImplementedError(f"{who} on the device: the built-in right-hand side {getattr(ode_fun, 'name', rid)!r} "
                                      "has no lane-per-trajectory form (fitzhugh_nagumo, lorenz63, higher_order, or a "
                                      "Python / from_source right-hand side)")
        if getattr(ode_fun, "n_block", d) != d:
            raise NotImplementedError(f"{who} on the device: the right-hand side {ode_fun.name!r} has {ode_fun.n_block} "
                                      f"blocks, ode_weight has {d}")
    obs = np.ascontiguousarray(obs_data, dtype=np.float64)
    if obs.ndim != 3 or obs.shape[1] != d:
        raise ValueError(f"obs_data must have shape (n_obs, {d}, n_ycols), got {obs.shape}")
    if not callable(obs_loglik_i):
        raise TypeError("obs_loglik_i must be a Python function obs_loglik_i(obs_data_i, ode_data_i, ind, **params)")
    return obs


def _ng_model(ode_fun, ode_weight, obs, obs_loglik_i, params):
    """The traced model of ``obs_loglik_i`` (the one run on symbols), kept by the hash of its generated source."""
    from ..trace import trace_obs_source
    d, p = int(np.shape(ode_weight)[-3]), int(np.shape(ode_weight)[-1])
    spec = _ng_param_spec(ode_fun, params)
    probe, active = trace_obs_source(obs_loglik_i, d, p, obs.shape[2], spec, _NG_PLACEHOLDER)
    key = hashlib.sha1(repr((probe, d, p, obs.shape[2], spec)).encode()).hexdigest()
    if key not in _obs_models:
        struct = "TracedObs_" + key[:10]
        _obs_models[key] = dict(source=probe.replace(_NG_PLACEHOLDER, struct), struct=struct, active=active,
                                n_theta=sum(s for _, s in spec), obs_id=None)
    return _obs_models[key]


def _ng_refusals(ode_fun, ode_weight, interrogate, kalman_type, obs_data, obs_times, obs_loglik_i, t_min, t_max, n_steps,
                 params):
    """Everything this build does not serve, raised before any device work; returns (obs, obs_ind, traced model)."""
    obs = _ng_config("daltonng", ode_fun, ode_weight, interrogate, kalman_type, obs_data, obs_loglik_i)
    times = np.asarray(obs_times, dtype=np.float64)
    if times.shape != (obs.shape[0],):
        raise ValueError(f"obs_times must have shape ({obs.shape[0]},), got {times.shape}")
    if np.any(times > float(t_max)):
        raise ValueError("daltonng: an observation time lies beyond t_max")
    ind = obs_index(t_min, t_max, n_steps, times)
    if np.any(np.diff(ind) <= 0):
        raise ValueError("daltonng: the observations' grid indices must be strictly increasing (one observation per grid "
                         "point, in time order)")
    return obs, ind, _ng_model(ode_fun, ode_weight, obs, obs_loglik_i, params)


def _ng_obs_id(model, d, p, n_ycols):
    """The library's id of a traced observation model (registered once; no device is needed for that)."""
    if model["obs_id"] is None:
        oid = C.c_int32(0)
        _lib.check(_lib.load().rk_register_obs_source(model["struct"].encode(), model["source"].encode(), d, p, n_ycols,
                                                      model["n_theta"], max(len(a) for a in model["active"]), C.byref(oid)))
        model["obs_id"] = oid.value
    return model["obs_id"]


def daltonng(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
             obs_data, obs_times, obs_loglik_i, kalman_type="standard", **params):
    """logy_x + logx_z - logx_yhat, the DALTON log-likelihood for non-Gaussian observations (dalton.py:851-949): a float, or
    an array (B,) for batched inputs.  The workspace (rk_daltonng_workspace_bytes: about 3.8 MB per trajectory at 4000 steps,
    two blocks, n_bstate = 3) lives for the call only; the plan keeps the uploaded observations and nothing else."""
    obs, ind, model = _ng_refusals(ode_fun, ode_weight, interrogate, kalman_type, obs_data, obs_times, obs_loglik_i, t_min,
                                   t_max, n_steps, params)
    plan = cached_plan(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type,
                       batch_minor=True, **params)
    oid = _ng_obs_id(model, plan.d, plan.p, obs.shape[2])
    d_obs, d_ind = plan.staged("daltonng", obs, ind)
    need = C.c_size_t(0)
    _lib.check(plan.dev.lib.rk_daltonng_workspace_bytes(C.byref(plan.cfg), int(ind.shape[0]), C.byref(need)))
    ws = plan.dev.empty((need.value // 8,))                         # two stored filters + the gain records: released on return
    plan.set_seed(key)
    out = plan.dev.empty((plan.B,))
    _lib.check(plan.dev.lib.rk_daltonng_loglik(plan.dev.h, C.byref(plan.cfg), C.byref(plan.inp), oid, d_obs.ptr, d_ind.ptr,
                                               int(ind.shape[0]), ws.ptr, ws.nbytes, out.ptr))
    return plan.per_traj(out)


def solve_mv_nn(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                obs_data, obs_times, obs_loglik_i, kalman_type="standard", **params):
    """Mean and variance of p(X_{0:N} | Yhat_{0:M}, Z_{1:N}) for non-Gaussian observations (dalton.py:955-1039):
    ``(mean (N+1, d, p), var (N+1, d, p, p))`` with a leading batch axis for batched inputs."""
    obs, ind, model = _ng_refusals(ode_fun, ode_weight, interrogate, kalman_type, obs_data, obs_times, obs_loglik_i, t_min,
                                   t_max, n_steps, params)
    plan = cached_plan(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type,
                       batch_minor=True, **params)
    oid = _ng_obs_id(model, plan.d, plan.p, obs.shape[2])
    d_obs, d_ind = plan.staged("daltonng", obs, ind)
    plan.launch(plan.dev.lib.rk_daltonng_solve, key, _lib.MODE_MV, _lib.MODE_MV, oid, d_obs.ptr, d_ind.ptr, int(ind.shape[0]))
    return plan.state_host()


# --- non-Gaussian observations on a non-uniform grid (an addition) -------------------------------

def _ng_on_grid(who, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_times, obs_loglik_i, kalman_type,
                params):
    """
    What the two grid calls do before their launch: ``daltonng``'s refusals of the configuration (``_ng_config``), the observation
    times against the nodes (``_obs_nodes``, ``dalton_grid``'s rule), ``rodeo_amd.solve_mv_grid``'s refusals of the grid and
    ``prior_at`` (called once per slot) and the trace of ``obs_loglik_i`` -- all before any device work -- then the cached
    batch-minor plan with the grid and the observations staged on it.  Returns ``(plan, g, obs_id, p_obs, p_node, n_obs)``; the
    pointers are None for an empty observation set.
    """
    from .. import grid
    obs = _ng_config(who, ode_fun, ode_weight, interrogate, kalman_type, obs_data, obs_loglik_i)
    node = _obs_nodes(who, grid._grid(t_grid), obs_times, obs.shape[0])
    ode, t, slot, pairs = grid._refusals(who, ode_fun, ode_weight, ode_init, t_grid, prior_at, kalman_type, params)
    model = _ng_model(ode_fun, ode_weight, obs, obs_loglik_i, params)
    plan = cached_plan(ode, ode_weight, ode_init, t[0], t[-1], len(slot), interrogate, pairs[0], kalman_type, batch_minor=True,
                       **params)
    (q, r), batched = _stack_pairs(pairs, plan.B)
    d_t, d_slot, d_q, d_r = plan.staged("grid", t, slot, q, r)
    g = _lib.GridIn(t=d_t.ptr, slot=d_slot.ptr, q=d_q.ptr, r=d_r.ptr, q_batched=batched, r_batched=batched, n_slots=len(pairs))
    oid = _ng_obs_id(model, plan.d, plan.p, obs.shape[2])
    p_obs = p_node = None
    if len(node):
        p_obs, p_node = (a.ptr for a in plan.staged("daltonng_grid", obs, node))
    return plan, g, oid, p_obs, p_node, len(node)


def daltonng_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                  obs_data, obs_times, obs_loglik_i, kalman_type="standard", **params):
    """
    ``daltonng`` on a non-uniform grid shared by the batch (an addition): logy_x + logx_z - logx_yhat, a float, or an array (B,)
    for batched inputs.  ``t_grid`` (N+1,), ``prior_at(dt)`` (called once per slot of ``grid_slots(t_grid)``) and the batching of
    what it returns are ``rodeo_amd.solve_mv_grid``'s; ``obs_data`` (n_obs, d, n_ycols), ``obs_loglik_i(obs_data_i, ode_data_i, ind,
    **params)`` -- ``ind`` is the observation's index i --, its tracing, the model cache and what is served (kalman_type
    "standard", n_bmeas = 1, n_bstate 2 .. 6, 2 .. 5 with three or more blocks, rodeo / schober / kramer, 1 .. 3 active components
    per block) are ``daltonng``'s.

    EVERY OBSERVATION TIME MUST BE A NODE (``dalton_grid``'s rule): time tau belongs to node k when |tau - t[k]| <=
    ``EVAL_AT_NODE_TOL`` times the shorter adjacent step, and ``rodeo_amd.grid_with_times(t_grid, obs_times)`` returns the grid with
    the times put in.  ValueError before any device work: a time that is no node, times not strictly increasing, two times on one
    node, a non-finite time, a time outside [t[0], t[-1]], and what ``solve_mv_grid`` and ``daltonng`` refuse.

    Step n -> n + 1 of the joint filter predicts with the step's own prior pair, interrogates at t[n+1], updates on z and, if node
    n + 1 is observed, conditions on the pseudo-observation yhat = mu-[A_b] + V g_A, V = (-H_AA)^{-1}, expanded at the predicted
    mean (z first, yhat second, like ``daltonng``).  An observation on node 0 does not enter the filter; it enters logy_x at
    ``ode_init``.  The two backward conditionals at node n re-evaluate the prediction and the gain from the filtered moments of
    node n with the pair of step n.  A point where the log-likelihood is not concave gives NaN, never an error.  With NO
    OBSERVATIONS the call does what ``daltonng`` does with none: both filters run on the device and the value is
    logx_z - logx_yhat of two equal filters.  The workspace (``rk_daltonng_workspace_bytes``) lives for the call only.
    """
    plan, g, oid, p_obs, p_node, n_obs = _ng_on_grid("daltonng_grid", ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                                                     obs_data, obs_times, obs_loglik_i, kalman_type, params)
    need = C.c_size_t(0)
    _lib.check(plan.dev.lib.rk_daltonng_workspace_bytes(C.byref(plan.cfg), n_obs, C.byref(need)))
    ws = plan.dev.empty((need.value // 8,))                         # two stored filters + the gain records: released on return
    plan.set_seed(key)
    out = plan.dev.empty((plan.B,))
    _lib.check(plan.dev.lib.rk_daltonng_grid_loglik(plan.dev.h, C.byref(plan.cfg), C.byref(plan.inp), oid, p_obs, p_node, n_obs,
                                                    C.byref(g), ws.ptr, ws.nbytes, out.ptr))
    return plan.per_traj(out)


def solve_mv_nn_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                     obs_data, obs_times, obs_loglik_i, kalman_type="standard", **params):
    """Mean and variance of p(X | Z, Yhat) on the nodes ``t_grid`` for non-Gaussian observations (an addition): ``(mean (N+1, d,
    p), var (N+1, d, p, p))`` with a leading batch axis for batched inputs -- ``daltonng_grid``'s joint filter, then
    ``rodeo_amd.solve_mv_grid``'s smoothing pass with every step's own prior pair.  Arguments, the node rule and the refusals are
    ``daltonng_grid``'s; with an empty observation set the result is ``rodeo_amd.solve_mv_grid``'s (the rule of
    ``dalton.solve_mv_grid``)."""
    who = "daltonng_grid (solve_mv_nn_grid)"
    plan, g, oid, p_obs, p_node, n_obs = _ng_on_grid(who, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data,
                                                     obs_times, obs_loglik_i, kalman_type, params)
    if n_obs == 0:                                                  # p(X | Z): rodeo_amd.solve_mv_grid itself
        plan.launch(plan.dev.lib.rk_solve_grid, key, _lib.MODE_MV, _lib.MODE_MV, C.byref(g))
    else:
        plan.launch(plan.dev.lib.rk_daltonng_grid_solve, key, _lib.MODE_MV, _lib.MODE_MV, oid, p_obs, p_node, n_obs, C.byref(g))
    if plan.layout != _lib.LAYOUT_BATCH_MINOR:
        raise RuntimeError(f"{who}: the plan reports layout {plan.layout}, not the batch-minor records")
    return plan.state_host()


def solve_sim(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
              obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", **params):
    """One draw from p(X_{0:N} | Y_{0:M}, Z_{1:N}) (dalton.py:463-545): ``x (N+1, d, p)`` [+ a leading batch axis].  ``key``
    is an integer seed of the solver's Philox stream (the draws of ``rodeo_amd.solve_sim``)."""
    plan = _solve(_lib.MODE_SIM, key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                  obs_data, obs_times, obs_weight, obs_var, kalman_type, params)
    return plan.x_host()
