"""
``rodeo.inference.fenrir`` (src/rodeo/inference/fenrir.py:261-327): the Fenrir approximate log-likelihood
log p(Y_{0:M} | Z_{1:N}) -- forward filter (``_solve_filter``, storing the predicted moments), then the backward
Markov chain of ``smooth_cond`` run as a Kalman filter backwards in time that conditions on the observations
(``_backward``, fenrir.py:86-259).  Both passes run on the device (``rk_solve_filter`` + ``rk_fenrir_backward``: on
the MFMA-tile kernels at n_bstate = 3, else lane-per-trajectory with ``RK_FLAG_STORE_PRED | RK_FLAG_BATCH_MINOR``);
only B doubles come back.

Same signature as the reference.  Extension: a leading batch axis on ``ode_init`` / ``prior_pars`` / ``**params``
(observations are shared) returns an array (B,).  Observations per block: n_bobs = 1 .. 3 (``obs_data`` (n_obs, n_block,
n_bobs), ``obs_weight`` (n_obs, n_block, n_bobs, n_bstate), ``obs_var`` (n_obs, n_block, n_bobs, n_bobs), fenrir.py:106-122);
vector observations run on the lane-per-trajectory kernels (LU update, eigendecomposition log-density of utils.py:60-78).
``kalman_type="square-root"`` (fenrir.py:292-296, 421-426): ``prior_pars[1]`` and ``obs_var`` are lower factors, the forward
pass is the square-root filter and every backward step map comes from ``square_root.py``; its ``forecast`` squares the
factor before the log-density sees it (square_root.py:343-344), so the value is the same log-likelihood as in covariance
form for ``L L^T`` inputs (tests).  Lane-per-trajectory kernels (``fenrir_sqrt.hip``), n_bstate 2 .. 8.
``fenrir_at`` (an addition; imported from this module, not re-exported by ``rodeo_amd.inference``): ``fenrir`` with the
observations at their own times, between grid nodes where they fall there (``rk_fenrir_backward_at``).
``fenrir_grid`` / ``solve_mv_grid`` (an addition, imported from this module like ``fenrir_at``): the likelihood and the
data-adaptive solver on a non-uniform grid shared by the batch, every observation on a node (``rk_fenrir_grid_loglik`` /
``rk_fenrir_grid_solve_mv``).
``fenrir_grid_jvp`` / ``fenrir_grid_grad`` / ``fenrir_grad`` (an addition, imported from this module likewise): ``fenrir_grid``'s
value with its derivatives in the ODE parameters and the initial state, forward mode on the device (``rk_fenrir_grid_jvp``,
DESIGN.md section 7 (23)), and in the two log-scales ``"log_sigma"`` / ``"log_obs_var"`` (``rk_fenrir_grid_jvp_hyper``, section 7 (25)).
"""
import collections
import ctypes as C
import os
import numpy as np
from .. import _lib
from ..solve import SolvePlan, cached_plan, _shape_rule
from . import _obs
from ._grad import _grad_config, _grad_of, _wrt_directions
from .dalton import _stage_all                                      # (lives there: see its comment)
from ._obs import _at_inputs, _check_obs, _grid_plan, _served, _stage_at
from .logpost import obs_index


def fenrir(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
           obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", **params):
    if kalman_type not in ("standard", "square-root"):
        raise NotImplementedError                                   # fenrir.py:293-298
    obs, D, Om, n_bobs = _check_obs(obs_data, obs_weight, obs_var)
    ind = obs_index(t_min, t_max, n_steps, obs_times)             # fenrir.py:118-120
    if np.any(np.diff(ind) < 0):
        raise ValueError("obs_times must be ascending")
    if kalman_type == "square-root":
        plan = cached_plan(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type, **params)
    else:
        plan = _plan_for(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type, params,
                         tiles_ok=n_bobs == 1)
    return _backward_on_grid(plan, key, obs, D, Om, n_bobs, ind)


def _filter_and_stage(plan, key, obs, D, Om, n_bobs, ind):
    """The forward filter of `plan`, then the observations at the grid indices `ind` on the device: they live on the plan and
    are uploaded again only when they change (``SolvePlan.staged``; a sampler calls this once per step)."""
    if D.shape[1:] != (plan.d, n_bobs, plan.p):
        raise ValueError(f"obs_weight must have shape (n_obs, {plan.d}, n_bobs, {plan.p})")
    plan.filter(key)
    return plan.staged("fenrir", obs, D, Om, ind)


def _backward_on_grid(plan, key, obs, D, Om, n_bobs, ind):
    """The forward filter of `plan` and rk_fenrir_backward with the observations at the grid indices `ind`."""
    d_obs, d_w, d_v, d_ind = _filter_and_stage(plan, key, obs, D, Om, n_bobs, ind)
    dev = plan.dev
    out = dev.empty((plan.B,))
    _lib.check(dev.lib.rk_fenrir_backward(dev.h, C.byref(plan.cfg), C.byref(plan.inp), C.byref(plan._out), d_obs.ptr,
                                          d_w.ptr, d_v.ptr, d_ind.ptr, int(ind.shape[0]), n_bobs, out.ptr))
    return plan.per_traj(out)


def _plan_for(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type, params,
              tiles_ok=True, tiles_blocked_ok=True):
    """A (cached, solve.cached_plan) plan on the MFMA-tile forward kernels when the configuration has them (n_bstate = 3:
    the backward pass then re-evaluates the predicted moments from the filtered tiles), else on the lane-per-trajectory
    kernels with stored predictions."""
    args = (ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type)
    plan = cached_plan(*args, **params)
    lay = C.c_int32(0)
    _lib.check(plan.dev.lib.rk_solve_layout(C.byref(plan.cfg), _lib.MODE_FILTER, C.byref(lay)))
    # n_bstate = 3: the tile kernels (one observation per block); n_bstate = 4 .. 8: the blocked tile forward pass and a
    # lane-per-block backward filter on its records (any n_bobs); else the lane kernels with stored predictions
    on_tiles = (lay.value == _lib.LAYOUT_TILE3 and tiles_ok) or \
               (lay.value in (_lib.LAYOUT_TILE4, _lib.LAYOUT_TILEP) and kalman_type == "standard" and tiles_blocked_ok)
    if not on_tiles:
        plan = cached_plan(*args, store_pred=True, batch_minor=True, **params)
    return plan


# --- observations between grid nodes (an addition) -----------------------------------------------

def fenrir_at(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
              obs_data, obs_times, obs_weight, obs_var, prior_at, kalman_type="standard", **params):
    """
    ``fenrir`` with the observations at their own times (an addition: ``fenrir`` snaps every time to the next grid node):
    log p(Y | Z), a float, or an array (B,) for batched inputs.  The first thirteen arguments and the batching rules are
    ``fenrir``'s; ``prior_at(dt)`` is ``solve_mv_at``'s, the prior ``(wgt_state, var_state)`` over a step of length dt
    (``lambda h: ibm_init(h, n_deriv, sigma)``).  Imported from this module, not re-exported by ``rodeo_amd.inference``.

    ``obs_times`` must be strictly increasing, finite and in [t_min, t_max] (ValueError; a time past t_max is an error here).
    A time within ``EVAL_AT_NODE_TOL`` of a step from a node is that node; two times on one node are an error.  When every
    time is a node, ``prior_at`` is never called and the call is ``fenrir`` on those node indices, bit for bit (the same
    kernels run).  Fenrir's forward pass is free of data, so it is unchanged; an observation at t in (t_n, t_n+1) adds hops to
    the backward Markov chain between the nodes n + 1 and n: the forward moments at the observation times are predictions from
    the filtered moments at t_n with ``prior_at(gap)``, each hop is the ``smooth_cond`` map between two neighbouring events,
    and the chain is conditioned on y where it lands on an observation time.  Nothing is interrogated between nodes.  The
    sub-step priors of every such interval must compose to ``prior_pars`` (``check_prior_at``'s 1e-10 bar).

    Served: ``kalman_type="standard"``; n_bstate = 3 with one observation per block on the MFMA tiles, n_bstate 2 .. 6 with
    n_bobs 1 .. 3 on the lane-per-trajectory kernels with stored predictions (``RK_FENRIR_AT_LANES=1``, read per call, forces
    the lanes where the tiles serve).  The square-root form and n_bstate 7, 8 raise NotImplementedError.  All refusals come
    before any device work.
    """
    obs, D, Om, n_bobs = _served("fenrir_at", ode_weight, kalman_type, obs_data, obs_weight, obs_var, got=True)
    table, stacked, batched = _at_inputs("fenrir_at", ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, prior_pars,
                                         obs.shape[0], obs_times, prior_at, params)
    args = (ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type, params)
    if stacked is None:                                             # every time is a node: fenrir itself, on those nodes
        return _backward_on_grid(_plan_for(*args, tiles_ok=n_bobs == 1), key, obs, D, Om, n_bobs, table[:, 0])
    lanes = os.environ.get("RK_FENRIR_AT_LANES", "0") not in ("", "0")
    plan = _plan_for(*args, tiles_ok=n_bobs == 1 and not lanes, tiles_blocked_ok=False)
    plan.filter(key)
    dev = plan.dev
    d_obs, d_w, d_v, at = _stage_at(plan, "fenrir_at", obs, D, Om, table, stacked, batched)
    need = C.c_size_t(0)
    _lib.check(dev.lib.rk_fenrir_at_workspace_bytes(C.byref(plan.cfg), n_bobs, at.n_pre + at.n_post, C.byref(need)))
    ws = dev.empty((need.value // 8,))                              # the hop records: released on return
    out = dev.empty((plan.B,))
    _lib.check(dev.lib.rk_fenrir_backward_at(dev.h, C.byref(plan.cfg), C.byref(plan.inp), C.byref(plan._out), d_obs.ptr, d_w.ptr,
                                             d_v.ptr, C.byref(at), int(table.shape[0]), n_bobs, ws.ptr, out.ptr))
    return plan.per_traj(out)


# --- Fenrir on a non-uniform grid (an addition) ---------------------------------------------------

def _on_grid(who, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_times, obs_weight, obs_var,
             kalman_type, params):
    """
    What the two grid calls do before their launch: ``_check_obs``'s shape errors, the observation times against the nodes
    (``dalton_grid``'s rule), ``rodeo_amd.solve_mv_grid``'s refusals of the configuration, the grid and ``prior_at`` (called once
    per slot) -- all before any device work -- then the cached batch-minor plan with the grid staged in ``solve_mv_grid``'s slot
    and the observations in their own.  Returns ``(plan, g, observation pointers and counts)``; the pointers are None for an
    empty observation set.
    """
    from .. import grid
    obs, D, Om, n_bobs = _check_obs(obs_data, obs_weight, obs_var)
    node = _obs._obs_nodes(who, grid._grid(t_grid), obs_times, obs.shape[0])        # (by attribute: tests/test_fenrir_grid_host.py wants no _obs_nodes of this module's own)
    ode, t, slot, pairs = grid._refusals(who, ode_fun, ode_weight, ode_init, t_grid, prior_at, kalman_type, params)
    d, p = (int(n) for n in (np.shape(ode_weight)[-3], np.shape(ode_weight)[-1]))
    if D.shape[1:] != (d, n_bobs, p):
        raise ValueError(f"obs_weight must have shape (n_obs, {d}, n_bobs, {p})")
    return _grid_plan("fenrir_grid", ode, ode_weight, ode_init, t, slot, pairs, interrogate, kalman_type, params, obs, D, Om, node,
                      n_bobs)


def fenrir_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", **params):
    """
    ``fenrir`` on a non-uniform grid shared by the batch (an addition): log p(Y | Z), a float, or an array (B,) for batched
    inputs.  ``t_grid`` (N+1,), ``prior_at(dt)`` (called once per slot of ``grid_slots(t_grid)``) and the batching of what it
    returns are ``rodeo_amd.solve_mv_grid``'s; the observation arguments and n_bobs = 1 .. 3 are ``fenrir``'s.  Imported from
    this module, not re-exported by ``rodeo_amd.inference``.

    EVERY OBSERVATION TIME MUST BE A NODE, by ``dalton_grid``'s rule: time tau belongs to node k when |tau - t[k]| <=
    ``EVAL_AT_NODE_TOL`` times the shorter adjacent step.  ``rodeo_amd.grid_with_times(t_grid, obs_times)`` returns the grid with
    the times put in.  Unlike ``fenrir_at``, the solver then interrogates the ODE at the observation times as well, and every
    observation has a record: ``solve_mv_grid`` smooths through it.

    The forward pass is ``solve_mv_grid``'s (Fenrir's is free of data).  Backwards the carry starts at the filtered moments of
    node N; for n = N-1 .. 0 the prediction of node n + 1 is re-evaluated from the filtered moments of node n with the prior pair
    of step n, the Markov chain steps with that pair's transition matrix, and the step conditions on y where node n is
    observed -- node 0 like any other (``dalton_grid`` only adds a density there).  An empty observation set gives 0.0.

    Served: ``kalman_type="standard"``, n_bmeas = 1, n_bstate 2 .. 6 (2 .. 5 with three or more blocks), the four
    interrogations (``interrogate_chkrebtii`` with an integer ``key``), built-in and plain-Python right-hand sides.  Refused
    before any device work: what ``solve_mv_grid`` refuses (``"square-root"``: NotImplementedError, not built), the node errors
    (ValueError) and ``fenrir``'s shape errors.  The block sums of a trajectory are added in block order: two calls give the
    same bits.
    """
    plan, g, (p_obs, p_w, p_v, p_node, n_obs, n_bobs) = _on_grid(
        "fenrir_grid", ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_times, obs_weight, obs_var,
        kalman_type, params)
    out = plan.dev.empty((plan.B,))
    plan.launch(plan.dev.lib.rk_fenrir_grid_loglik, key, _lib.MODE_FILTER, p_obs, p_w, p_v, p_node, n_obs, n_bobs, C.byref(g),
                out.ptr)
    return plan.per_traj(out)


def solve_mv_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                  obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", **params):
    """
    Fenrir's data-adaptive solver on the nodes ``t_grid`` (an addition): mean and variance of p(X | Z, Y), ``(mean (N+1, d, p),
    var (N+1, d, p, p))`` with a leading batch axis for batched inputs -- ``fenrir_grid``'s backward filter with its moments
    kept, then ``solve_mv``'s smoothing sweep over them (nodes 0 and 1 keep the backward filter's own estimates).  Arguments, the
    node rule and the refusals are ``fenrir_grid``'s; with an empty observation set the backward filter never conditions and
    the result is the posterior of ``rodeo_amd.solve_mv_grid`` reached by another recursion.  The sweep inverts the backward
    filter's predicted variances: with ``interrogate_kramer`` / ``interrogate_schober`` (an exact measurement) these can be
    singular, as in ``solve_mv``.
    """
    return _solve_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_times, obs_weight, obs_var,
                       kalman_type, params).state_host()


def _solve_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_times, obs_weight, obs_var,
                kalman_type, params):
    """``solve_mv_grid`` up to the download: the plan whose batch-minor records hold the smoothed moments."""
    plan, g, (p_obs, p_w, p_v, p_node, n_obs, n_bobs) = _on_grid(
        "fenrir.solve_mv_grid", ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_times, obs_weight,
        obs_var, kalman_type, params)
    nbytes = C.c_size_t(0)
    _lib.check(plan.dev.lib.rk_fenrir_workspace_bytes(C.byref(plan.cfg), C.byref(nbytes)))
    ws = plan.dev.empty((nbytes.value // 8,))                       # the stored backward filter: released on return
    plan.launch(plan.dev.lib.rk_fenrir_grid_solve_mv, key, _lib.MODE_MV, p_obs, p_w, p_v, p_node, n_obs, n_bobs, C.byref(g), ws.ptr)
    if plan.layout != _lib.LAYOUT_BATCH_MINOR:
        raise RuntimeError(f"fenrir.solve_mv_grid: the plan reports layout {plan.layout}, not the batch-minor records")
    plan.sync()                                                     # (the sweep has read the workspace before it is released)
    return plan


# --- Fenrir gradients on the device (an addition) --------------------------------------------------

FenrirGrad = collections.namedtuple("FenrirGrad", ["value", "grad"])

# The tangent records of one call grow with the direction count K ((N + 1) d (p + p^2) B K doubles).  The directions are
# independent, so they run in chunks whose records fit this many bytes; a chunk is at least one direction.
_GRAD_WORKSPACE_BYTES = 2 ** 32


def _jvp(who, key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_times, obs_weight, obs_var, tangents,
         kalman_type, params):
    """``fenrir_grid_jvp``'s body: the gradient refusals (``_grad.py``'s helpers under this call's name), then ``fenrir_grid``'s in
    its order, the directions, and -- unless the observation set is empty -- the cached plan with the grid, the observations and
    the directions staged on it and one rk_fenrir_grid_jvp per chunk of directions.  Returns (value (B,), dvalue (B, K), batched)."""
    from .. import grid
    if not isinstance(tangents, dict):
        raise ValueError(f"{who}: tangents must be a dict name -> directions")
    ode_fun = _grad_config(who, ode_fun, ode_weight, interrogate, kalman_type, obs_weight, list(tangents), params, sibling="fenrir_grid")
    obs, D, Om, n_bobs = _check_obs(obs_data, obs_weight, obs_var)
    node = _obs._obs_nodes(who, grid._grid(t_grid), obs_times, obs.shape[0])
    ode, t, slot, pairs = grid._refusals(who, ode_fun, ode_weight, ode_init, t_grid, prior_at, kalman_type, params)
    d, p = int(np.shape(ode_weight)[-3]), int(np.shape(ode_weight)[-1])
    if D.shape[1:] != (d, n_bobs, p):
        raise ValueError(f"obs_weight must have shape (n_obs, {d}, n_bobs, {p})")
    sizes = _shape_rule(ode, ode_weight, ode_init, pairs[0], params)[-1]
    B, batched = (sizes[0], True) if sizes else (1, False)
    K, dtheta, dtheta_b, dinit, dinit_b, hyper = _stage_all(who, ode, tangents, params, B, batched, d, p)
    dls, dls_b, dlo, dlo_b = hyper if hyper is not None else (None, 0, None, 0)
    if len(node) == 0:                                              # nothing is conditioned on: no plan, no launch
        return np.zeros(B), np.zeros((B, K)), batched
    plan, g, (p_obs, p_w, p_v, p_node, n_obs, n_bobs) = _grid_plan("fenrir_grid", ode, ode_weight, ode_init, t, slot, pairs, interrogate,
                                                                   kalman_type, params, obs, D, Om, node, n_bobs)
    per_dir = C.c_size_t(0)
    _lib.check(plan.dev.lib.rk_fenrir_grid_jvp_workspace_bytes(C.byref(plan.cfg), 1, C.byref(per_dir)))
    K_c = min(K, max(1, _GRAD_WORKSPACE_BYTES // per_dir.value))
    ws = plan.dev.empty((K_c * per_dir.value // 8,))                # the tangent records of one chunk: released on return
    value, dvalue = None, np.zeros((plan.B, K))
    for ci, k0 in enumerate(range(0, K, K_c)):
        k1 = min(K, k0 + K_c)
        d_th, d_x0 = plan.staged(("fenrir_grad", ci), np.zeros(1) if dtheta is None else dtheta[k0:k1],
                                 np.zeros(1) if dinit is None else dinit[k0:k1])
        val, dval = plan.dev.empty((plan.B,)), plan.dev.empty((plan.B, k1 - k0))
        head = (key, _lib.MODE_FILTER, p_obs, p_w, p_v, p_node, n_obs, n_bobs, C.byref(g), k1 - k0,
                None if dtheta is None else d_th.ptr, dtheta_b, None if dinit is None else d_x0.ptr, dinit_b)
        if hyper is None:                                           # (the kernels of every call without a reserved name)
            plan.launch(plan.dev.lib.rk_fenrir_grid_jvp, *head, ws.ptr, val.ptr, dval.ptr)
        else:                                                       # (the hyper directions are sliced with the others)
            d_ls, d_lo = plan.staged(("fenrir_grad_hyper", ci), np.zeros(1) if dls is None else dls[k0:k1],
                                     np.zeros(1) if dlo is None else dlo[k0:k1])
            plan.launch(plan.dev.lib.rk_fenrir_grid_jvp_hyper, *head, None if dls is None else d_ls.ptr, dls_b,
                        None if dlo is None else d_lo.ptr, dlo_b, ws.ptr, val.ptr, dval.ptr)
        dvalue[:, k0:k1] = dval.to_host()
        if value is None:                                           # (every chunk recomputes the same primal filter)
            value = val.to_host()
    plan.sync()                                                     # (the backward kernel has read the workspace before it is released)
    return value, dvalue, batched


def fenrir_grid_jvp(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                    obs_data, obs_times, obs_weight, obs_var, tangents, kalman_type="standard", **params):
    """
    ``fenrir_grid`` and its directional derivatives (an addition; forward mode, on the device): ``(value, dvalue)``.  The first
    eleven arguments, ``kalman_type`` and ``**params`` are ``fenrir_grid``'s.  ``tangents`` is ``dalton_grid_jvp``'s: a dict that holds
    K directions, its keys names of ``params`` and / or ``"ode_init"``; a parameter direction has shape (K, size), or (B, K, size)
    when it differs per trajectory, an ``"ode_init"`` direction (K, d, p) or (B, K, d, p); a missing key is a zero direction.
    ``value`` is ``fenrir_grid``'s result, a float or (B,); ``dvalue`` is (K,) or (B, K): entry k is the derivative of ``value`` along
    direction k of (params, ode_init).  Imported from this module, not re-exported by ``rodeo_amd.inference``.

    It is the exact derivative of ``fenrir_grid``'s formulas as the kernels compute them.  Forward, a (trajectory, direction) pair
    per lane runs the data-free filter with its tangent and stores the tangent of every node's filtered moments; backward, a lane
    per (block, trajectory, direction) runs the derivative of the Markov chain -- of the smoothing gain, of the chain's offset and
    noise, of the conditioning on y -- next to the chain itself.  No atomics, and the block sums are added in block order: two
    calls give the same bits.  The tangent records take (N + 1) d (p + p^2) B K doubles; beyond ``_GRAD_WORKSPACE_BYTES`` (4 GiB)
    the directions run in chunks, which changes no bit of the result.

    THE 1e-8 RULE.  A y term that ``fenrir_grid`` drops (a forecast variance |w| <= 1e-8, utils.py:60-78) contributes nothing to
    the derivative either: where the value jumps, the derivative is that of the side the parameters are on.

    THE TWO LOG-SCALES.  Two reserved names are directions too, unless ``params`` has a parameter of
    that name (which then wins).  ``"log_sigma"``, shape (K, d) or (B, K, d): entry b is the rate of log sigma_b, the prior scale
    of block b, under the scale law ``evidence_scale`` relies on -- every step's prior variance R_b is proportional to sigma_b^2
    and Q does not depend on it, which is what ``prior_at = lambda h: ibm_init(h, p, sigma)`` satisfies; the initial variance is
    not scaled.  A ``prior_at`` that is no such scale family gets the derivative of (Q, e^{2c} R) in c, and nothing else.
    ``"log_obs_var"``, shape (K, d) or (B, K, d): entry b is the rate of a common log-scale of block b's observation variances,
    at every observation, node 0 and node N included.  They mix with the other names in one call, with one K; a call that holds
    one of them runs kernels of its own (``rk_fenrir_grid_jvp_hyper``), every other call the kernels it ran before.
    In chunked runs the two arrays are sliced with the others.

    Served: kalman_type "standard", n_bmeas = 1, n_bobs = 1, rodeo / schober / kramer, n_bstate 2 and 3 with n_block n_bstate^2
    <= 27; ``rodeo_amd.ode.fitzhugh_nagumo``, ``lorenz63`` and plain Python right-hand sides (a function, or ``ode.from_python``'s
    result: traced once more with generic parameters, ``rodeo_amd.trace.grad_from_python``, and built with hiprtc).
    NotImplementedError ("not built") before any device work: interrogate_chkrebtii, the square-root form, n_bobs > 1,
    n_bmeas > 1, another size or right-hand side, and a direction in the prior ("sigma"), ``ode_weight``, the data or the grid.
    ValueError before any device work: an unknown name in ``tangents``, a direction of the wrong shape or non-finite, K = 0, and
    whatever ``fenrir_grid`` refuses.  An empty observation set returns (0.0, zeros) without a launch.
    """
    value, dvalue, batched = _jvp("fenrir_grid_jvp", key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data,
                                  obs_times, obs_weight, obs_var, tangents, kalman_type, params)
    return (value, dvalue) if batched else (float(value[0]), dvalue[0])


def fenrir_grid_grad(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                     obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", wrt=("theta",), init_jac=None, **params):
    """
    ``fenrir_grid`` and its gradient (an addition): ``FenrirGrad(value, grad)`` with ``grad`` a dict name -> (size,), or (B, size)
    for batched inputs, for every name in ``wrt`` -- names of ``params`` and / or ``"ode_init"``, whose gradient has shape (d, p) or
    (B, d, p).  This is ``fenrir_grid_jvp`` with the unit directions; the direction count is the sum of the sizes.  ``wrt`` and
    ``init_jac`` are ``dalton_grid_grad``'s: ``init_jac`` is a dict name -> d ode_init / d param, shape (d, p, size) or (B, d, p, size),
    added into that parameter's ``ode_init`` direction, so that the returned gradient is the total derivative for an initial state
    built from the parameters (the quick start's ``init(v0, t, theta)``).  ``wrt`` may hold ``"log_sigma"`` and ``"log_obs_var"``
    (``fenrir_grid_jvp``'s two log-scales, d unit directions each): ``grad["log_sigma"]`` and ``grad["log_obs_var"]`` are (d,) or
    (B, d); ``init_jac`` for either is a ValueError.  Served, refused and the 1e-8 rule as ``fenrir_grid_jvp``;
    ValueError as well for a name in ``init_jac`` that is no parameter in ``wrt`` and for a Jacobian of the wrong shape.
    """
    who = "fenrir_grid_grad"
    tangents, layout = _wrt_directions(who, "fenrir_grid", ode_fun, ode_weight, ode_init, interrogate, kalman_type, obs_weight, wrt,
                                       init_jac, params)
    value, dvalue, batched = _jvp(who, key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_times,
                                  obs_weight, obs_var, tangents, kalman_type, params)
    return FenrirGrad(value if batched else float(value[0]), _grad_of(dvalue, layout, batched))


def fenrir_grad(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", wrt=("theta",), init_jac=None, **params):
    """
    ``fenrir`` and its gradient on the uniform grid (an addition): ``fenrir_grid_grad`` on ``np.linspace(t_min, t_max, n_steps + 1)``
    with ``prior_at = lambda dt: prior_pars``; the observation times are mapped to nodes by ``fenrir``'s own rule (``obs_index``: the
    next grid index, which must not decrease; a last time past t_max is conditioned on at node n_steps, as ``fenrir`` does).  Here
    the nodes must not repeat (ValueError): ``fenrir_grid`` has one observation per node.  The first thirteen arguments are
    ``fenrir``'s, ``wrt`` and ``init_jac`` ``fenrir_grid_grad``'s; returns ``FenrirGrad(value, grad)``.

    The value agrees with ``fenrir``'s to the cross-route bar (1e-7 of max(1, |value|)), NOT bit for bit: the time of node n is
    the table's ``linspace`` entry here and ``t_min + (t_max - t_min) (n + 1) / n_steps`` there, which may differ by an ulp, and
    ``fenrir`` may run on the tiles or on stored predictions where this call re-evaluates them.  Served, refused and the 1e-8 rule
    as ``fenrir_grid_jvp``; ``wrt`` may hold ``"log_sigma"`` (with ``prior_pars = ibm_init(dt, p, sigma)``: the derivative in
    log sigma) and ``"log_obs_var"`` as in ``fenrir_grid_grad``.
    """
    _grad_config("fenrir_grad", ode_fun, ode_weight, interrogate, kalman_type, obs_weight, (wrt,) if isinstance(wrt, str) else tuple(wrt),
                 params, sibling="fenrir_grid")
    obs, D, Om, _ = _check_obs(obs_data, obs_weight, obs_var)
    ind = obs_index(t_min, t_max, n_steps, obs_times)               # fenrir.py:118-120
    if np.any(np.diff(ind) < 0):
        raise ValueError("obs_times must be ascending")
    ind = np.minimum(ind, int(n_steps))                             # fenrir_bwd_kernel: an index past n_steps is node n_steps
    if np.any(np.diff(ind) == 0):
        raise ValueError("fenrir_grad: the observations' grid indices must be strictly increasing (one observation per grid "
                         "point)")
    t = np.linspace(float(t_min), float(t_max), int(n_steps) + 1)
    return fenrir_grid_grad(key, ode_fun, ode_weight, ode_init, t, interrogate, lambda dt: prior_pars, obs, t[ind], D, Om,
                            kalman_type=kalman_type, wrt=wrt, init_jac=init_jac, **params)


def solve_mv(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
             obs_data, obs_times, obs_weight, obs_var, kalman_type="standard", **params):
    """
    Fenrir's data-adaptive solver (src/rodeo/inference/fenrir.py:405-457): mean and variance of
    p(X_{0:N} | Z_{1:N}, Y_{0:M}) -- forward filter, backward filter through the observations, smoothing pass over the
    backward filter (``_smooth_mv``, fenrir.py:333-402).  Same arguments as ``fenrir``; returns ``(mean (N+1, d, p), var
    (N+1, d, p, p))`` with a leading batch axis for batched inputs.  Lane-per-trajectory kernels (``rk_fenrir_solve_mv``).
    On the blocked-tile route (a cached plan) the observations share ``fenrir``'s upload cache: uploaded when they change.
    """
    if kalman_type not in ("standard", "square-root"):
        raise NotImplementedError                                   # fenrir.py:421-426
    obs, D, Om, n_bobs = _check_obs(obs_data, obs_weight, obs_var)
    ind = obs_index(t_min, t_max, n_steps, obs_times)
    if np.any(np.diff(ind) < 0):
        raise ValueError("obs_times must be ascending")
    sq = kalman_type == "square-root"                               # (its forward pass is batch-minor and keeps no predictions)
    if not sq:
        # n_bstate = 4 .. 8: forward pass on the blocked MFMA tiles, backward filter and smoothing pass on its records
        # (rk_fenrir_solve_mv_tiles: no stored predictions, no batch-minor copy of the filter's output)
        tplan = cached_plan(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type, **params)
        lay = C.c_int32(0)
        _lib.check(tplan.dev.lib.rk_solve_layout(C.byref(tplan.cfg), _lib.MODE_FILTER, C.byref(lay)))
        if lay.value in (_lib.LAYOUT_TILE4, _lib.LAYOUT_TILEP) and 4 <= tplan.p <= 8:
            return _solve_mv_tiles(tplan, key, obs, D, Om, ind, n_bobs)
    plan = SolvePlan(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type,
                     store_pred=not sq, batch_minor=not sq, **params)
    (d_obs, d_w, d_v, d_ind), ws = _smoother_inputs(plan, key, obs, D, Om, n_bobs, ind)
    dev = plan.dev
    _lib.check(dev.lib.rk_fenrir_solve_mv(dev.h, C.byref(plan.cfg), C.byref(plan.inp), C.byref(plan._out), d_obs.ptr,
                                          d_w.ptr, d_v.ptr, d_ind.ptr, int(ind.shape[0]), n_bobs, ws.ptr))
    return plan.state_host()


def _smoother_inputs(plan, key, obs, D, Om, n_bobs, ind):
    """What both routes of ``solve_mv`` do first: ``_filter_and_stage`` (the observations share ``fenrir``'s cache on a cached
    plan, so a loop of calls uploads them once) and the workspace of rk_fenrir_workspace_bytes, released on return."""
    staged = _filter_and_stage(plan, key, obs, D, Om, n_bobs, ind)
    nbytes = C.c_size_t(0)
    _lib.check(plan.dev.lib.rk_fenrir_workspace_bytes(C.byref(plan.cfg), C.byref(nbytes)))
    return staged, plan.dev.empty((nbytes.value // 8,))


def _solve_mv_tiles(plan, key, obs, D, Om, ind, n_bobs):
    """``solve_mv`` on a plan whose forward pass runs on the blocked tiles (n_bstate 4 .. 8)."""
    (d_obs, d_w, d_v, d_ind), ws = _smoother_inputs(plan, key, obs, D, Om, n_bobs, ind)
    dev = plan.dev
    N, d, p, B = plan.cfg.n_steps, plan.d, plan.p, plan.cfg.n_traj
    mean, var = dev.empty((N + 1, d, p, B)), dev.empty((N + 1, d, p, p, B))
    _lib.check(dev.lib.rk_fenrir_solve_mv_tiles(dev.h, C.byref(plan.cfg), C.byref(plan.inp), C.byref(plan._out), d_obs.ptr,
                                                d_w.ptr, d_v.ptr, d_ind.ptr, int(ind.shape[0]), n_bobs, ws.ptr, mean.ptr, var.ptr))
    m, v = mean.batch_first(), var.batch_first()
    return (m, v) if plan.batched else (m[0], v[0])
