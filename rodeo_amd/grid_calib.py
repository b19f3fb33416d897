"""
``solve_evidence_grid`` / ``solve_mv_dynamic_grid`` / ``solve_sim_dynamic_grid`` (an addition): the two
calibration tools -- ``solve_evidence`` and ``solve_mv_dynamic`` / ``solve_sim_dynamic`` -- on the grid that ``solve_mv_grid``
runs on, so that the prior scale sigma is calibrated on the discretisation the solver then uses.

    solve_evidence_grid   (key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, kalman_type="standard", **params)
        -> Evidence(logdens, quad, logdet, n_steps)                       n_steps = N = len(t_grid) - 1
    solve_mv_dynamic_grid (key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, kalman_type="standard",
                           scale_min=0.0, **params)
        -> DynamicMV(mean (N+1, d, p), var (N+1, d, p, p), scale (N, d), logdens)
    solve_sim_dynamic_grid(... same arguments ...)
        -> DynamicSim(x (N+1, d, p), scale (N, d), logdens)

THE GRID is ``solve_mv_grid``'s: ``t_grid`` (N+1,) finite, strictly increasing, shared by the batch; step n -> n + 1 takes the pair
(Q_n, R_n) = ``prior_at(h_rep[slot[n]])`` of ``grid_slots(t_grid)`` -- ``prior_at`` is called once per slot -- and interrogates at
``t_grid[n+1]``.

THE EVIDENCE is ``solve_evidence``'s with that pair at every step: quad_b = sum_n z^2 / s, logdet_b = sum_n log s, the plain
Gaussian density.  ``evidence_scale`` and ``evidence_at`` work on the result unchanged: the scale law holds when EVERY R_n of
block b becomes c_b R_n, which is ``prior_at`` with sigma sqrt(c_b).

THE DYNAMIC SOLVER is ``solve_mv_dynamic``'s step with the step's own pair: mu- = Q_n mu, P = Q_n Sigma Q_n^T,
c = max(z^2 / (W~ R_n W~^T), scale_min), Sigma- = P + c R_n, interrogate_rodeo's var_meas from this Sigma-, ``scale[n, b] = c``.  The
backward passes re-evaluate Sigma- as Q_n Sigma_f[n] Q_n^T + scale[n] R_n and form the gain with Q_n.  ``scale[n, b]`` multiplies
R_n, which already carries the step's length (h_n^(2q+1) for the IBM prior): it is an estimate of (sigma_hat / sigma)^2 and can
be compared across steps of different length.

All of it runs on the device (``rk_solve_evidence_grid``, ``rk_solve_dynamic_grid``): ``grid_evidence_kernel`` or
``grid_dynamic_fwd_kernel``, one lane per trajectory, then ``grid_dynamic_bwd_mv_kernel`` / ``grid_dynamic_bwd_sim_kernel``, one lane
per (trajectory, block), on batch-minor records.
"""
import ctypes as C
import math
import numpy as np
from . import _lib
from . import grid as _grid
from .dynamic import BSTATE as DYNAMIC_BSTATE, BSTATE_THREE_BLOCKS as DYNAMIC_BSTATE_THREE_BLOCKS, DynamicMV, DynamicSim
from .evidence import BSTATE as _EVIDENCE_BSTATE, BSTATE_THREE_BLOCKS as EVIDENCE_BSTATE_THREE_BLOCKS, Evidence
from .inference._obs import _stack_pairs
from .solve import _KALMAN, _interrogate_id, cached_plan

# n_bstate served: the ranges of solve_evidence's standard lanes and of solve_mv_dynamic (DYNAMIC_BSTATE), the uniform counterparts
EVIDENCE_BSTATE = _EVIDENCE_BSTATE["standard"]

_CHKREBTII_EVIDENCE = ("it draws its interrogation point from the predicted variance, so the scale law behind the closed-form "
                       "calibration does not hold (rodeo, schober, kramer)")
_CHKREBTII_DYNAMIC = ("it draws its interrogation point from the predicted variance, which here depends on the point through the "
                      "scale (rodeo, schober, kramer)")


def _refusals(name, bstate, bstate_three, why_not_chkrebtii, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, kalman_type,
              params):
    """What these entries refuse beyond ``grid._refusals`` -- interrogate_chkrebtii and an n_bstate outside their narrower range
    -- then ``grid._refusals`` itself, all before any device work; returns its (ode, t, slot, pairs)."""
    if kalman_type not in _KALMAN:
        raise NotImplementedError(f"{name}: unknown kalman_type {kalman_type!r}")
    if kalman_type != "standard":
        raise NotImplementedError(f"{name}: kalman_type='square-root' is not built")
    if _interrogate_id(interrogate)[0] == _lib.INTERROGATE_CHKREBTII:
        raise NotImplementedError(f"{name}: interrogate_chkrebtii is not served: {why_not_chkrebtii}")
    W = np.shape(ode_weight)
    if len(W) in (3, 4) and W[-2] == 1:                              # (anything else is grid._refusals' to name)
        d, p = W[-3], W[-1]
        if not bstate[0] <= p <= bstate[1]:
            raise NotImplementedError(f"{name} on the device: n_bstate in {bstate[0]}..{bstate[1]}, got {p}")
        if d >= 3 and p > bstate_three:
            raise NotImplementedError(f"{name} on the device: n_bstate up to {bstate_three} with three or more blocks, got {p}")
    return _grid._refusals(name, ode_fun, ode_weight, ode_init, t_grid, prior_at, kalman_type, params)


def _floor(name, scale_min):
    try:
        floor = float(scale_min)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: scale_min must be a finite number >= 0, got {scale_min!r}") from None
    if not math.isfinite(floor) or floor < 0.0:
        raise ValueError(f"{name}: scale_min must be a finite number >= 0, got {scale_min!r}")
    return floor


def _plan_and_grid(ode, t, slot, pairs, ode_weight, ode_init, interrogate, kalman_type, params):
    """The cached batch-minor plan (its own prior pair is slot 0's) and the staged grid, as ``grid._run`` has them."""
    plan = cached_plan(ode, ode_weight, ode_init, t[0], t[-1], len(slot), interrogate, pairs[0], kalman_type,
                       batch_minor=True, **params)
    (q, r), batched = _stack_pairs(pairs, plan.B)
    d_t, d_slot, d_q, d_r = plan.staged("grid", t, slot, q, r)
    g = _lib.GridIn(t=d_t.ptr, slot=d_slot.ptr, q=d_q.ptr, r=d_r.ptr, q_batched=batched, r_batched=batched, n_slots=len(pairs))
    return plan, g


def solve_evidence_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, kalman_type="standard", **params):
    """
    log p(Z_{1:N} = 0) of the solver on the nodes ``t_grid`` and its per-block parts: ``Evidence(logdens, quad, logdet, n_steps)``
    with ``n_steps`` = N = ``len(t_grid) - 1``, ``logdens`` a float and ``quad`` / ``logdet`` of shape (d,), or (B,) and (B, d) for
    batched inputs.  Arguments, batching rules, slots and the ``t_grid`` / ``prior_at`` refusals are ``solve_mv_grid``'s
    (``prior_at`` is called once per slot); ``key`` is accepted and unused: the three served interrogations draw nothing.

    ``evidence_scale(ev)`` and ``evidence_at(ev, c)`` work unchanged on the result.  The scale law behind them holds when every
    R_n of block b becomes c_b R_n -- ``prior_at`` with sigma sqrt(c_b) -- so ``sigma * sqrt(evidence_scale(ev))`` is the quasi-MLE
    of sigma on THIS grid.  The density is the plain Gaussian one, with no cut-off on the forecast variance s, as for
    ``solve_evidence``.

    Refused before any device work: everything ``solve_mv_grid`` refuses; NotImplementedError for an unknown ``kalman_type``, for
    ``"square-root"`` (not built), for ``interrogate_chkrebtii`` (no scale law) and for n_bstate outside 2 .. 6 (2 .. 5 with three
    or more blocks).
    """
    name = "solve_evidence_grid"
    ode, t, slot, pairs = _refusals(name, EVIDENCE_BSTATE, EVIDENCE_BSTATE_THREE_BLOCKS, _CHKREBTII_EVIDENCE, ode_fun, ode_weight,
                                    ode_init, t_grid, interrogate, prior_at, kalman_type, params)
    plan, g = _plan_and_grid(ode, t, slot, pairs, ode_weight, ode_init, interrogate, kalman_type, params)
    plan.set_seed(key)
    dev = plan.dev
    logdens, quad, logdet = dev.empty((plan.B,)), dev.empty((plan.d, plan.B)), dev.empty((plan.d, plan.B))
    _lib.check(dev.lib.rk_solve_evidence_grid(dev.h, C.byref(plan.cfg), C.byref(plan.inp), C.byref(g), logdens.ptr, quad.ptr,
                                              logdet.ptr))
    ld, q, l = logdens.to_host(), quad.batch_first(), logdet.batch_first()
    if plan.batched:
        return Evidence(ld, np.ascontiguousarray(q), np.ascontiguousarray(l), plan.N)
    return Evidence(float(ld[0]), q[0].copy(), l[0].copy(), plan.N)


def _run_dynamic(name, mode, key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, kalman_type, scale_min, params):
    """The refusals, the plan and the staged grid, one rk_solve_dynamic_grid; returns the plan and (scale, logdens) on the host."""
    floor = _floor(name, scale_min)
    ode, t, slot, pairs = _refusals(name, DYNAMIC_BSTATE, DYNAMIC_BSTATE_THREE_BLOCKS, _CHKREBTII_DYNAMIC, ode_fun, ode_weight,
                                    ode_init, t_grid, interrogate, prior_at, kalman_type, params)
    plan, g = _plan_and_grid(ode, t, slot, pairs, ode_weight, ode_init, interrogate, kalman_type, params)
    dev = plan.dev
    scale, logdens = dev.empty((plan.N, plan.d, plan.B)), dev.empty((plan.B,))
    plan.launch(dev.lib.rk_solve_dynamic_grid, key, mode, mode, C.byref(g), floor, scale.ptr, logdens.ptr)
    if plan.layout != _lib.LAYOUT_BATCH_MINOR:                       # (batch_minor=True: the records rk_solve_dynamic_grid writes)
        raise RuntimeError(f"{name}: the plan reports layout {plan.layout}, not the batch-minor records")
    s = scale.batch_first()
    return plan, (s if plan.batched else s[0]), plan.per_traj(logdens)


def solve_mv_dynamic_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, kalman_type="standard", scale_min=0.0,
                          **params):
    """
    Mean and variance of the solver on the nodes ``t_grid`` with a per-step calibrated prior scale:
    ``DynamicMV(mean, var, scale, logdens)`` with ``mean`` (N+1, d, p), ``var`` (N+1, d, p, p), ``scale`` (N, d) and ``logdens`` a
    float; batched inputs add a leading B to every output.  Arguments, batching rules, slots and the ``t_grid`` / ``prior_at``
    refusals are ``solve_mv_grid``'s; ``scale_min`` is ``solve_mv_dynamic``'s floor on every scale.

    ``scale[n, b]`` is the factor on R_n, block b's prior variance for the step from node n to n + 1.  R_n already carries that
    step's length (h_n^(2q+1) for the IBM prior), so ``scale[n, b]`` is an estimate of (sigma_hat / sigma)^2 that can be compared
    across steps of different length.  With ``scale_min = 0``, replacing every R_n by k R_n leaves mean, var and logdens unchanged
    up to rounding and divides ``scale`` by k; with a floor above every estimate the result is ``solve_mv_grid``'s under
    (Q_n, scale_min R_n) and ``logdens`` is ``solve_evidence_grid``'s under that prior.

    Refused before any device work: everything ``solve_mv_grid`` refuses; NotImplementedError for an unknown ``kalman_type``, for
    ``"square-root"`` (not built), for ``interrogate_chkrebtii`` (its point is drawn from the predicted variance, which here
    depends on the point) and for n_bstate outside 2 .. 5 (2 .. 4 with three or more blocks); ValueError for a negative or
    non-finite ``scale_min``.
    """
    plan, scale, logdens = _run_dynamic("solve_mv_dynamic_grid", _lib.MODE_MV, key, ode_fun, ode_weight, ode_init, t_grid,
                                        interrogate, prior_at, kalman_type, scale_min, params)
    mean, var = plan.state_host()
    return DynamicMV(mean, var, scale, logdens)


def solve_sim_dynamic_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, kalman_type="standard", scale_min=0.0,
                           **params):
    """
    One sample solution per trajectory on the nodes ``t_grid`` with a per-step calibrated prior scale:
    ``DynamicSim(x, scale, logdens)`` with ``x`` (N+1, d, p) and ``scale`` / ``logdens`` as for ``solve_mv_dynamic_grid`` (same
    arguments, batching rules, ``scale_min`` and refusals; ``scale[n, b]`` multiplies R_n, which already carries the step's
    length, so it can be compared across steps).  ``key`` seeds the backward draws, keyed by trajectory, step and block like
    ``solve_sim``'s; ``x[0]`` is ``ode_init``.
    """
    plan, scale, logdens = _run_dynamic("solve_sim_dynamic_grid", _lib.MODE_SIM, key, ode_fun, ode_weight, ode_init, t_grid,
                                        interrogate, prior_at, kalman_type, scale_min, params)
    return DynamicSim(plan.x_host(), scale, logdens)
