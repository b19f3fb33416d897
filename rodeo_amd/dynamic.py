"""
``solve_mv_dynamic`` / ``solve_sim_dynamic`` (an addition): the solver with a per-step calibrated
prior scale ("dynamic diffusion"), where ``solve_evidence`` / ``evidence_scale`` give one scale per block for the whole horizon.

    solve_mv_dynamic (key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                      kalman_type="standard", scale_min=0.0, **params)
        -> DynamicMV(mean (N+1, d, p), var (N+1, d, p, p), scale (N, d), logdens)
    solve_sim_dynamic(... same arguments ...)
        -> DynamicSim(x (N+1, d, p), scale (N, d), logdens)

THE RECURSION.  With the filtered moments (mu, Sigma) of block b at node n (Sigma_0 = 0), step n -> n + 1 predicts
mu- = Q mu and P = Q Sigma Q^T without the prior variance R, interrogates at mu- (W~ = ode_weight + wgt_meas, a = mean_meas),
forms the innovation z = 0 - (W~ mu- + a) and r = W~ R W~^T and takes

    c = max(z^2 / r, scale_min)                       ``scale[n, b]``

as the scale of R for this step: Sigma- = P + c R.  interrogate_rodeo's var_meas is W Sigma- W^T with this Sigma-, the others'
is 0; s = W~ Sigma- W~^T + var_meas and the usual update follow.  The backward passes are ``solve_mv``'s and ``solve_sim``'s
on these predictions.  ``logdens`` is the log-evidence of ``solve_evidence`` under the scaled prior,
-1/2 sum_b sum_n (z^2 / s + log s) - d N log(2 pi) / 2.

Two properties.  SCALE INVARIANCE: with ``scale_min = 0``, replacing R_b by k R_b leaves mean, var and logdens unchanged up to
rounding and divides ``scale`` by k -- the sigma handed to ``ibm_init`` stops being an input that matters.  FIRST STEP: Sigma_0 = 0
gives s = c r under schober and kramer, so the first step's z^2 / s is 1 (1/2 under rodeo, s = 2 c r).

All of it runs on the device (``rk_solve_dynamic``): ``dynamic_fwd_kernel``, one lane per trajectory, then
``dynamic_bwd_mv_kernel`` or ``dynamic_bwd_sim_kernel``, one lane per (trajectory, block), on batch-minor records.
"""
import collections
import math
import numpy as np
from . import _lib
from .solve import _KALMAN, _device_ode, _interrogate_id, _shape_rule, cached_plan

DynamicMV = collections.namedtuple("DynamicMV", ["mean", "var", "scale", "logdens"])
DynamicSim = collections.namedtuple("DynamicSim", ["x", "scale", "logdens"])

BSTATE = (2, 5)                                                     # n_bstate served (6 is left out on purpose: DESIGN.md)
BSTATE_THREE_BLOCKS = 4                                             # three or more blocks: at 5 the forward kernel out-spills solve_evidence's


def _refusals(name, ode_fun, ode_weight, ode_init, interrogate, prior_pars, kalman_type, scale_min, params):
    """Everything this build does not serve, raised before any device work; returns the right-hand side as a DeviceODE."""
    if kalman_type not in _KALMAN:
        raise NotImplementedError(f"{name}: unknown kalman_type {kalman_type!r}")
    if kalman_type != "standard":
        raise NotImplementedError(f"{name}: kalman_type='square-root' is not built")
    if _interrogate_id(interrogate)[0] == _lib.INTERROGATE_CHKREBTII:
        raise NotImplementedError(f"{name}: interrogate_chkrebtii is not served: it draws its interrogation point from the "
                                  "predicted variance, which here depends on the point through the scale (rodeo, schober, "
                                  "kramer)")
    try:
        floor = float(scale_min)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: scale_min must be a finite number >= 0, got {scale_min!r}") from None
    if not math.isfinite(floor) or floor < 0.0:
        raise ValueError(f"{name}: scale_min must be a finite number >= 0, got {scale_min!r}")
    W = np.shape(ode_weight)
    if len(W) not in (3, 4):
        raise ValueError("ode_weight must have shape (n_block, n_bmeas, n_bstate) [+ a leading batch axis]")
    d, m, p = W[-3:]
    if m != 1:
        raise NotImplementedError(f"{name} on the device: n_bmeas = 1 only (the dense / indep_init form is not served)")
    if not BSTATE[0] <= p <= BSTATE[1]:
        raise NotImplementedError(f"{name} on the device: n_bstate in {BSTATE[0]}..{BSTATE[1]}, got {p}")
    if d >= 3 and p > BSTATE_THREE_BLOCKS:
        raise NotImplementedError(f"{name} on the device: n_bstate up to {BSTATE_THREE_BLOCKS} with three or more blocks, got {p}")
    ode = _device_ode(ode_fun, ode_weight, params)
    if (ode.n_block, ode.n_bmeas) != (d, m):
        raise ValueError(f"ODE '{ode.name}' has (n_block, n_bmeas) = ({ode.n_block}, {ode.n_bmeas}) but ode_weight has ({d}, {m})")
    _shape_rule(ode, ode_weight, ode_init, prior_pars, params)      # ValueError: ranks, mismatched shapes, batch sizes
    return ode, floor


def _run(name, mode, key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type, scale_min,
         params):
    """The refusals, the cached batch-minor plan, one rk_solve_dynamic; returns the plan and (scale, logdens) on the host."""
    ode, floor = _refusals(name, ode_fun, ode_weight, ode_init, interrogate, prior_pars, kalman_type, scale_min, params)
    plan = cached_plan(ode, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type,
                       batch_minor=True, **params)
    dev = plan.dev
    scale, logdens = dev.empty((plan.N, plan.d, plan.B)), dev.empty((plan.B,))
    plan.launch(dev.lib.rk_solve_dynamic, key, mode, mode, floor, scale.ptr, logdens.ptr)
    if plan.layout != _lib.LAYOUT_BATCH_MINOR:                       # (batch_minor=True: the records rk_solve_dynamic writes)
        raise RuntimeError(f"{name}: the plan reports layout {plan.layout}, not the batch-minor records")
    s = scale.batch_first()                                          # (like state_host(): a view of the download, no transpose)
    return plan, (s if plan.batched else s[0]), plan.per_traj(logdens)


def solve_mv_dynamic(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                     kalman_type="standard", scale_min=0.0, **params):
    """
    Mean and variance of the solver with a per-step calibrated prior scale: ``DynamicMV(mean, var, scale, logdens)`` with
    ``mean`` (N+1, d, p), ``var`` (N+1, d, p, p), ``scale`` (N, d) -- ``scale[n, b]`` the factor on block b's prior variance for
    the step from node n to n + 1 -- and ``logdens`` a float; batched inputs add a leading B to every output (``logdens``
    (B,)).  The first nine arguments and the batching rules are ``solve_mv``'s (a leading batch axis on ``ode_init``,
    ``prior_pars``, ``**params``); ``key`` is accepted and unused: the three served interrogations draw nothing.

    ``scale_min`` (default 0.0, the pure formula) is a floor on every scale.  It is a keyword of this function, so an ODE
    parameter named ``scale_min`` is not possible.  At 0.0, a step whose innovation z is exactly 0 gives a scale of 0, hence a
    forecast variance s = 0 and inf / NaN as the arithmetic produces them -- as ``solve_evidence`` documents for its own s; a
    positive floor rules that out.  With a floor above every estimate the result is ``solve_mv``'s under (Q, scale_min R).

    The estimate presumes a consistent initial state: ``first_order_pad``'s zero-padded higher derivatives make the first
    scales large, which is the estimator inflating the uncertainty, not a defect.

    Refused before any device work: NotImplementedError for an unknown ``kalman_type``, for ``"square-root"`` (not built), for
    ``interrogate_chkrebtii`` (its point is drawn from the predicted variance, which here depends on the point), n_bmeas > 1
    and n_bstate outside 2 .. 5 (2 .. 4 with three or more blocks: the forward lane kernel would spill more than
    ``solve_evidence``'s); ValueError for the shapes ``solve_mv`` refuses and for a negative or non-finite ``scale_min``.
    """
    plan, scale, logdens = _run("solve_mv_dynamic", _lib.MODE_MV, key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps,
                                interrogate, prior_pars, kalman_type, scale_min, params)
    mean, var = plan.state_host()
    return DynamicMV(mean, var, scale, logdens)


def solve_sim_dynamic(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                      kalman_type="standard", scale_min=0.0, **params):
    """
    One sample solution per trajectory of the solver with a per-step calibrated prior scale: ``DynamicSim(x, scale, logdens)``
    with ``x`` (N+1, d, p) and ``scale`` / ``logdens`` as for ``solve_mv_dynamic`` (same arguments, batching rules, ``scale_min``
    and refusals).  ``key`` seeds the backward draws, keyed by trajectory, step and block like ``solve_sim``'s; ``x[0]`` is
    ``ode_init``.
    """
    plan, scale, logdens = _run("solve_sim_dynamic", _lib.MODE_SIM, key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps,
                                interrogate, prior_pars, kalman_type, scale_min, params)
    return DynamicSim(plan.x_host(), scale, logdens)
