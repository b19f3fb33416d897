"""
``solve_evidence`` (an addition): the solver's own marginal likelihood log p(Z_{1:N} = 0), the
evidence of the interrogations under the prior, and from it the calibrated prior scale sigma in closed form.

    solve_evidence(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                   kalman_type="standard", **params) -> Evidence(logdens, quad, logdet, n_steps)
    evidence_scale(ev)  -> c = quad / n_steps                       the quasi-MLE is sigma_hat = sigma * sqrt(c)
    evidence_at(ev, c)  -> the log-evidence under prior_var_b -> c_b prior_var_b, without another solve

With z_{n,b} the innovation of block b at step n and s_{n,b} its forecast variance, quad_b = sum_n z^2 / s,
logdet_b = sum_n log s and logdens = -1/2 sum_b (quad_b + logdet_b) - d N log(2 pi) / 2.

THE SCALE LAW.  Under interrogate_rodeo / _schober / _kramer (an exact initial value, a block-diagonal Jacobian), replacing
block b's prior variance R_b by c_b R_b (its factor by sqrt(c_b) times the factor in the square-root form) leaves every
filtered and predicted mean and every innovation unchanged and multiplies every covariance of block b and every s_{n,b}
by c_b.  Hence quad_b -> quad_b / c_b and logdet_b -> logdet_b + N log c_b, the log-evidence under the rescaled prior is
-1/2 sum_b [quad_b / c_b + logdet_b + N log c_b + N log 2 pi] and its maximum is at c_b = quad_b / N.  One forward pass
calibrates sigma.  interrogate_chkrebtii draws its point from the predicted variance: no such law, refused.

All of it runs on the device (``rk_solve_evidence``): one kernel launch, nothing stored per step, 2 d + 1 doubles per
trajectory come back.  Routes: the p = 3 MFMA tiles (standard form, up to four blocks; ``evidence_tile3_kernels.hpp``),
else one lane per trajectory (standard, n_bstate 2 .. 6, 2 .. 5 with three or more blocks) or per (trajectory, block)
(square-root, n_bstate 2 .. 8) (``evidence_kernels.hpp``); ``RK_EVIDENCE_LANES=1`` forces the lanes at n_bstate = 3.
"""
import collections
import ctypes as C
import numpy as np
from . import _lib
from .solve import _KALMAN, _device_ode, _interrogate_id, _shape_rule, cached_plan

Evidence = collections.namedtuple("Evidence", ["logdens", "quad", "logdet", "n_steps"])

HALF_LOG_2PI = 0.5 * 1.83787706640934548356                        # (the device's constant, evidence_kernels.hpp)
BSTATE = {"standard": (2, 6), "square-root": (2, 8)}                # n_bstate served per Kalman form
BSTATE_THREE_BLOCKS = 5                                             # standard form, three or more blocks: the lane kernel spills at 6


def _refusals(ode_fun, ode_weight, ode_init, interrogate, prior_pars, kalman_type, params):
    """Everything this build does not serve, raised before any device work; returns the right-hand side as a DeviceODE."""
    if kalman_type not in _KALMAN:
        raise NotImplementedError(f"solve_evidence: unknown kalman_type {kalman_type!r}")
    if _interrogate_id(interrogate)[0] == _lib.INTERROGATE_CHKREBTII:
        raise NotImplementedError("solve_evidence: interrogate_chkrebtii is not served: it draws its interrogation point from "
                                  "the predicted variance, so the scale law behind the closed-form calibration does not hold "
                                  "(rodeo, schober, kramer)")
    W = np.shape(ode_weight)
    if len(W) not in (3, 4):
        raise ValueError("ode_weight must have shape (n_block, n_bmeas, n_bstate) [+ a leading batch axis]")
    d, m, p = W[-3:]
    if m != 1:
        raise NotImplementedError("solve_evidence on the device: n_bmeas = 1 only (the dense / indep_init form is not served)")
    lo, hi = BSTATE[kalman_type]
    if not lo <= p <= hi:
        raise NotImplementedError(f"solve_evidence on the device: n_bstate in {lo}..{hi} in the {kalman_type} form, got {p}")
    if kalman_type == "standard" and d >= 3 and p > BSTATE_THREE_BLOCKS:
        raise NotImplementedError(f"solve_evidence on the device: n_bstate up to {BSTATE_THREE_BLOCKS} with three or more blocks "
                                  f"in the standard form, got {p}")
    ode = _device_ode(ode_fun, ode_weight, params)
    if (ode.n_block, ode.n_bmeas) != (d, m):
        raise ValueError(f"ODE '{ode.name}' has (n_block, n_bmeas) = ({ode.n_block}, {ode.n_bmeas}) but ode_weight has ({d}, {m})")
    _shape_rule(ode, ode_weight, ode_init, prior_pars, params)      # ValueError: ranks, mismatched shapes, batch sizes
    return ode


def solve_evidence(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                   kalman_type="standard", **params):
    """
    log p(Z_{1:N} = 0) of the solver under ``prior_pars`` and its per-block parts: ``Evidence(logdens, quad, logdet, n_steps)``
    with ``logdens`` a float and ``quad`` / ``logdet`` of shape (d,), or (B,) and (B, d) for batched inputs.  The first nine
    arguments and the batching rules are ``solve_mv``'s (a leading batch axis on ``ode_init``, ``prior_pars``, ``**params``);
    ``key`` is accepted and unused: the three served interrogations draw nothing.

    The density is the plain Gaussian one, with no cut-off on the forecast variance s: a zero, negative or non-finite s gives
    inf or NaN as the arithmetic produces it.  It is therefore NOT ``dalton``'s marginal term wherever the rule of
    utils.py:60-78 (|s| <= 1e-8 dropped) drops a step -- an absolute threshold on s would break the scale law.

    Refused before any device work: NotImplementedError for an unknown ``kalman_type``, ``interrogate_chkrebtii`` (no scale
    law), n_bmeas > 1 (the dense / ``indep_init`` form) and n_bstate outside the served range (standard 2 .. 6, 2 .. 5 with
    three or more blocks; square-root 2 .. 8); ValueError for the shapes ``solve_mv`` refuses, a right-hand side with another
    block count than ``ode_weight`` among them.  In the square-root form
    ``prior_pars`` holds the factor of the prior variance, as for ``solve_mv``.
    """
    ode = _refusals(ode_fun, ode_weight, ode_init, interrogate, prior_pars, kalman_type, params)
    plan = cached_plan(ode, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type,
                       batch_minor=True, **params)
    plan.set_seed(key)
    dev = plan.dev
    logdens, quad, logdet = dev.empty((plan.B,)), dev.empty((plan.d, plan.B)), dev.empty((plan.d, plan.B))
    _lib.check(dev.lib.rk_solve_evidence(dev.h, C.byref(plan.cfg), C.byref(plan.inp), logdens.ptr, quad.ptr, logdet.ptr))
    ld, q, l = logdens.to_host(), quad.batch_first(), logdet.batch_first()
    if plan.batched:
        return Evidence(ld, np.ascontiguousarray(q), np.ascontiguousarray(l), plan.N)
    return Evidence(float(ld[0]), q[0].copy(), l[0].copy(), plan.N)


def evidence_scale(ev):
    """c = quad / n_steps, shape (..., d): the scale of each block's prior variance that maximises the evidence.  The
    quasi-MLE of the prior scale is ``sigma_hat = sigma * sqrt(c)``."""
    return np.asarray(ev.quad, dtype=np.float64) / float(ev.n_steps)


def evidence_at(ev, c):
    """The log-evidence under prior_var_b -> c_b prior_var_b for any c > 0 (shape (d,) or (..., d), broadcast against ``ev``),
    from the scale law: -1/2 sum_b [quad_b / c_b + logdet_b + N log c_b] - d N log(2 pi) / 2, the blocks summed in block
    order.  At c = 1 it returns ``ev.logdens``."""
    c = np.asarray(c, dtype=np.float64)
    if np.any(~(c > 0)):
        raise ValueError("evidence_at: c must be positive")
    quad, logdet = np.asarray(ev.quad, dtype=np.float64), np.asarray(ev.logdet, dtype=np.float64)
    N, d = float(ev.n_steps), quad.shape[-1]
    terms = quad / c + (logdet + N * np.log(c))
    tot = np.zeros(terms.shape[:-1])
    for b in range(d):                                              # (block order, like the device)
        tot = tot + terms[..., b]
    out = -0.5 * tot - float(d * int(ev.n_steps)) * HALF_LOG_2PI
    return float(out) if out.ndim == 0 else out
