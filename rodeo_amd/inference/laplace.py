"""
Laplace approximation of a parameter posterior: what ``fitz_laplace`` of docs/examples/parameter.md:239-275 does with
``jaxopt`` (mode), ``jax.jacfwd(jax.jacrev(.))`` (Hessian at the mode) and ``jax.random.multivariate_normal`` (draws), for
a log-posterior that is built around one BATCHED call of ``fenrir`` / ``dalton`` / ``basic`` / ``magi_logdens``.

There is no automatic differentiation here.  Gradient and Hessian are central differences: for k parameters one
evaluation of both needs S = 2 k^2 + 1 log-posterior values, and the solver evaluates that many trajectories in one
launch, so one Newton iteration costs one batched ``logpost`` call.  Results are therefore finite-difference values: with
the step h the truncation error is O(h^2) and the rounding error of a second difference is about eps |f| / h^2.
``step=None`` takes h_i = eps^(1/4) max(1, |u_i|) (about 1.2e-4) at the starting point, the usual balance of the two for
second differences; pass ``step`` (a scalar or (k,)) to override it.  The step is fixed for the whole run.

    laplace(logpost, upars_init, *, step=None, max_iter=50, gtol=1e-5, n_samples=0, key=None) -> LaplaceResult

``logpost(upars (B, k)) -> (B,)`` is the user's batched log-posterior on the unconstrained scale: their constraint
transform and log-prior in NumPy around one batched solver call.  ``upars_init`` is (k,) or (C, k): C independent starts
are solved in lock-step, every ``logpost`` call gets the (C S, k) points of all of them.

Each iteration: ``rk_fd_stencil`` (the points, csrc/laplace_kernels.hpp has their order) -> download -> ``logpost`` ->
upload -> ``rk_fd_grad_hess`` -> ``rk_newton_step``.  The optimiser is a damped Newton iteration (Levenberg-Marquardt
on ``damping``, per centre): the step solves (-H + damping I) delta = g; the next stencil is centred on the trial point
u + delta and its centre value is the trial value, so a trial is accepted when that value improved (or is equal within
eps^(5/8) max(1, |f|), the resolution of the comparison) and its stencil is finite (its gradient and Hessian are then
already there), and otherwise the kept point's step is retaken with ten times
the damping -- a rejected step costs one launch, not two.  A Hessian whose negative is not positive definite (``ok = 0``
from the device) raises the damping in the same way, without a new stencil.  A centre is converged when max |g_i| <
``gtol`` at a kept point; converged centres stay in the batch unchanged.  Two consequences of the resolution in the
acceptance rule: ``LaplaceResult.logpost`` is the value at the returned mode and may lie below the best value visited, by at
most eps^(5/8) max(1, |f|) per accepted step; and where max |g_i| stays above ``gtol`` at that resolution (a very sharp
posterior, or a ``gtol`` below the rounding of the differences) the iteration may go on accepting such steps until
``max_iter`` and return ``converged = False`` with a point that is a mode to the precision of the log-density.

Refused before any device work of this module (ValueError): k > 12 (the Newton step keeps its factor in registers), a
non-finite ``upars_init`` or ``step``, a ``logpost`` that does not return one finite value per row at the starting
points; ``n_samples > 0`` without an integer ``key``.  A later ``logpost`` result that is not of shape (C S,) is refused
too.  Non-finite values at later stencil points are not errors: they are counted in ``n_bad`` and the trial is rejected.

THE GRADIENT MODE, for a log-posterior that comes with its exact gradient -- ``fenrir_grad`` /
``dalton_grad`` / ``fenrir_grid_grad`` / ``dalton_grid_grad`` under the user's chain rule:

    laplace_grad(value_and_grad, upars_init, *, step=None, max_iter=50, gtol=1e-5, n_samples=0, key=None, check_grad=True)
        -> LaplaceResult

``value_and_grad(upars (B, k)) -> (value (B,), grad (B, k))``.  The gradient is the user's, the Hessian a central FIRST
difference of gradients on S = 2 k + 1 points per centre (u and u +- h_i e_i, the leading points of the stencil above):
H_ii = (g_i(u + h_i e_i) - g_i(u - h_i e_i)) / (2 h_i), and H_ij the mean of the two one-sided estimates (d g_j / d u_i and
d g_i / d u_j).  Its rounding error is eps |g| / h where the value mode has eps |f| / h^2, its truncation error O(h^2);
``step=None`` takes h_i = eps^(1/3) max(1, |u_i|) (about 6e-6), the balance of the two for first differences.  Each iteration:
``rk_fd_grad_stencil`` -> download -> ``value_and_grad`` -> upload -> ``rk_fd_hess_from_grad`` -> ``rk_newton_step``; the
optimiser, its acceptance rule, its constants and the meaning of every field of ``LaplaceResult`` are the ones above (both
entry points run ``_newton``), and ``max |g_i| < gtol`` is tested on the user's gradient, not on a difference quotient.
``n_bad`` counts non-finite values and non-finite gradient entries.

``check_grad``: on the first stencil, for every centre and coordinate, the user's g_i(u) is compared with the quotient
q_i = (f(u + h_i e_i) - f(u - h_i e_i)) / (2 h_i) of the values that stencil holds anyway, and a ValueError names centre,
coordinate, both numbers and the bar when

    |q_i - g_i| > 8 (t_i / 6 + 2 eps max(|f+|, |f-|, 1) / h_i) + 10 GRAD_PARITY max(1, max_j |g_j|)

with t_i = |g_i(u + h_i e_i) - 2 g_i(u) + g_i(u - h_i e_i)|: t_i / 6 is the quotient's truncation error h^2 |d^2 g_i / du_i^2| / 6
read off the gradient stencil, the second term its rounding, the third the bar the device gradients are held to (1e-7 of
max |g|) times ten; the factor 8 covers the variation of the third derivative over the stencil.  It catches a chain rule
written wrongly (d / d log theta without the factor theta; a forgotten ``init_jac``), which would otherwise converge to a wrong
point without a sign.  The rounding term assumes values good to eps |f|.  ``dalton``'s are not: it is the difference of two
log-densities and carries their rounding (measured: 1e-10 |f|), so at the default step its quotient can miss the bar with a
correct gradient; pass ``check_grad=False`` there, or test once with a larger ``step``.

``pull_back(grad, jac)`` is the chain rule the user's function needs: ``grad`` the dict a ``*_grad`` call returns, ``jac`` a dict
name -> d(that argument) / du of shape (B, ...argument shape..., k); the (B, k) sum of the contractions.

Refused before any device work of this module (ValueError, messages that name ``laplace_grad``): what ``laplace`` refuses, a
result at the start that is not a pair of shapes ((B,), (B, k)), a non-finite value or gradient at the start.  A later result of
the wrong shape is refused too.
"""
import ctypes as C
from typing import NamedTuple
import numpy as np
from .. import _lib
from ..device import default_device
from .pseudo_marginal import standard_normal

K_MAX = 12                                   # csrc/laplace_kernels.hpp LAPLACE_KMAX
_DAMP_UP, _DAMP_DOWN, _MAX_DAMP_RAISES = 10.0, 0.1, 40
# A trial counts as "not worse" down to this relative change of the log-posterior.  Close to the mode of a sharp posterior
# the gain a Newton step predicts, g^2 / (2 |H|), is far below the rounding of the log-density itself while the gradient is
# still above gtol, so a strict comparison there compares noise.  Measured on the FitzHugh-Nagumo fit at N = 800 (|H| up to
# 1.5e6, f = 87.7): the step that took max |g| from 3e-3 to 4e-8 lowered f by 7e-10 (8e-12 relative) and a strict rule
# threw it away, after which the run stalled at max |g| ~ 1e-3.  eps^(5/8) = 1.6e-10 is an order above that noise and two
# below eps^(1/2) |f|, the size of the second differences the stencil is built to resolve.
_F_RESOLUTION = np.finfo(np.float64).eps ** 0.625


class LaplaceResult(NamedTuple):
    """``mode`` (C, k), ``logpost`` (C,), ``hessian`` (C, k, k) of the log-posterior at the mode, ``cov`` (C, k, k) =
    (-hessian)^-1, ``log_evidence`` (C,) = logpost + k/2 log 2 pi - 1/2 log det(-hessian), ``converged`` (C,) bool,
    ``n_iter`` (stencils evaluated), ``n_bad`` (C,) non-finite stencil values met on the way, ``samples`` (C, n_samples, k)
    or None.  ``cov`` and ``log_evidence`` are NaN where -hessian is not positive definite.  For a (k,) start the leading
    axis is dropped."""
    mode: np.ndarray
    logpost: np.ndarray
    hessian: np.ndarray
    cov: np.ndarray
    log_evidence: np.ndarray
    converged: np.ndarray
    n_iter: int
    n_bad: np.ndarray
    samples: object = None


def n_stencil(k):
    """Number of stencil points per centre."""
    return 2 * k * k + 1


def default_step(upars):
    """h_i = eps^(1/4) max(1, |u_i|), the largest over the centres: (k,)."""
    u = np.atleast_2d(np.asarray(upars, dtype=np.float64))
    return np.finfo(np.float64).eps ** 0.25 * np.maximum(1.0, np.max(np.abs(u), axis=0))


def n_stencil_grad(k):
    """Number of stencil points per centre in the gradient mode."""
    return 2 * k + 1


def default_grad_step(upars):
    """h_i = eps^(1/3) max(1, |u_i|), the largest over the centres: (k,).  The balance of a central FIRST difference of
    gradients: truncation h^2 |g''| / 6 against rounding eps |g| / h."""
    u = np.atleast_2d(np.asarray(upars, dtype=np.float64))
    return np.finfo(np.float64).eps ** (1.0 / 3.0) * np.maximum(1.0, np.max(np.abs(u), axis=0))


def _check_args(who, upars_init, step, n_samples, key, default):
    """The refusals that need neither the device nor the user's function; returns (u (C, k), step (k,), single)."""
    u = np.array(upars_init, dtype=np.float64)
    single = u.ndim == 1
    if u.ndim not in (1, 2) or u.size == 0:
        raise ValueError(f"{who}: upars_init must have shape (k,) or (C, k), got {u.shape}")
    u = np.atleast_2d(u)
    n_c, k = u.shape
    if k > K_MAX:
        raise ValueError(f"{who}: k <= {K_MAX} parameters (the device Newton step keeps its factor in registers), got {k}")
    if not np.all(np.isfinite(u)):
        raise ValueError(f"{who}: upars_init is not finite")
    h = default(u) if step is None else np.broadcast_to(np.asarray(step, dtype=np.float64), (k,)).copy()
    if not (np.all(np.isfinite(h)) and np.all(h > 0)):
        raise ValueError(f"{who}: step must be positive and finite")
    if n_samples < 0 or (n_samples > 0 and not isinstance(key, (int, np.integer))):
        raise ValueError(f"{who}: n_samples > 0 needs an integer key (the seed of the Philox stream)")
    return u, h, single


def _check(logpost, upars_init, step, n_samples, key):
    """The refusals that need no device; returns (u (C, k), step (k,), single, f0 (C,))."""
    u, h, single = _check_args("laplace", upars_init, step, n_samples, key, default_step)
    n_c = len(u)
    f0 = np.asarray(logpost(u.copy()), dtype=np.float64)
    if f0.shape != (n_c,):
        raise ValueError(f"laplace: logpost must return one value per row, shape ({n_c},) for {n_c} rows, got {f0.shape}")
    if not np.all(np.isfinite(f0)):
        raise ValueError(f"laplace: logpost is not finite at upars_init: {f0}")
    return u, h, single, f0


class DeviceSteps:
    """The three device calls (``stencil``, ``grad_hess``, ``newton``) on buffers that live for one run, host arrays in and
    out.  ``laplace`` is built on it; it is public so that one iteration can be taken apart (scripts/laplace_times.py times
    its parts, tests/test_gpu_laplace.py checks each call against the NumPy restatement).  ``newton`` uploads gradient and
    Hessian again although ``grad_hess`` has just produced them on the device: the driver steps from the KEPT point of
    each centre, which after a rejected trial is not the one the last stencil was taken at."""

    def __init__(self, n_c, k, h):
        self.dev = dev = default_device()
        self.n_c, self.k, self.S = n_c, k, n_stencil(k)
        self.step = dev.to_device(h)
        self.u = dev.empty((n_c, k))
        self.pts = dev.empty((n_c, self.S, k))
        self.vals = dev.empty((n_c, self.S))
        self.grad, self.hess = dev.empty((n_c, k)), dev.empty((n_c, k, k))
        self.n_bad, self.ok = dev.empty((n_c,), np.int32), dev.empty((n_c,), np.int32)
        self.damping, self.delta, self.logdet = dev.empty((n_c,)), dev.empty((n_c, k)), dev.empty((n_c,))

    def stencil(self, u):
        """(C, k) -> the (C S, k) points on the host."""
        self.u.upload(u)
        _lib.check(self.dev.lib.rk_fd_stencil(self.dev.h, self.n_c, self.k, self.u.ptr, self.step.ptr, self.pts.ptr))
        return self.pts.to_host().reshape(self.n_c * self.S, self.k)

    def grad_hess(self, vals):
        """(C S,) -> grad (C, k), hess (C, k, k), n_bad (C,)."""
        self.vals.upload(vals.reshape(self.n_c, self.S))
        _lib.check(self.dev.lib.rk_fd_grad_hess(self.dev.h, self.n_c, self.k, self.vals.ptr, self.step.ptr, self.grad.ptr,
                                                self.hess.ptr, self.n_bad.ptr))
        return self.grad.to_host(), self.hess.to_host(), self.n_bad.to_host()

    def newton(self, grad, hess, damping):
        """delta (C, k), logdet (C,), ok (C,) of the kept gradient / Hessian at the given damping."""
        self.grad.upload(grad)
        self.hess.upload(hess)
        self.damping.upload(damping)
        _lib.check(self.dev.lib.rk_newton_step(self.dev.h, self.n_c, self.k, self.grad.ptr, self.hess.ptr, self.damping.ptr,
                                               self.delta.ptr, self.logdet.ptr, self.ok.ptr))
        return self.delta.to_host(), self.logdet.to_host(), self.ok.to_host().astype(bool)


class DeviceGradSteps(DeviceSteps):
    """``DeviceSteps`` for the gradient mode: ``grad_stencil`` and ``hess_from_grad`` on the S = 2 k + 1 points of
    ``laplace_grad``, and ``DeviceSteps.newton`` as it is.  Only the buffers of this mode are allocated, so ``stencil`` and
    ``grad_hess`` are not available here."""

    def __init__(self, n_c, k, h):
        self.dev = dev = default_device()
        self.n_c, self.k, self.S = n_c, k, n_stencil_grad(k)
        self.step = dev.to_device(h)
        self.u = dev.empty((n_c, k))
        self.pts = dev.empty((n_c, self.S, k))
        self.vals, self.grads = dev.empty((n_c, self.S)), dev.empty((n_c, self.S, k))
        self.grad, self.hess, self.grad_fd = dev.empty((n_c, k)), dev.empty((n_c, k, k)), dev.empty((n_c, k))
        self.n_bad, self.ok = dev.empty((n_c,), np.int32), dev.empty((n_c,), np.int32)
        self.damping, self.delta, self.logdet = dev.empty((n_c,)), dev.empty((n_c, k)), dev.empty((n_c,))

    def stencil(self, u):
        raise NotImplementedError("DeviceGradSteps holds the 2 k + 1 point stencil only: grad_stencil")

    def grad_hess(self, vals):
        raise NotImplementedError("DeviceGradSteps reduces values and gradients: hess_from_grad")

    def grad_stencil(self, u):
        """(C, k) -> the (C (2 k + 1), k) points on the host: the leading rows of ``DeviceSteps.stencil``."""
        self.u.upload(u)
        _lib.check(self.dev.lib.rk_fd_grad_stencil(self.dev.h, self.n_c, self.k, self.u.ptr, self.step.ptr, self.pts.ptr))
        return self.pts.to_host().reshape(self.n_c * self.S, self.k)

    def hess_from_grad(self, vals, grads):
        """vals (C S,), grads (C S, k) -> grad (C, k), hess (C, k, k), n_bad (C,), grad_fd (C, k)."""
        self.vals.upload(vals.reshape(self.n_c, self.S))
        self.grads.upload(grads.reshape(self.n_c, self.S, self.k))
        _lib.check(self.dev.lib.rk_fd_hess_from_grad(self.dev.h, self.n_c, self.k, self.vals.ptr, self.grads.ptr, self.step.ptr,
                                                     self.grad.ptr, self.hess.ptr, self.grad_fd.ptr, self.n_bad.ptr))
        return self.grad.to_host(), self.hess.to_host(), self.n_bad.to_host(), self.grad_fd.to_host()


def _first_damping(hess):
    """Where damping starts when it is first needed: 2^-9 of the Hessian's largest diagonal entry (of 1 at least)."""
    d = np.max(np.abs(np.diagonal(hess, axis1=-2, axis2=-1)), axis=-1)
    return 2.0 ** -9 * np.maximum(1.0, np.where(np.isfinite(d), d, 1.0))


def _raise_damping(damping, hess, which):
    first = _first_damping(hess)
    damping[which] = np.where(damping[which] > 0, damping[which] * _DAMP_UP, first[which])


def laplace(logpost, upars_init, *, step=None, max_iter=50, gtol=1e-5, n_samples=0, key=None):
    """Mode, Hessian and normal approximation of ``logpost`` from the start(s) ``upars_init`` (module docstring)."""
    u, h, single, f_keep = _check(logpost, upars_init, step, n_samples, key)
    n_c, k = u.shape
    S = n_stencil(k)
    dv = DeviceSteps(n_c, k, h)

    def evaluate(trial, first):
        pts = dv.stencil(trial)
        vals = np.asarray(logpost(pts), dtype=np.float64)
        if vals.shape != (n_c * S,):
            raise ValueError(f"laplace: logpost returned shape {vals.shape} for {n_c * S} points ({n_c} centres x {S})")
        g_t, h_t, bad_t = dv.grad_hess(vals)
        return vals.reshape(n_c, S)[:, 0], g_t, h_t, bad_t
    return _newton(dv, evaluate, u, f_keep, single, max_iter, gtol, n_samples, key)


def _newton(dv, evaluate, u, f_keep, single, max_iter, gtol, n_samples, key):
    """The damped Newton iteration of both entry points (module docstring) from the checked starts ``u`` (C, k) with values
    ``f_keep``.  ``evaluate(trial (C, k), first) -> (f (C,), grad (C, k), hess (C, k, k), n_bad (C,))`` is one stencil at the
    trial points; ``dv.newton`` is the step."""
    n_c, k = u.shape
    grad, hess = np.full((n_c, k), np.nan), np.full((n_c, k, k), np.nan)
    damping = np.zeros(n_c)
    converged, failed = np.zeros(n_c, bool), np.zeros(n_c, bool)
    n_bad = np.zeros(n_c, np.int64)
    trial = u.copy()
    n_iter = 0
    while n_iter < max_iter:
        f_t, g_t, h_t, bad_t = evaluate(trial, n_iter == 0)
        live = ~(converged | failed)
        n_bad += np.where(live, bad_t, 0)
        first = n_iter == 0
        n_iter += 1
        with np.errstate(invalid="ignore"):
            accept = live & (bad_t == 0) & (first | (f_t > f_keep - _F_RESOLUTION * np.maximum(1.0, np.abs(f_keep))))
        if first:
            failed |= live & ~accept                     # a start whose stencil is not finite has nothing to fall back on
        u[accept], f_keep[accept], grad[accept], hess[accept] = trial[accept], f_t[accept], g_t[accept], h_t[accept]
        damping[accept] *= _DAMP_DOWN
        damping[damping < 1e-12] = 0.0
        rejected = live & ~accept & ~failed
        _raise_damping(damping, hess, rejected)
        converged |= accept & (np.max(np.abs(grad), axis=1) < gtol)
        live = ~(converged | failed)
        if not live.any():
            break
        # the step of every kept point; an indefinite -H + damping I raises that centre's damping until the factor exists
        g_in, h_in = np.where(live[:, None], grad, 0.0), np.where(live[:, None, None], hess, -np.eye(k))
        for _ in range(_MAX_DAMP_RAISES):
            delta, _, ok = dv.newton(g_in, h_in, damping)
            if ok[live].all():
                break
            _raise_damping(damping, hess, live & ~ok)
        failed |= live & ~ok
        trial = np.where((live & ok)[:, None], u + np.nan_to_num(delta), u)
    # curvature at the kept points, without damping
    good = np.all(np.isfinite(hess), axis=(1, 2))
    _, logdet, ok = dv.newton(np.zeros((n_c, k)), np.where(good[:, None, None], hess, -np.eye(k)), np.zeros(n_c))
    ok &= good
    cov = np.full((n_c, k, k), np.nan)
    for c in np.flatnonzero(ok):
        cov[c] = np.linalg.inv(-hess[c])
        cov[c] = 0.5 * (cov[c] + cov[c].T)
    log_ev = np.where(ok, f_keep + 0.5 * k * np.log(2 * np.pi) - 0.5 * np.where(ok, logdet, 0.0), np.nan)
    samples = None
    if n_samples > 0:
        z = standard_normal(int(key), (n_c, n_samples, k))
        samples = np.full((n_c, n_samples, k), np.nan)
        for c in np.flatnonzero(ok):
            samples[c] = u[c] + z[c] @ np.linalg.cholesky(cov[c]).T
    res = (u, f_keep, hess, cov, log_ev, converged)
    if single:
        res = tuple(a[0] for a in res)
        n_bad, samples = n_bad[0], (samples[0] if samples is not None else None)
    return LaplaceResult(*res, n_iter, n_bad, samples)


# --- the gradient mode ------------------------------------------------------------------------------

GRAD_PARITY = 1e-7                           # the bar tests/test_gpu_fenrir_grad.py / test_gpu_dalton_grad.py hold the gradients to


def pull_back(grad, jac):
    """The chain rule from the arguments of a ``*_grad`` call back to u: ``grad`` is the dict such a call returns (name ->
    (B, ...argument shape...)), ``jac`` a dict name -> d(that argument) / du of shape (B, ...argument shape..., k).  Returns the
    (B, k) sum over the names of ``jac`` of the contraction over the argument's axes."""
    out = 0.0
    for name, J in jac.items():
        if name not in grad:
            raise ValueError(f"pull_back: jac has {name!r}, grad has {sorted(grad)}")
        g, J = np.asarray(grad[name], dtype=np.float64), np.asarray(J, dtype=np.float64)
        if J.ndim != g.ndim + 1 or J.shape[:-1] != g.shape:
            raise ValueError(f"pull_back: jac[{name!r}] must have shape {g.shape + ('k',)}, got {J.shape}")
        out = out + np.einsum("bi,bik->bk", g.reshape(len(g), -1), J.reshape(len(g), -1, J.shape[-1]))
    return out


def _value_and_grad(value_and_grad, pts, what):
    """One call of the user's function on the (B, k) points, refused unless it is a pair of shapes ((B,), (B, k))."""
    B, k = pts.shape
    res = value_and_grad(pts)
    if not (isinstance(res, (tuple, list)) and len(res) == 2):
        raise ValueError(f"laplace_grad: value_and_grad must return a pair (value, gradient) of shapes (({B},), ({B}, {k})){what}, "
                         f"got {type(res).__name__}")
    vals, grads = np.asarray(res[0], dtype=np.float64), np.asarray(res[1], dtype=np.float64)
    if vals.shape != (B,) or grads.shape != (B, k):
        raise ValueError(f"laplace_grad: value_and_grad must return a pair (value, gradient) of shapes (({B},), ({B}, {k})){what}, "
                         f"got ({vals.shape}, {grads.shape})")
    return vals, grads


def _check_grad(vals, grads, grad_fd, h):
    """The user's gradient at the centres against the difference quotient of their values (``laplace_grad``'s docstring):
    vals (C, S), grads (C, S, k), grad_fd (C, k) from the device."""
    eps = np.finfo(np.float64).eps
    k = len(h)
    i = np.arange(k)
    g0 = grads[:, 0]                                                                     # (C, k)
    gp, gm = grads[:, 1 + 2 * i, i], grads[:, 2 + 2 * i, i]                              # g_i(u +- h_i e_i): (C, k)
    fp, fm = np.abs(vals[:, 1 + 2 * i]), np.abs(vals[:, 2 + 2 * i])
    t = np.abs(gp - 2.0 * g0 + gm)
    floor = 10.0 * GRAD_PARITY * np.maximum(1.0, np.max(np.abs(g0), axis=1, keepdims=True))
    bar = 8.0 * (t / 6.0 + 2.0 * eps * np.maximum(np.maximum(fp, fm), 1.0) / h) + floor
    with np.errstate(invalid="ignore"):
        miss = np.abs(grad_fd - g0) > bar
    if miss.any():
        c, j = (int(a) for a in np.argwhere(miss)[0])
        raise ValueError(f"laplace_grad: the gradient of value_and_grad disagrees with the difference quotient of its values at "
                         f"centre {c}, coordinate {j}: gradient {g0[c, j]:.10e}, (f(u + h e) - f(u - h e)) / (2 h) = "
                         f"{grad_fd[c, j]:.10e} with h = {h[j]:.3e}, difference {abs(grad_fd[c, j] - g0[c, j]):.3e} above the "
                         f"bar {bar[c, j]:.3e} ({int(miss.sum())} of {miss.size} entries miss it; a chain rule written wrongly? "
                         f"check_grad=False skips this test)")


def laplace_grad(value_and_grad, upars_init, *, step=None, max_iter=50, gtol=1e-5, n_samples=0, key=None, check_grad=True):
    """``laplace`` for a log-posterior that comes with its exact gradient (module docstring): the mode by the same damped
    Newton iteration on the user's gradient, the Hessian a central first difference of gradients on the 2 k + 1 point
    stencil."""
    u, h, single = _check_args("laplace_grad", upars_init, step, n_samples, key, default_grad_step)
    n_c, k = u.shape
    S = n_stencil_grad(k)
    f_keep, g0 = _value_and_grad(value_and_grad, u.copy(), " at upars_init")
    f_keep = f_keep.copy()                                           # (the loop writes the kept values into it)
    if not (np.all(np.isfinite(f_keep)) and np.all(np.isfinite(g0))):
        raise ValueError(f"laplace_grad: value_and_grad is not finite at upars_init: value {f_keep}, gradient {g0}")
    dv = DeviceGradSteps(n_c, k, h)

    def evaluate(trial, first):
        pts = dv.grad_stencil(trial)
        vals, grads = _value_and_grad(value_and_grad, pts, f" for the {n_c} x {S} stencil points")
        g_t, h_t, bad_t, g_fd = dv.hess_from_grad(vals, grads)
        if first and check_grad:
            ok = bad_t == 0                                          # (a centre with a non-finite stencil fails in the loop)
            _check_grad(vals.reshape(n_c, S)[ok], grads.reshape(n_c, S, k)[ok], g_fd[ok], h)
        return vals.reshape(n_c, S)[:, 0], g_t, h_t, bad_t
    return _newton(dv, evaluate, u, f_keep, single, max_iter, gtol, n_samples, key)
