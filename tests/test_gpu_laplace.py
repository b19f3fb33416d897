"""
rodeo_amd.inference.laplace on the device: the three kernels (rk_fd_stencil, rk_fd_grad_hess, rk_newton_step) against the
NumPy restatement tests/laplace_oracle.py, and the driver on quadratics (exact answers), on a linear-Gaussian model whose
log-likelihood is exactly quadratic in the initial value (dense conditioning, tests/test_oracle_fenrir.py), and on the
FitzHugh-Nagumo parameters against the same driver around the CPU oracle's fenrir.

Tolerances come from the formulas, not from what the device gives.  With f the log-posterior, h the step and eps = 2^-52:
a second difference of values that carry a relative error r has an absolute error of at most 4 r max|f| / h^2, a first
difference r max|f| / h.  On a quadratic, central differences have no truncation error, so against the matrix A the
NumPy restatement is held to 16 eps max|f| / h^2 (r = 4 eps: the rounding of the four values and of the points), and the
device to the restatement within 4 eps max|f| / h^2 (same formula, same order of operations: a few ulps of the summed
terms).  Against an independent implementation of the log-density, r = 1e-7 is the parity tests/test_gpu_dalton.py and
tests/test_gpu_inference.py hold the device to.  Every figure is printed before it is asserted
(profiles/laplace_checks.txt keeps one run's output).
"""
import ctypes as C
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd import _lib
from rodeo_amd.inference import laplace as lap
from rodeo_amd.interrogate import interrogate_kramer
from oracle import fenrir as ofen, odes, priors, interrogations as oi
import laplace_oracle as lo
from test_oracle_fenrir import _exact_loglik

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
PARITY = 1e-7                        # device log-density against the oracles (tests/test_gpu_dalton.py _check_ll)


def _report(name, **figs):
    print("laplace_check " + name + "  " + "  ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}"
                                                    for k, v in figs.items()))


# ---- 1. exact curvature ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_c", [1, 7])
@pytest.mark.parametrize("k", [1, 2, 5, 12])
def test_grad_hess_is_exact_on_a_quadratic(k, n_c):
    A, m, c0, starts, logpost = lo.quadratic(k, n_c, seed=k)
    h = lap.default_step(starts)
    dv = lap.DeviceSteps(n_c, k, h)
    pts = dv.stencil(starts)
    np.testing.assert_array_equal(pts, lo.stencil(starts, h).reshape(-1, k))         # same points, same order, same bits
    vals = logpost(pts)
    g, H, bad = dv.grad_hess(vals)
    go, Ho, bado = lo.grad_hess(vals.reshape(n_c, -1), h)
    fmax, hmin = float(np.max(np.abs(vals))), float(np.min(h))
    dev_H, dev_g = float(np.max(np.abs(H - Ho))), float(np.max(np.abs(g - go)))
    ora_H = float(np.max(np.abs(Ho + A)))
    ora_g = float(np.max(np.abs(go - (A @ (m - starts).T).T)))
    _report("quadratic", k=k, C=n_c, dev_vs_numpy_H=dev_H, bound=4 * EPS * fmax / hmin ** 2, rel=dev_H / np.max(np.abs(Ho)),
            dev_vs_numpy_g=dev_g, numpy_vs_A=ora_H, bound_A=16 * EPS * fmax / hmin ** 2, numpy_vs_grad=ora_g)
    assert np.all(bad == 0) and np.all(bado == 0)
    assert dev_H <= 4 * EPS * fmax / hmin ** 2 and dev_g <= 4 * EPS * fmax / hmin
    np.testing.assert_array_equal(g, go)                # one expression per entry, IEEE operations, same order: the same
    np.testing.assert_array_equal(H, Ho)                # bits as the restatement, not only within the bound
    assert ora_H <= 16 * EPS * fmax / hmin ** 2 and ora_g <= 16 * EPS * fmax / hmin
    assert np.array_equal(H, np.swapaxes(H, 1, 2))                                   # symmetric by construction


# ---- 2. one Newton step lands on the mode ------------------------------------------------------------------------------
@pytest.mark.parametrize("n_c", [1, 7])
@pytest.mark.parametrize("k", [1, 2, 5, 12])
def test_newton_lands_on_the_mode_of_a_quadratic(k, n_c):
    A, m, c0, starts, logpost = lo.quadratic(k, n_c, seed=k)
    res = lap.laplace(logpost, starts, n_samples=4000, key=11)
    h = lap.default_step(starts)
    fmax = float(np.max(np.abs(logpost(lo.stencil(starts, h).reshape(-1, k)))))
    b_H, b_g = 16 * EPS * fmax / np.min(h) ** 2, 16 * EPS * fmax / np.min(h)
    lam_min = np.linalg.eigvalsh(A)[0]
    dist = float(np.max(np.linalg.norm(starts - m, axis=1)))
    tol_mode = (np.sqrt(k) * b_g + k * b_H * dist) / lam_min              # |A^-1| (gradient error + Hessian error x step)
    tol_cov = k * b_H / lam_min ** 2 * 2                                  # first-order perturbation of the inverse
    e_mode, e_cov = float(np.max(np.abs(res.mode - m))), float(np.max(np.abs(res.cov - np.linalg.inv(A))))
    ev = c0 + 0.5 * k * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(A)[1]
    e_ev = float(np.max(np.abs(res.log_evidence - ev)))
    tol_ev = 0.5 * k * b_H / lam_min * 2 + 4 * EPS * abs(ev) + 0.5 * np.max(np.linalg.eigvalsh(A)) * k * tol_mode ** 2
    _report("newton", k=k, C=n_c, n_iter=res.n_iter, mode_err=e_mode, tol_mode=float(tol_mode), cov_err=e_cov,
            tol_cov=float(tol_cov), evidence_err=e_ev, tol_evidence=float(tol_ev))
    assert res.mode.shape == (n_c, k) and res.samples.shape == (n_c, 4000, k)
    assert np.all(res.converged) and res.n_iter == 2 and np.all(res.n_bad == 0)
    assert e_mode <= tol_mode and e_cov <= tol_cov and e_ev <= tol_ev
    assert np.max(np.abs(res.hessian + A)) <= b_H
    # the draws have the approximation's moments (4000 draws: standard error of a mean sqrt(cov / 4000))
    sd = np.sqrt(np.diagonal(res.cov, axis1=1, axis2=2))
    assert np.max(np.abs(res.samples.mean(axis=1) - res.mode) / sd) < 5 / np.sqrt(4000)
    one = lap.laplace(logpost, starts[0], step=h)                         # a (k,) start drops the centre axis
    assert one.mode.shape == (k,) and one.hessian.shape == (k, k) and bool(one.converged) and one.samples is None
    np.testing.assert_array_equal(one.mode, res.mode[0])


# ---- 3. real log-density, exact answer ---------------------------------------------------------------------------------
N_LIN, P_LIN, OM = 10, 3, 0.05
W_LIN = np.array([[[0.0, 0.0, 1.0]]])
D_LIN = np.array([1.0, 0.0, 0.0])
FORCING = {"a": np.array([-1.0, 0.0, 0.0]), "f": lambda t: np.sin(2 * t)}


def _x0_lin(u):
    """x(0), x'(0) free; x''(0) = sin 0 - x(0)."""
    u = np.atleast_2d(u)
    return np.stack([u[:, 0], u[:, 1], -u[:, 0]], axis=1)[:, None, :]          # (B, 1, 3)


@pytest.mark.parametrize("method", ["dalton", "fenrir"])
def test_linear_gaussian_model_has_the_exact_mode_and_hessian(method):
    Q, R = priors.ibm_init(1.0 / N_LIN, P_LIN, np.array([0.5]))
    obs_times = np.array([0.2, 0.5, 1.0])
    ind = np.searchsorted(np.linspace(0.0, 1.0, N_LIN + 1), obs_times)
    y = np.random.default_rng(0).standard_normal((3, 1, 1)) * 0.3 - 0.5
    ow, ov = np.tile(D_LIN[None, None, None, :], (3, 1, 1, 1)), np.full((3, 1, 1, 1), OM)
    fn = {"dalton": ra.inference.dalton, "fenrir": ra.inference.fenrir}[method]

    def logpost(u):
        return fn(None, ra.ode.higher_order, W_LIN, _x0_lin(u), 0.0, 1.0, N_LIN, interrogate_kramer, (Q, R), y, obs_times, ow, ov)

    def exact(u):
        return _exact_loglik(W_LIN[0, 0], _x0_lin(u)[0, 0], Q[0], R[0], N_LIN, 0.0, 1.0, FORCING, ind, D_LIN, OM, y[:, 0, 0])

    # the exact log-likelihood is a quadratic in u: its gradient and Hessian at `start` from exact evaluations, unit steps
    start = np.array([-1.0, 0.0])
    e = np.eye(2)
    f0 = exact(start)
    g_ex = np.array([(exact(start + e[i]) - exact(start - e[i])) / 2 for i in range(2)])
    H_ex = np.empty((2, 2))
    for i in range(2):
        H_ex[i, i] = exact(start + e[i]) - 2 * f0 + exact(start - e[i])
    H_ex[0, 1] = H_ex[1, 0] = (exact(start + e[0] + e[1]) - exact(start + e[0] - e[1]) - exact(start - e[0] + e[1])
                               + exact(start - e[0] - e[1])) / 4
    mode_ex = start - np.linalg.solve(H_ex, g_ex)
    # exactly quadratic: no truncation error at any step, so a large step (0.1) keeps the 1 / h^2 amplification of the
    # log-density's parity small
    h = 0.1
    res = lap.laplace(logpost, start, step=h)
    fmax = max(1.0, max(abs(exact(start + s * h * (e[0] + e[1]))) for s in (-1, 0, 1)), abs(f0))
    tol_H, tol_g = 4 * PARITY * fmax / h ** 2, PARITY * fmax / h
    tol_mode = np.linalg.norm(np.linalg.inv(H_ex), 2) * (np.sqrt(2) * tol_g + 2 * tol_H * np.linalg.norm(mode_ex - start))
    e_H, e_mode = float(np.max(np.abs(res.hessian - H_ex))), float(np.max(np.abs(res.mode - mode_ex)))
    _report("linear_" + method, n_iter=res.n_iter, hess_err=e_H, tol_hess=tol_H, mode_err=e_mode, tol_mode=float(tol_mode),
            logpost_err=float(abs(res.logpost - exact(mode_ex))))
    assert bool(res.converged) and np.all(np.linalg.eigvalsh(H_ex) < 0)
    assert e_H <= tol_H and e_mode <= tol_mode
    assert abs(res.logpost - exact(mode_ex)) <= PARITY * fmax + 0.5 * np.linalg.norm(H_ex, 2) * 2 * tol_mode ** 2


# ---- 4. nonlinear parameters -------------------------------------------------------------------------------------------
def test_fitzhugh_nagumo_parameters_agree_with_the_driver_on_the_cpu_oracle():
    N, t_max, p, n_obs = 100, 5.0, 3, 6
    theta, x0 = np.array([0.2, 0.2, 3.0]), np.array([-1.0, 1.0])
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    prior = ra.ibm_init(t_max / N, p, np.array([0.1, 0.1]))
    obs_times = np.linspace(0.0, t_max, n_obs)
    X, _ = ra.solve_mv(None, ra.ode.fitzhugh_nagumo, W, init(x0, 0.0, theta=theta), 0.0, t_max, N, interrogate_kramer, prior,
                       theta=theta)
    idx = np.searchsorted(np.linspace(0.0, t_max, N + 1), obs_times)
    noise_sd = np.sqrt(0.005)
    y = (X[idx, :, 0] + noise_sd * np.random.default_rng(1).standard_normal((n_obs, 2)))[:, :, None]
    ow = np.zeros((n_obs, 2, 1, p)); ow[..., 0] = 1.0
    ov = np.full((n_obs, 2, 1, 1), noise_sd ** 2)

    def constrain(u):
        th = np.exp(u[:, :3])
        return th, np.stack([init(u[b, 3:5], 0.0, theta=th[b]) for b in range(len(u))])

    def logprior(u):
        return np.sum(-0.5 * (u / 10.0) ** 2 - np.log(10.0) - 0.5 * np.log(2 * np.pi), axis=1)

    def logpost_dev(u):
        th, X0 = constrain(u)
        return ra.inference.fenrir(None, ra.ode.fitzhugh_nagumo, W, X0, 0.0, t_max, N, interrogate_kramer, prior, y, obs_times,
                                   ow, ov, theta=th) + logprior(u)

    def logpost_cpu(u):
        th, X0 = constrain(u)
        return np.array([ofen.fenrir(None, odes.fitzhugh_nagumo, W, X0[b], 0.0, t_max, N, oi.interrogate_kramer, prior, y,
                                     obs_times, ow, ov, theta=th[b]) for b in range(len(u))]) + logprior(u)

    start = np.concatenate([np.log(theta), x0]) + 0.05
    gtol = 1e-5
    dev = lap.laplace(logpost_dev, start, gtol=gtol)
    cpu = lap.laplace(logpost_cpu, start, gtol=gtol)
    h = float(np.min(lap.default_step(start)))
    fmax = max(1.0, abs(cpu.logpost))
    tol_H, tol_g = 4 * PARITY * fmax / h ** 2, PARITY * fmax / h
    # both runs stop where their own gradient is below gtol: the modes differ by at most |H^-1| (2 gtol + gradient parity)
    tol_mode = np.linalg.norm(np.linalg.inv(cpu.hessian), 2) * np.sqrt(5) * (2 * gtol + tol_g)
    # gradient of the device log-posterior at the device's mode, from one more stencil
    dv = lap.DeviceSteps(1, 5, lap.default_step(start))
    g_mode, _, _ = dv.grad_hess(logpost_dev(dv.stencil(dev.mode[None])))
    e_H, e_mode = float(np.max(np.abs(dev.hessian - cpu.hessian))), float(np.max(np.abs(dev.mode - cpu.mode)))
    _report("fitzhugh_fenrir", n_iter_dev=dev.n_iter, n_iter_cpu=cpu.n_iter, grad_at_mode=float(np.max(np.abs(g_mode))),
            hess_diff=e_H, tol_hess=tol_H, hess_scale=float(np.max(np.abs(cpu.hessian))), mode_diff=e_mode,
            tol_mode=float(tol_mode), logpost_diff=float(abs(dev.logpost - cpu.logpost)))
    assert bool(dev.converged) and bool(cpu.converged)
    assert np.max(np.abs(g_mode)) < gtol
    assert np.all(np.linalg.eigvalsh(dev.hessian) < 0)
    assert e_H <= tol_H and e_mode <= tol_mode
    assert np.max(np.abs(np.exp(dev.mode[:3]) - theta)) < 0.5 and np.all(np.isfinite(dev.cov))     # a fit, not a stray point


# ---- 5. failure is visible ---------------------------------------------------------------------------------------------
def test_a_non_finite_stencil_value_is_counted_and_poisons_its_centre_only():
    k, n_c = 3, 3
    A, m, c0, starts, logpost = lo.quadratic(k, n_c, seed=5)
    h = lap.default_step(starts)
    dv = lap.DeviceSteps(n_c, k, h)
    vals = logpost(dv.stencil(starts)).reshape(n_c, -1)
    clean = dv.grad_hess(vals.reshape(-1))
    for bad_value in (np.nan, np.inf, -np.inf):
        v = vals.copy()
        v[1, 11] = bad_value
        g, H, bad = dv.grad_hess(v.reshape(-1))
        assert list(bad) == [0, 1, 0]
        assert np.all(np.isnan(g[1])) and np.all(np.isnan(H[1]))
        for c in (0, 2):
            np.testing.assert_array_equal(g[c], clean[0][c])
            np.testing.assert_array_equal(H[c], clean[1][c])
    v = vals.copy()
    v[2, :] = np.nan
    assert list(dv.grad_hess(v.reshape(-1))[2]) == [0, 0, 2 * k * k + 1]


def test_an_indefinite_hessian_gives_ok_zero_and_the_driver_raises_damping():
    dv = lap.DeviceSteps(3, 2, np.array([1e-4, 1e-4]))
    hess = np.stack([-np.eye(2), np.diag([-1.0, 1.0]), np.array([[-2.0, 0.5], [0.5, -1.0]])])
    grad = np.ones((3, 2))
    delta, logdet, ok = dv.newton(grad, hess, np.zeros(3))
    do, lo_, oko = lo.newton_step(grad, hess, np.zeros(3))
    assert list(ok) == [True, False, True] and list(oko) == [True, False, True]
    assert np.all(np.isnan(delta[1])) and np.isnan(logdet[1])
    np.testing.assert_allclose(delta[[0, 2]], do[[0, 2]], rtol=1e-14)
    np.testing.assert_allclose(logdet[[0, 2]], lo_[[0, 2]], rtol=1e-14, atol=1e-15)
    delta, logdet, ok = dv.newton(grad, hess, np.array([0.0, 3.0, 0.0]))              # damped: the factor exists
    assert ok.all() and np.all(np.isfinite(delta))
    np.testing.assert_allclose(delta[1], [0.25, 0.5], rtol=1e-14)
    # the driver: a start where the curvature in u_0 is positive (f = -(u0^2 - 1)^2 - u1^2 at u0 = 0.1) still reaches
    # the maximum at (1, 0), by damped steps
    calls = []

    def logpost(u):
        calls.append(len(u))
        return -(u[:, 0] ** 2 - 1.0) ** 2 - u[:, 1] ** 2
    res = lap.laplace(logpost, np.array([0.1, 0.5]))
    _report("saddle_start", n_iter=res.n_iter, mode0=float(res.mode[0]), mode1=float(res.mode[1]))
    assert bool(res.converged) and res.n_iter > 2
    np.testing.assert_allclose(res.mode, [1.0, 0.0], atol=1e-5)
    assert calls[0] == 1 and set(calls[1:]) == {9}                                    # one batched call per iteration


def test_a_step_into_a_non_finite_region_is_rejected_not_taken():
    # f = log u - u, start u = 3: the undamped step goes to u = -3 where f is NaN
    with np.errstate(invalid="ignore"):
        res = lap.laplace(lambda u: np.log(u[:, 0]) - u[:, 0], np.array([[3.0], [0.9]]))
    _report("nan_region", n_iter=res.n_iter, n_bad0=int(res.n_bad[0]), n_bad1=int(res.n_bad[1]))
    assert np.all(res.converged) and res.n_bad[0] > 0 and res.n_bad[1] == 0
    np.testing.assert_allclose(res.mode[:, 0], [1.0, 1.0], atol=1e-5)
    np.testing.assert_allclose(res.hessian[:, 0, 0], [-1.0, -1.0], atol=1e-5)


def test_more_than_twelve_parameters_are_unsupported_by_the_library():
    dev = ra.default_device()
    buf = dev.zeros((13 * 13 + 64,))
    ib = dev.zeros((4,), np.int32)
    rc = dev.lib.rk_newton_step(dev.h, 1, 13, buf.ptr, buf.ptr, buf.ptr, buf.ptr, buf.ptr, ib.ptr)
    assert rc == _lib.RK_ERR_UNSUPPORTED
    assert dev.lib.rk_fd_stencil(dev.h, 0, 2, buf.ptr, buf.ptr, buf.ptr) == _lib.RK_ERR_INVALID


def test_a_later_logpost_result_of_the_wrong_shape_is_refused():
    # one value per row at the start (C rows), one value too many for the C S stencil points afterwards
    n_c, k = 2, 3
    calls = []

    def logpost(u):
        calls.append(len(u))
        return -0.5 * np.sum(np.asarray(u) ** 2, axis=1) if len(calls) == 1 else np.zeros(len(u) + 1)
    with pytest.raises(ValueError, match=r"\(39,\) for 38 points"):
        lap.laplace(logpost, np.ones((n_c, k)))
    assert calls == [n_c, n_c * (2 * k * k + 1)]


@pytest.mark.parametrize("factor, accepted", [(0.5, True), (10.0, False)])
def test_a_trial_is_accepted_down_to_the_resolution_and_not_below(factor, accepted):
    """f = -u^2 / 2 from u = 1e-4 (max |g| = 1e-4 > gtol): the undamped step lands on 0.  The values of the SECOND stencil are
    shifted as a whole (gradient and Hessian unchanged) so that its centre value lies below the kept value by `factor` x the
    resolution eps^(5/8) max(1, |f|): half of it is accepted, and the result's logpost is then that lower value; ten times
    is rejected and the step retaken with damping."""
    u0, res = 1e-4, lap._F_RESOLUTION
    f_keep = -0.5 * u0 ** 2
    calls = []

    def logpost(u):
        calls.append(len(u))
        f = -0.5 * u[:, 0] ** 2
        if calls.count(3) == 2 and len(u) == 3:
            f = f - f[0] + (f_keep - factor * res)
        return f
    out = lap.laplace(logpost, np.array([u0]))
    _report("resolution", factor=factor, n_iter=out.n_iter, logpost=float(out.logpost), kept_before=f_keep)
    assert bool(out.converged) and abs(out.mode[0]) < 1e-5                  # g = -u: converged means |u| < gtol
    if accepted:
        assert out.n_iter == 2 and out.logpost == f_keep - factor * res < f_keep
    else:
        assert out.n_iter > 2 and out.logpost > f_keep


# ---- 6. determinism ----------------------------------------------------------------------------------------------------
def test_repeated_calls_give_identical_bits():
    k, n_c = 12, 7
    A, m, c0, starts, logpost = lo.quadratic(k, n_c, seed=3)
    h = lap.default_step(starts)
    out = []
    for _ in range(2):
        dv = lap.DeviceSteps(n_c, k, h)
        vals = logpost(dv.stencil(starts))
        g, H, _ = dv.grad_hess(vals)
        delta, logdet, ok = dv.newton(g, H, np.full(n_c, 0.25))
        out.append((g, H, delta, logdet))
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
