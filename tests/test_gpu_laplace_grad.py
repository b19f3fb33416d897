"""
rodeo_amd.inference.laplace.laplace_grad on the device: the two kernels (rk_fd_grad_stencil, rk_fd_hess_from_grad) against the
NumPy restatement tests/laplace_grad_oracle.py bit for bit, and the driver on quadratics (exact answers), on a linear system
whose log-likelihood is exactly quadratic in the initial value (``fenrir_grad`` / ``dalton_grad`` against unit-step differences
of the CPU oracles), and on the FitzHugh-Nagumo parameters of tests/test_laplace_grad_host.py (``fenrir_grad`` against the same
driver around the CPU restatement, and against the value-mode ``laplace`` on the device).

Tolerances come from the formulas, not from what the device gives.  With g the gradient of the log-posterior, h the step and
eps = 2^-52: a first difference of gradients that carry a relative error r has an absolute error of at most r max|g| / h.  On a
quadratic a central difference has no truncation error, so against the matrix A the Hessian is held to 16 eps max|g| / h_min
(r = 4 eps: the rounding of the gradients and of the points); against an independent implementation of the gradient, r =
GRAD_PARITY = 1e-7 is the bar tests/test_gpu_fenrir_grad.py and tests/test_gpu_dalton_grad.py hold the device to.  Every figure
is printed before it is asserted (profiles/laplace_grad_checks.txt keeps one run's output).
"""
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd import _lib
from rodeo_amd.inference import laplace as lap
from rodeo_amd.inference.fenrir import fenrir_grad
from rodeo_amd.inference.dalton import dalton_grad
from rodeo_amd.interrogate import interrogate_kramer
from oracle import fenrir as ofen, priors, interrogations as oi
import dalton_oracle
import laplace_oracle as lo
import laplace_grad_oracle as lgo
from test_laplace_grad_host import (quadratic_tolerances, check_quadratic_fit, _report, FHN_SHAPE, FHN_START_OFFSET, memo)

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
PARITY = 1e-7                        # device log-density against the oracles (tests/test_gpu_laplace.py)
GRAD_PARITY = lap.GRAD_PARITY


# ---- 1. the kernels on quadratics ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_c", [1, 7])
@pytest.mark.parametrize("k", [1, 2, 5, 12])
def test_kernels_equal_the_restatement_bit_for_bit_on_a_quadratic(k, n_c):
    A, m, c0, starts, vg = lgo.quadratic_vg(k, n_c, seed=k)
    h = lap.default_grad_step(starts)
    dv = lap.DeviceGradSteps(n_c, k, h)
    pts = dv.grad_stencil(starts)
    assert pts.shape == (n_c * (2 * k + 1), k)
    np.testing.assert_array_equal(pts, lgo.grad_stencil(starts, h).reshape(-1, k))                    # same points, order, bits
    full = lap.DeviceSteps(n_c, k, h).stencil(starts).reshape(n_c, -1, k)
    np.testing.assert_array_equal(pts.reshape(n_c, -1, k), full[:, :2 * k + 1])                       # rk_fd_stencil's leading rows
    vals, grads = vg(pts)
    out = dv.hess_from_grad(vals, grads)
    ref = lgo.hess_from_grad(vals.reshape(n_c, -1), grads.reshape(n_c, -1, k), h)
    g, H, bad, g_fd = out
    gmax, hmin = float(np.max(np.abs(grads))), float(np.min(h))
    e_H = float(np.max(np.abs(H + A)))
    _report("quadratic", k=k, C=n_c, hess_vs_A=e_H, bound=16 * EPS * gmax / hmin, in_eps_g_over_h=e_H / (EPS * gmax / hmin),
            grad_fd_vs_grad=float(np.max(np.abs(g_fd - g))), dev_vs_numpy_H=float(np.max(np.abs(H - ref[1]))))
    assert bad.dtype == np.int32 and np.all(bad == 0)
    for got, want in zip(out, ref):                     # one expression per entry, IEEE operations, same order: the same bits
        np.testing.assert_array_equal(got, want)
    assert e_H <= 16 * EPS * gmax / hmin
    assert np.array_equal(H, np.swapaxes(H, 1, 2))                                                    # symmetric by construction
    again = lap.DeviceGradSteps(n_c, k, h)
    assert again.grad_stencil(starts).tobytes() == pts.tobytes()
    for a, b in zip(again.hess_from_grad(vals, grads), out):
        assert a.tobytes() == b.tobytes()


def test_a_non_finite_entry_is_counted_and_poisons_its_centre_only():
    k, n_c = 3, 3
    A, m, c0, starts, vg = lgo.quadratic_vg(k, n_c, seed=5)
    h = lap.default_grad_step(starts)
    dv = lap.DeviceGradSteps(n_c, k, h)
    vals, grads = vg(dv.grad_stencil(starts))
    vals, grads = vals.reshape(n_c, -1), grads.reshape(n_c, -1, k)
    for bad_value in (np.nan, np.inf, -np.inf):
        for where in ("value", "gradient"):
            v, G = vals.copy(), grads.copy()
            if where == "value":
                v[1, 4] = bad_value
            else:
                G[1, 6, 2] = bad_value
            out, ref = dv.hess_from_grad(v, G), lgo.hess_from_grad(v, G, h)
            assert list(out[2]) == [0, 1, 0]
            for got, want in zip(out, ref):
                np.testing.assert_array_equal(got, want)                                              # (NaN where the restatement has NaN)
    v, G = vals.copy(), grads.copy()
    v[2, :], G[2, :, 0] = np.nan, np.inf
    assert list(dv.hess_from_grad(v, G)[2]) == [0, 0, 2 * (2 * k + 1)]


# ---- 2. the driver on quadratics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_c", [1, 7])
@pytest.mark.parametrize("k", [1, 2, 5, 12])
def test_the_driver_lands_on_the_mode_of_a_quadratic_in_two_iterations(k, n_c):
    A, m, c0, starts, vg = lgo.quadratic_vg(k, n_c, seed=k)
    tol = quadratic_tolerances(A, m, c0, starts, vg)
    res = lap.laplace_grad(vg, starts, n_samples=4000, key=11)
    check_quadratic_fit(res, A, m, tol, "driver_quadratic", k, n_c)
    assert res.samples.shape == (n_c, 4000, k)
    sd = np.sqrt(np.diagonal(res.cov, axis1=1, axis2=2))
    assert np.max(np.abs(res.samples.mean(axis=1) - res.mode) / sd) < 5 / np.sqrt(4000)
    one = lap.laplace_grad(vg, starts[0], step=tol["h"])                              # a (k,) start drops the centre axis
    assert one.mode.shape == (k,) and one.hessian.shape == (k, k) and bool(one.converged) and one.samples is None
    np.testing.assert_array_equal(one.mode, res.mode[0])


# ---- 3. real log-densities, exact answer -----------------------------------------------------------------------------------------
# x' = v, v' = sin 2t - x as two first-order blocks (the gradient kernels refuse ``higher_order``), traced from plain Python.
N_LIN, P_LIN, OM = 10, 3, 0.05


def _lin(X, t):
    return np.array([[X[1, 0]], [np.sin(2 * t) - X[0, 0]]])


class _LinOracle:
    """The same right-hand side for the CPU oracles, with the block-diagonal Jacobian they ask for: it is zero (each block's
    derivative depends on the other block only), so kramer's linearisation is exact here and the filter means are affine in x(0)."""

    def __call__(self, X, t):
        X = np.asarray(X)
        return np.stack([X[..., 1, 0], np.sin(2 * t) - X[..., 0, 0]], axis=-1)[..., None]

    def jac(self, X, t):
        return np.zeros(np.shape(X)[:-1] + (1, np.shape(X)[-1]))


def _x0_lin(u):
    """(x(0), v(0)) -> the padded state [[x, v, 0], [v, sin 0 - x, 0]]: (B, 2, 3)."""
    u = np.atleast_2d(u)
    z = np.zeros(len(u))
    return np.stack([np.stack([u[:, 0], u[:, 1], z], axis=1), np.stack([u[:, 1], -u[:, 0], z], axis=1)], axis=1)


JAC_LIN = np.zeros((2, 3, 2))                                                        # d (padded state) / d u, constant
JAC_LIN[0, 0, 0], JAC_LIN[0, 1, 1], JAC_LIN[1, 0, 1], JAC_LIN[1, 1, 0] = 1.0, 1.0, 1.0, -1.0


@pytest.mark.parametrize("method", ["fenrir", "dalton"])
def test_linear_system_has_the_exact_mode_and_hessian(method):
    W, init = ra.utils.first_order_pad(_lin, 2, P_LIN)
    np.testing.assert_array_equal(init(np.array([-1.0, 0.5]), 0.0), _x0_lin(np.array([-1.0, 0.5]))[0])
    Q, R = priors.ibm_init(1.0 / N_LIN, P_LIN, np.array([0.5, 0.5]))
    obs_times = np.array([0.2, 0.5, 1.0])
    y = np.zeros((3, 2, 1, ))
    y[:, 0, 0] = np.random.default_rng(0).standard_normal(3) * 0.3 - 0.5             # three observations of x; the block of v
    ow = np.zeros((3, 2, 1, P_LIN)); ow[:, 0, 0, 0] = 1.0                            # has a zero row: a constant term
    ov = np.full((3, 2, 1, 1), OM)
    dev_fn = {"fenrir": fenrir_grad, "dalton": dalton_grad}[method]

    def value_and_grad(u):
        res = dev_fn(None, _lin, W, _x0_lin(u), 0.0, 1.0, N_LIN, interrogate_kramer, (Q, R), y, obs_times, ow, ov, wrt=("ode_init",))
        return res.value, lap.pull_back(res.grad, dict(ode_init=np.broadcast_to(JAC_LIN, (len(u),) + JAC_LIN.shape)))

    ode = _LinOracle()

    def exact(u):
        if method == "fenrir":
            return float(ofen.fenrir(None, ode, W, _x0_lin(u)[0], 0.0, 1.0, N_LIN, oi.interrogate_kramer, (Q, R), y, obs_times, ow, ov))
        return float(dalton_oracle.dalton(ode, W, _x0_lin(u)[0], 0.0, 1.0, N_LIN, oi.interrogate_kramer, (Q, R), y, obs_times, ow, ov))

    # the log-likelihood is a quadratic in u: its gradient and Hessian at `start` from oracle evaluations, unit steps
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
    h = 0.1                                                                          # exactly quadratic: no truncation error
    res = lap.laplace_grad(value_and_grad, start, step=h)
    # max|g| over everything the run evaluates: the stencils at the start and at the mode, from the exact quadratic
    pts = np.concatenate([lgo.grad_stencil(start[None], [h, h])[0], lgo.grad_stencil(mode_ex[None], [h, h])[0]])
    gmax = float(np.max(np.abs(g_ex + (pts - start) @ H_ex)))
    tol_H = GRAD_PARITY * gmax / h
    tol_mode = np.linalg.norm(np.linalg.inv(H_ex), 2) * (np.sqrt(2) * GRAD_PARITY * gmax + 2 * tol_H * np.linalg.norm(mode_ex - start))
    e_H, e_mode = float(np.max(np.abs(res.hessian - H_ex))), float(np.max(np.abs(res.mode - mode_ex)))
    _report("linear_" + method, n_iter=res.n_iter, hess_err=e_H, tol_hess=tol_H, mode_err=e_mode, tol_mode=float(tol_mode),
            max_g=gmax, logpost_err=float(abs(res.logpost - exact(mode_ex))), hess_scale=float(np.max(np.abs(H_ex))))
    assert bool(res.converged) and res.n_bad == 0 and np.all(np.linalg.eigvalsh(H_ex) < 0)
    assert e_H <= tol_H and e_mode <= tol_mode


# ---- 4. nonlinear parameters -----------------------------------------------------------------------------------------------------
def _device_backend(case, fn):
    c = case

    def backend(X0, th, init_jac):
        res = fn(None, ra.ode.fitzhugh_nagumo, c["W"], X0, 0.0, c["t_max"], c["N"], interrogate_kramer, c["prior"], c["y"],
                 c["obs_times"], c["ow"], c["ov"], wrt=("theta", "ode_init"),
                 init_jac=None if init_jac is None else dict(theta=init_jac), theta=th)
        return res.value, res.grad
    return backend


@pytest.fixture(scope="module")
def fhn():
    case = lgo.fhn_case(**FHN_SHAPE)
    start = np.concatenate([np.log(case["theta"]), case["x0"]]) + FHN_START_OFFSET
    return dict(case=case, start=start)


def _logpost_for(case, fn):
    def logpost(u):
        th = np.exp(u[:, :3])
        X0 = np.stack([case["init"](u[b, 3:5], 0.0, theta=th[b]) for b in range(len(u))])
        ll = fn(None, ra.ode.fitzhugh_nagumo, case["W"], X0, 0.0, case["t_max"], case["N"], interrogate_kramer, case["prior"],
                case["y"], case["obs_times"], case["ow"], case["ov"], theta=th)
        return ll + np.sum(-0.5 * (u / 10.0) ** 2 - np.log(10.0) - 0.5 * np.log(2 * np.pi), axis=1)
    return logpost


def _cross_mode(name, case, start, dev, vg_dev, value_fn, gtol):
    """``laplace`` (differences of values) on the device log-posterior of the same case against ``laplace_grad``: the bounds of
    tests/test_gpu_laplace.py's test_fitzhugh_nagumo_parameters_agree_with_the_driver_on_the_cpu_oracle."""
    val = lap.laplace(_logpost_for(case, value_fn), start, gtol=gtol)
    h2 = float(np.min(lap.default_step(start)))
    fmax = max(1.0, abs(float(dev.logpost)))
    tol_H, tol_g = 4 * PARITY * fmax / h2 ** 2, PARITY * fmax / h2
    tol_mode = np.linalg.norm(np.linalg.inv(dev.hessian), 2) * np.sqrt(5) * (2 * gtol + tol_g)
    e_H, e_mode = float(np.max(np.abs(val.hessian - dev.hessian))), float(np.max(np.abs(val.mode - dev.mode)))
    g_at_val = vg_dev(val.mode[None])[1]
    _report(name, n_iter_value_mode=val.n_iter, n_iter_grad_mode=dev.n_iter, hess_diff=e_H, tol_hess=tol_H, mode_diff=e_mode,
            tol_mode=float(tol_mode), exact_grad_at_value_mode=float(np.max(np.abs(g_at_val))))
    assert bool(val.converged)
    assert e_H <= tol_H and e_mode <= tol_mode


def test_fitzhugh_nagumo_fenrir_agrees_with_the_driver_on_the_cpu_restatement(fhn, monkeypatch):
    case, start, gtol = fhn["case"], fhn["start"], 1e-5
    vg_dev = lgo.fhn_value_and_grad(case, _device_backend(case, fenrir_grad))
    dev = lap.laplace_grad(vg_dev, start, gtol=gtol)
    vg_cpu = lgo.fhn_value_and_grad(case, memo(lgo.fhn_oracle_backend(case)))
    with monkeypatch.context() as mp:
        mp.setattr(lap, "DeviceGradSteps", lgo.HostGradSteps)
        cpu = lap.laplace_grad(vg_cpu, start, gtol=gtol)
    h = lap.default_grad_step(start)
    hmin = float(np.min(h))
    gmax = float(np.max(np.abs(vg_cpu(lgo.grad_stencil(cpu.mode[None], h)[0])[1])))   # over the stencil the Hessian comes from
    tol_H = GRAD_PARITY * gmax / hmin
    # both runs stop where their own gradient is below gtol: the modes differ by at most |H^-1| (2 gtol + gradient parity)
    tol_mode = np.linalg.norm(np.linalg.inv(cpu.hessian), 2) * np.sqrt(5) * (2 * gtol + GRAD_PARITY * gmax)
    g_mode = vg_dev(dev.mode[None])[1]
    e_H, e_mode = float(np.max(np.abs(dev.hessian - cpu.hessian))), float(np.max(np.abs(dev.mode - cpu.mode)))
    _report("fitzhugh_fenrir", n_iter_dev=dev.n_iter, n_iter_cpu=cpu.n_iter, grad_at_mode=float(np.max(np.abs(g_mode))),
            hess_diff=e_H, tol_hess=tol_H, hess_scale=float(np.max(np.abs(cpu.hessian))), max_g=gmax, mode_diff=e_mode,
            tol_mode=float(tol_mode), logpost_diff=float(abs(dev.logpost - cpu.logpost)))
    assert bool(dev.converged) and bool(cpu.converged) and dev.n_bad == 0
    assert np.max(np.abs(g_mode)) < gtol                                              # the exact gradient, not a quotient
    assert np.all(np.linalg.eigvalsh(dev.hessian) < 0)
    assert e_H <= tol_H and e_mode <= tol_mode
    assert np.max(np.abs(np.exp(dev.mode[:3]) - case["theta"])) < 0.5 and np.all(np.isfinite(dev.cov))
    _cross_mode("fitzhugh_fenrir_cross_mode", case, start, dev, vg_dev, ra.inference.fenrir, gtol)
    # a wrong chain rule raises at the start, and does not when the test is switched off
    for chain in ("no_theta_factor", "no_init_jac"):
        wrong = lgo.fhn_value_and_grad(case, _device_backend(case, fenrir_grad), chain=chain)
        with pytest.raises(ValueError, match=r"laplace_grad: the gradient of value_and_grad disagrees .* centre 0, coordinate "
                                             r"[0-2]: gradient .* above the bar") as err:
            lap.laplace_grad(wrong, start, max_iter=1)
        print("laplace_grad_check " + chain + "  " + str(err.value))
        assert lap.laplace_grad(wrong, start, max_iter=1, check_grad=False).n_iter == 1


def test_fitzhugh_nagumo_dalton_agrees_with_the_value_mode(fhn):
    """``dalton_grad`` under ``laplace_grad`` against ``laplace`` on ``dalton`` (the CPU restatement of DALTON's gradient under
    the driver would take this test past its few seconds, so the device's two modes are held against each other).

    ``check_grad=False``: DALTON's value is the difference of two log-densities and carries their rounding, not eps |f|.  Measured
    on this case (f = 2.38): values scatter 4.9e-10 about their tangent line over 21 points 1e-9 apart (Fenrir: 1.8e-14), so at the
    default h = 9.6e-6 the difference quotient is off by 1.8e-5 in coordinate 0 while the bar, whose rounding term is
    2 eps max(|f|, 1) / h, stands at 1.6e-5; at h = 1e-4 quotient and gradient agree to 1.8e-7 and the difference falls as h^2
    down to there, as Fenrir's does down to 2e-10.  The gradient is right; the test's rounding term does not cover DALTON."""
    case, start, gtol = fhn["case"], fhn["start"], 1e-5
    vg_dev = lgo.fhn_value_and_grad(case, _device_backend(case, dalton_grad))
    dev = lap.laplace_grad(vg_dev, start, gtol=gtol, check_grad=False)
    g_mode = vg_dev(dev.mode[None])[1]
    _report("fitzhugh_dalton", n_iter=dev.n_iter, grad_at_mode=float(np.max(np.abs(g_mode))), logpost=float(dev.logpost))
    assert bool(dev.converged) and dev.n_bad == 0 and np.max(np.abs(g_mode)) < gtol
    assert np.all(np.linalg.eigvalsh(dev.hessian) < 0)
    _cross_mode("fitzhugh_dalton_cross_mode", case, start, dev, vg_dev, ra.inference.dalton, gtol)


# ---- 5. failure is visible -------------------------------------------------------------------------------------------------------
def test_a_nan_gradient_entry_at_a_later_stencil_is_counted_and_the_trial_rejected():
    k, n_c = 3, 2
    A, m, c0, starts, vg = lgo.quadratic_vg(k, n_c, seed=7)
    clean = lap.laplace_grad(vg, starts)
    calls = []

    def flawed(u):
        calls.append(len(u))
        f, g = vg(u)
        if len(calls) == 3:                              # the second stencil: one gradient entry of centre 1
            g = g.copy()
            g[(2 * k + 1) + 4, 1] = np.nan
        return f, g
    res = lap.laplace_grad(flawed, starts)
    _report("nan_gradient", n_iter=res.n_iter, n_bad0=int(res.n_bad[0]), n_bad1=int(res.n_bad[1]))
    assert list(res.n_bad) == [0, 1] and np.all(res.converged)
    assert clean.n_iter == 2 and res.n_iter > 2          # the trial of centre 1 was rejected and retaken with damping
    np.testing.assert_array_equal(res.mode[0], clean.mode[0])
    assert np.max(np.abs(res.mode[1] - m)) < 1e-5 / np.linalg.eigvalsh(A)[0] * np.sqrt(k)              # |g| < gtol there


def test_a_later_result_of_the_wrong_shape_is_refused():
    calls = []

    def short(u):
        calls.append(len(u))
        u = np.asarray(u)
        f, g = -0.5 * np.sum(u ** 2, axis=1), -u
        return (f, g) if len(calls) < 3 else (f, g[:-1])
    with pytest.raises(ValueError, match=r"\(\(14,\), \(13, 3\)\)"):
        lap.laplace_grad(short, np.ones((2, 3)))
    assert calls == [2, 14, 14]


def test_the_library_refuses_thirteen_parameters_and_no_centre_and_serves_afterwards():
    dev = ra.default_device()
    buf = dev.zeros((27 * 13 + 13 * 13 + 64,))
    ib = dev.zeros((4,), np.int32)
    assert dev.lib.rk_fd_grad_stencil(dev.h, 1, 13, buf.ptr, buf.ptr, buf.ptr) == _lib.RK_ERR_UNSUPPORTED
    assert dev.lib.rk_fd_hess_from_grad(dev.h, 1, 13, buf.ptr, buf.ptr, buf.ptr, buf.ptr, buf.ptr, buf.ptr,
                                        ib.ptr) == _lib.RK_ERR_UNSUPPORTED
    assert dev.lib.rk_fd_grad_stencil(dev.h, 0, 2, buf.ptr, buf.ptr, buf.ptr) == _lib.RK_ERR_INVALID
    assert dev.lib.rk_fd_hess_from_grad(dev.h, 0, 2, buf.ptr, buf.ptr, buf.ptr, buf.ptr, buf.ptr, buf.ptr, ib.ptr) == _lib.RK_ERR_INVALID
    assert dev.lib.rk_fd_grad_stencil(dev.h, 1, 0, buf.ptr, buf.ptr, buf.ptr) == _lib.RK_ERR_INVALID
    A, m, c0, starts, vg = lgo.quadratic_vg(2, 1, seed=2)                             # a served call works afterwards
    res = lap.laplace_grad(vg, starts)
    assert np.all(res.converged) and np.max(np.abs(res.mode - m)) < 1e-8
