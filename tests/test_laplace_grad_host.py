"""
rodeo_amd.inference.laplace.laplace_grad on the host (no GPU): the interface, the refusals that come before any device work,
the NumPy restatement tests/laplace_grad_oracle.py of its two kernels (by hand for k = 2, against the leading rows of the
value-mode stencil, exact on quadratics within the rounding bound the formula implies), and the driver itself on a NumPy
stand-in for the device steps: on quadratics, and on a small FitzHugh-Nagumo Fenrir fit built on tests/fenrir_grad_oracle.py,
where ``check_grad`` must pass the correct chain rule and catch two wrong ones.

Tolerances come from the formulas.  A first difference of gradients that carry a relative error r has an absolute error of at
most r max|g| / h; on a quadratic a central difference has no truncation error, so against the matrix A the restated Hessian
is held to 16 eps max|g| / h_min (r = 4 eps: the rounding of the gradients and of the points), and the difference quotient of
the values to 16 eps max|f| / h_min.
"""
import inspect
import numpy as np
import pytest
from rodeo_amd import _lib
from rodeo_amd.inference import laplace as lap
import laplace_oracle as lo
import laplace_grad_oracle as lgo

EPS = np.finfo(np.float64).eps


def _report(name, **figs):
    print("laplace_grad_check " + name + "  " + "  ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}"
                                                         for k, v in figs.items()))


# ---- interface ---------------------------------------------------------------------------------------------------------------
def test_interface():
    sig = inspect.signature(lap.laplace_grad)
    assert list(sig.parameters) == ["value_and_grad", "upars_init", "step", "max_iter", "gtol", "n_samples", "key", "check_grad"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in sig.parameters.items()
               if n not in ("value_and_grad", "upars_init"))
    d = {n: p.default for n, p in sig.parameters.items()}
    assert (d["step"], d["max_iter"], d["gtol"], d["n_samples"], d["key"], d["check_grad"]) == (None, 50, 1e-5, 0, None, True)
    assert lap.n_stencil_grad(5) == 11 and lap.n_stencil_grad(12) == 25 and lap.GRAD_PARITY == 1e-7
    lib = _lib.load()
    for name in ("rk_fd_grad_stencil", "rk_fd_hess_from_grad"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    for name in ("grad_stencil", "hess_from_grad", "newton"):
        assert callable(getattr(lap.DeviceGradSteps, name))
    # the value mode is what it was
    assert list(inspect.signature(lap.laplace).parameters) == ["logpost", "upars_init", "step", "max_iter", "gtol", "n_samples", "key"]
    assert lap.LaplaceResult._fields == ("mode", "logpost", "hessian", "cov", "log_evidence", "converged", "n_iter", "n_bad",
                                         "samples")
    for name in ("stencil", "grad_hess", "newton"):
        assert callable(getattr(lap.DeviceSteps, name))


def test_default_grad_step_is_the_cube_root_of_eps_scaled():
    u = np.array([[0.5, -3.0], [0.1, 2.0]])
    np.testing.assert_array_equal(lap.default_grad_step(u), EPS ** (1 / 3) * np.maximum(1.0, np.max(np.abs(u), axis=0)))
    np.testing.assert_array_equal(lap.default_grad_step(u[0]), EPS ** (1 / 3) * np.array([1.0, 3.0]))


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_stencil_and_formulas_k2_by_hand():
    u, h = np.array([[1.0, 10.0]]), np.array([0.5, 2.0])
    hand = np.array([[1.0, 10.0],
                     [1.5, 10.0], [0.5, 10.0],                               # +- h_0
                     [1.0, 12.0], [1.0, 8.0]])                               # +- h_1
    np.testing.assert_array_equal(lgo.grad_stencil(u, h)[0], hand)
    # values and gradients written down, not derived from a function: every entry of the formulas is told apart
    vals = np.array([[7.0, 9.0, 4.0, 1.0, 13.0]])
    grads = np.array([[[3.0, -5.0],
                       [4.0, 2.0], [1.0, -6.0],                              # G[1], G[2]: at u +- h_0 e_0
                       [11.0, 7.0], [-1.0, -9.0]]])                          # G[3], G[4]: at u +- h_1 e_1
    g, H, bad, g_fd = lgo.hess_from_grad(vals, grads, h)
    np.testing.assert_array_equal(g[0], [3.0, -5.0])
    np.testing.assert_array_equal(g_fd[0], [(9.0 - 4.0) / 1.0, (1.0 - 13.0) / 4.0])
    h01 = 0.5 * ((2.0 - -6.0) / 1.0 + (11.0 - -1.0) / 4.0)                   # mean of d g_1 / d u_0 and d g_0 / d u_1
    np.testing.assert_array_equal(H[0], [[(4.0 - 1.0) / 1.0, h01], [h01, (7.0 - -9.0) / 4.0]])
    assert h01 == 5.5 and bad[0] == 0


@pytest.mark.parametrize("k", [1, 2, 5, 12])
def test_the_stencil_is_the_leading_rows_of_the_value_mode_stencil(k):
    rng = np.random.default_rng(k)
    u, h = rng.standard_normal((7, k)) * 3.0, rng.uniform(1e-6, 1e-2, k)
    pts = lgo.grad_stencil(u, h)
    assert pts.shape == (7, 2 * k + 1, k)
    np.testing.assert_array_equal(pts, lo.stencil(u, h)[:, :2 * k + 1])


@pytest.mark.parametrize("n_c", [1, 7])
@pytest.mark.parametrize("k", [1, 2, 5, 12])
def test_restatement_is_exact_on_quadratics_within_the_rounding_bound(k, n_c):
    A, m, c0, starts, vg = lgo.quadratic_vg(k, n_c, seed=k)
    h = lap.default_grad_step(starts)
    vals, grads = vg(lgo.grad_stencil(starts, h).reshape(-1, k))
    vals, grads = vals.reshape(n_c, -1), grads.reshape(n_c, -1, k)
    g, H, bad, g_fd = lgo.hess_from_grad(vals, grads, h)
    gmax, fmax, hmin = float(np.max(np.abs(grads))), float(np.max(np.abs(vals))), float(np.min(h))
    e_H, e_fd = float(np.max(np.abs(H + A))), float(np.max(np.abs(g_fd - g)))
    _report("restated_quadratic", k=k, C=n_c, hess_err=e_H, bound=16 * EPS * gmax / hmin, in_eps_g_over_h=e_H / (EPS * gmax / hmin),
            grad_fd_err=e_fd, bound_fd=16 * EPS * fmax / hmin)
    assert np.all(bad == 0)
    np.testing.assert_array_equal(g, grads[:, 0])
    assert e_H <= 16 * EPS * gmax / hmin
    assert np.array_equal(H, np.swapaxes(H, 1, 2))                                   # symmetric bit for bit
    assert e_fd <= 16 * EPS * fmax / hmin


def test_a_non_finite_value_or_gradient_entry_is_counted_and_poisons_its_centre_only():
    k, n_c = 3, 3
    A, m, c0, starts, vg = lgo.quadratic_vg(k, n_c, seed=5)
    h = lap.default_grad_step(starts)
    vals, grads = vg(lgo.grad_stencil(starts, h).reshape(-1, k))
    vals, grads = vals.reshape(n_c, -1), grads.reshape(n_c, -1, k)
    clean = lgo.hess_from_grad(vals, grads, h)
    for bad_value in (np.nan, np.inf, -np.inf):
        for where in ("value", "gradient"):
            v, G = vals.copy(), grads.copy()
            if where == "value":
                v[1, 4] = bad_value
            else:
                G[1, 6, 2] = bad_value
            g, H, bad, g_fd = lgo.hess_from_grad(v, G, h)
            assert list(bad) == [0, 1, 0]
            assert np.all(np.isnan(g[1])) and np.all(np.isnan(H[1])) and np.all(np.isnan(g_fd[1]))
            for c in (0, 2):
                for got, want in zip((g, H, g_fd), (clean[0], clean[1], clean[3])):
                    np.testing.assert_array_equal(got[c], want[c])
    v, G = vals.copy(), grads.copy()
    v[2, :], G[2, :, 0] = np.nan, np.inf
    assert list(lgo.hess_from_grad(v, G, h)[2]) == [0, 0, 2 * (2 * k + 1)]


# ---- refusals: ValueError before any device work --------------------------------------------------------------------------------
def _quad(u):
    u = np.asarray(u)
    return -0.5 * np.sum(u ** 2, axis=1), -u


@pytest.fixture
def no_device(monkeypatch):
    def fail():
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(lap, "default_device", fail)


def test_what_laplace_refuses_is_refused_under_the_new_name(no_device):
    for start in (np.zeros(13), np.zeros((3, 13))):
        with pytest.raises(ValueError, match="laplace_grad: k <= 12"):
            lap.laplace_grad(_quad, start)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="laplace_grad: upars_init is not finite"):
            lap.laplace_grad(_quad, np.array([0.0, bad, 1.0]))
    for start in (np.zeros((2, 2, 2)), np.zeros(0)):
        with pytest.raises(ValueError, match="laplace_grad: upars_init must have shape"):
            lap.laplace_grad(_quad, start)
    for step in (0.0, -1e-3, np.nan, [1e-3, 0.0]):
        with pytest.raises(ValueError, match="laplace_grad: step"):
            lap.laplace_grad(_quad, np.zeros(2), step=step)
    with pytest.raises(ValueError, match="laplace_grad: n_samples > 0 needs an integer key"):
        lap.laplace_grad(_quad, np.zeros(2), n_samples=10)


def test_a_result_that_is_not_a_pair_of_the_right_shapes_is_refused(no_device):
    n_c, k = 4, 3
    wrong = [lambda u: _quad(u)[0],                                          # the value alone
             lambda u: _quad(u) + (0,),                                      # three things
             lambda u: (_quad(u)[0][:-1], _quad(u)[1]),                      # a value short
             lambda u: (_quad(u)[0][:, None], _quad(u)[1]),                  # values (B, 1)
             lambda u: (_quad(u)[0], _quad(u)[1][:, :-1]),                   # gradient (B, k - 1)
             lambda u: (_quad(u)[0], _quad(u)[1].T),                         # gradient (k, B)
             lambda u: (0.0, np.zeros(k))]                                   # not batched
    for fn in wrong:
        with pytest.raises(ValueError, match=r"laplace_grad: value_and_grad must return .*\(4,\), \(4, 3\)\).* at upars_init"):
            lap.laplace_grad(fn, np.zeros((n_c, k)))


def test_a_non_finite_value_or_gradient_at_the_start_is_refused(no_device):
    with np.errstate(invalid="ignore", divide="ignore"):
        with pytest.raises(ValueError, match="laplace_grad: value_and_grad is not finite at upars_init"):
            lap.laplace_grad(lambda u: (np.log(u[:, 0]), np.stack([1.0 / u[:, 0], 0.0 * u[:, 1]], axis=1)),
                             np.array([[1.0, 2.0], [-1.0, 2.0]]))
        with pytest.raises(ValueError, match="laplace_grad: value_and_grad is not finite at upars_init"):
            lap.laplace_grad(lambda u: (0.0 * u[:, 0], np.stack([1.0 / u[:, 0], 0.0 * u[:, 1]], axis=1)), np.array([0.0, 2.0]))


# ---- the driver on a NumPy stand-in for the device steps ------------------------------------------------------------------------
@pytest.fixture
def host_steps(monkeypatch):
    monkeypatch.setattr(lap, "DeviceGradSteps", lgo.HostGradSteps)


def quadratic_tolerances(A, m, c0, starts, vg):
    """The tolerances of tests/test_gpu_laplace.py's ``test_newton_lands_on_the_mode_of_a_quadratic`` with the gradient mode's
    error terms: b_H = 16 eps max|g| / h_min for the Hessian and b_g = 4 eps max|g| for the gradient (it is the user's, not a
    difference quotient), max|g| over the stencil of the starts.  Also used by tests/test_gpu_laplace_grad.py."""
    k = len(m)
    h = lap.default_grad_step(starts)
    gmax = float(np.max(np.abs(vg(lgo.grad_stencil(starts, h).reshape(-1, k))[1])))
    b_H, b_g = 16 * EPS * gmax / np.min(h), 4 * EPS * gmax
    lam = np.linalg.eigvalsh(A)
    dist = float(np.max(np.linalg.norm(starts - m, axis=1)))
    tol_mode = (np.sqrt(k) * b_g + k * b_H * dist) / lam[0]
    tol_cov = k * b_H / lam[0] ** 2 * 2
    ev = c0 + 0.5 * k * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(A)[1]
    tol_ev = 0.5 * k * b_H / lam[0] * 2 + 4 * EPS * abs(ev) + 0.5 * lam[-1] * k * tol_mode ** 2
    return dict(h=h, b_H=float(b_H), tol_mode=float(tol_mode), tol_cov=float(tol_cov), ev=float(ev), tol_ev=float(tol_ev))


def check_quadratic_fit(res, A, m, tol, name, k, n_c):
    e_mode, e_cov = float(np.max(np.abs(res.mode - m))), float(np.max(np.abs(res.cov - np.linalg.inv(A))))
    e_ev, e_H = float(np.max(np.abs(res.log_evidence - tol["ev"]))), float(np.max(np.abs(res.hessian + A)))
    _report(name, k=k, C=n_c, n_iter=res.n_iter, mode_err=e_mode, tol_mode=tol["tol_mode"], cov_err=e_cov, tol_cov=tol["tol_cov"],
            evidence_err=e_ev, tol_evidence=tol["tol_ev"], hess_err=e_H, b_H=tol["b_H"])
    assert res.mode.shape == (n_c, k)
    assert np.all(res.converged) and res.n_iter == 2 and np.all(res.n_bad == 0)
    assert e_mode <= tol["tol_mode"] and e_cov <= tol["tol_cov"] and e_ev <= tol["tol_ev"] and e_H <= tol["b_H"]


@pytest.mark.parametrize("n_c", [1, 7])
@pytest.mark.parametrize("k", [1, 2, 5, 12])
def test_the_driver_lands_on_the_mode_of_a_quadratic_in_two_iterations(k, n_c, host_steps):
    A, m, c0, starts, vg = lgo.quadratic_vg(k, n_c, seed=k)
    tol = quadratic_tolerances(A, m, c0, starts, vg)
    calls = []

    def counted(u):
        calls.append(len(u))
        return vg(u)
    res = lap.laplace_grad(counted, starts)
    check_quadratic_fit(res, A, m, tol, "host_driver_quadratic", k, n_c)
    assert calls == [n_c] + [n_c * (2 * k + 1)] * 2                                   # the start, then one batched call an iteration
    one = lap.laplace_grad(vg, starts[0], step=tol["h"])                              # a (k,) start drops the centre axis
    assert one.mode.shape == (k,) and one.hessian.shape == (k, k) and bool(one.converged) and one.samples is None
    np.testing.assert_array_equal(one.mode, res.mode[0])


def test_later_bad_points_are_counted_and_a_later_wrong_shape_is_refused(host_steps):
    # f = log u - u from u = 3: the undamped step goes to u = -3, where value and gradient stencils are NaN
    def vg(u):
        with np.errstate(invalid="ignore"):
            return np.log(u[:, 0]) - u[:, 0], 1.0 / np.where(u > 0, u, np.nan) - 1.0
    res = lap.laplace_grad(vg, np.array([[3.0], [0.9]]))
    assert np.all(res.converged) and res.n_bad[0] > 0 and res.n_bad[1] == 0
    np.testing.assert_allclose(res.mode[:, 0], [1.0, 1.0], atol=1e-5)
    np.testing.assert_allclose(res.hessian[:, 0, 0], [-1.0, -1.0], atol=1e-5)
    calls = []

    def short(u):
        calls.append(len(u))
        f, g = _quad(u)
        return (f, g) if len(calls) < 3 else (f, g[:-1])
    with pytest.raises(ValueError, match=r"\(\(14,\), \(13, 3\)\)"):
        lap.laplace_grad(short, np.ones((2, 3)))
    assert calls == [2, 14, 14]


# ---- FitzHugh-Nagumo, Fenrir, theta and x(0): k = 5 -----------------------------------------------------------------------------
# The smallest shape found at which the fit behaves (searched on the CPU restatement, t_max = 5, six observations of both
# variables, start 0.02 off the truth in every coordinate): N = 10 and N = 15 do not converge in 50 iterations (N = 15 ends on an
# indefinite Hessian), N = 20 converges but from 0.05 off needs 15 iterations, N = 30 needs six and its Hessian has eigenvalues
# from -2.1e3 to -2.4.  One iteration is 11 points x 9 directions of the pure-NumPy recursion, about 0.7 s.
FHN_SHAPE = dict(N=30, t_max=5.0, n_obs=6)
FHN_START_OFFSET = 0.02


class memo:
    """A backend whose results are kept by the bytes of its arguments: the wrong chain rules and the check at the mode ask for
    stencils the fit has evaluated already."""

    def __init__(self, backend):
        self.backend, self.kept, self.calls = backend, {}, 0

    def __call__(self, X0, th, J):
        key = (X0.tobytes(), th.tobytes(), None if J is None else J.tobytes())
        if key not in self.kept:
            self.calls += 1
            self.kept[key] = self.backend(X0, th, J)
        return self.kept[key]


@pytest.fixture(scope="module")
def fhn():
    case = lgo.fhn_case(**FHN_SHAPE)
    backend = memo(lgo.fhn_oracle_backend(case))
    start = np.concatenate([np.log(case["theta"]), case["x0"]]) + FHN_START_OFFSET
    saved = lap.DeviceGradSteps
    lap.DeviceGradSteps = lgo.HostGradSteps
    try:
        fit = lap.laplace_grad(lgo.fhn_value_and_grad(case, backend), start)
    finally:
        lap.DeviceGradSteps = saved
    return dict(case=case, backend=backend, start=start, fit=fit)


def test_fitzhugh_nagumo_fit_converges_on_the_restatement(fhn):
    fit, case = fhn["fit"], fhn["case"]
    eig = np.linalg.eigvalsh(fit.hessian)
    _report("host_fitzhugh", n_iter=fit.n_iter, logpost=float(fit.logpost), eig_max=float(eig[-1]), eig_min=float(eig[0]),
            theta=np.array2string(np.exp(fit.mode[:3]), precision=4), x0=np.array2string(fit.mode[3:], precision=4))
    assert bool(fit.converged) and fit.n_bad == 0 and np.all(eig < 0)
    g_mode = lgo.fhn_value_and_grad(case, fhn["backend"])(fit.mode[None])[1]
    assert np.max(np.abs(g_mode)) < 1e-5                                              # the exact gradient, not a quotient
    assert np.max(np.abs(np.exp(fit.mode[:3]) - case["theta"])) < 0.5 and np.all(np.isfinite(fit.cov))   # a fit, not a stray point


def test_check_grad_passes_the_right_chain_rule_and_catches_two_wrong_ones(fhn, host_steps):
    case, backend = fhn["case"], fhn["backend"]
    for at in (fhn["start"], fhn["fit"].mode):                                        # (the fit itself has passed it at the start)
        lap.laplace_grad(lgo.fhn_value_and_grad(case, backend), at, max_iter=1)
    for chain in ("no_theta_factor", "no_init_jac"):
        vg = lgo.fhn_value_and_grad(case, backend, chain=chain)
        with pytest.raises(ValueError, match=r"laplace_grad: the gradient of value_and_grad disagrees .* centre 0, coordinate "
                                             r"[0-2]: gradient .* above the bar") as err:
            lap.laplace_grad(vg, fhn["start"], max_iter=1)
        print("laplace_grad_check host_" + chain + "  " + str(err.value))
        res = lap.laplace_grad(vg, fhn["start"], max_iter=1, check_grad=False)        # silent: the user has asked for it
        assert res.n_iter == 1 and not bool(res.converged)


# ---- pull_back ------------------------------------------------------------------------------------------------------------------
def test_pull_back_is_the_contraction_an_explicit_loop_gives():
    rng = np.random.default_rng(0)
    B, k = 4, 5
    grad = dict(theta=rng.standard_normal((B, 3)), ode_init=rng.standard_normal((B, 2, 3)), unused=rng.standard_normal((B, 2)))
    jac = dict(theta=rng.standard_normal((B, 3, k)), ode_init=rng.standard_normal((B, 2, 3, k)))
    want = np.zeros((B, k))
    for b in range(B):
        for j in range(k):
            for i in range(3):
                want[b, j] += grad["theta"][b, i] * jac["theta"][b, i, j]
            for r in range(2):
                for s in range(3):
                    want[b, j] += grad["ode_init"][b, r, s] * jac["ode_init"][b, r, s, j]
    got = lap.pull_back(grad, jac)
    assert got.shape == (B, k)
    np.testing.assert_allclose(got, want, rtol=0, atol=8 * EPS * np.max(np.abs(want)))
    np.testing.assert_array_equal(lap.pull_back(grad, dict(theta=jac["theta"])),
                                  np.einsum("bi,bik->bk", grad["theta"], jac["theta"]))
    with pytest.raises(ValueError, match="pull_back: jac has 'sigma'"):
        lap.pull_back(grad, dict(sigma=np.zeros((B, 2, k))))
    with pytest.raises(ValueError, match=r"pull_back: jac\['theta'\] must have shape"):
        lap.pull_back(grad, dict(theta=np.zeros((B, k, 3, 2))))
