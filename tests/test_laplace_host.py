"""
rodeo_amd.inference.laplace on the host (no GPU): the interface, the refusals that come before any device work, and the
NumPy restatement tests/laplace_oracle.py (stencil order against a hand-written k = 2 case, difference formulas exact on
quadratics within the rounding bound the formula implies, the damped step).
"""
import inspect
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd import _lib
from rodeo_amd.inference import laplace as lap
import laplace_oracle as lo

EPS = np.finfo(np.float64).eps


def test_module_is_exported_and_bound():
    assert ra.inference.laplace is lap
    sig = inspect.signature(lap.laplace)
    assert list(sig.parameters) == ["logpost", "upars_init", "step", "max_iter", "gtol", "n_samples", "key"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in sig.parameters.items() if n not in ("logpost", "upars_init"))
    assert sig.parameters["step"].default is None and sig.parameters["max_iter"].default == 50
    assert lap.LaplaceResult._fields == ("mode", "logpost", "hessian", "cov", "log_evidence", "converged", "n_iter", "n_bad",
                                         "samples")
    lib = _lib.load()
    for name in ("rk_fd_stencil", "rk_fd_grad_hess", "rk_newton_step"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lap.K_MAX == 12 and lap.n_stencil(5) == 51 and lap.n_stencil(12) == 289


def test_default_step_is_the_fourth_root_of_eps_scaled():
    h = lap.default_step(np.array([[0.5, -3.0], [0.1, 2.0]]))
    np.testing.assert_array_equal(h, EPS ** 0.25 * np.array([1.0, 3.0]))
    assert EPS ** 0.25 == 2.0 ** -13


def test_stencil_order_k2_by_hand():
    u, h = np.array([[1.0, 10.0]]), np.array([0.5, 2.0])
    hand = np.array([[1.0, 10.0],
                     [1.5, 10.0], [0.5, 10.0],                               # +- h_0
                     [1.0, 12.0], [1.0, 8.0],                                # +- h_1
                     [1.5, 12.0], [1.5, 8.0], [0.5, 12.0], [0.5, 8.0]])      # (+,+) (+,-) (-,+) (-,-)
    np.testing.assert_array_equal(lo.stencil(u, h)[0], hand)
    assert lo.pairs(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    for k in (1, 2, 5, 12):
        pts = lo.stencil(np.zeros((3, k)), np.ones(k))
        assert pts.shape == (3, 2 * k * k + 1, k)
        assert len({tuple(p) for p in pts[0]}) == 2 * k * k + 1            # all points distinct


def test_formulas_k2_by_hand():
    # f = 3 + 2 x - y - x^2 - 2 y^2 + 0.5 x y  at (0, 0): grad (2, -1), hess [[-2, .5], [.5, -4]]
    f = lambda p: 3 + 2 * p[..., 0] - p[..., 1] - p[..., 0] ** 2 - 2 * p[..., 1] ** 2 + 0.5 * p[..., 0] * p[..., 1]
    h = np.array([0.25, 0.5])
    g, H, bad = lo.grad_hess(f(lo.stencil(np.zeros((1, 2)), h)), h)
    np.testing.assert_allclose(g[0], [2.0, -1.0], atol=1e-14)
    np.testing.assert_allclose(H[0], [[-2.0, 0.5], [0.5, -4.0]], atol=1e-13)
    assert bad[0] == 0 and H[0, 0, 1] == H[0, 1, 0]


@pytest.mark.parametrize("k", [1, 2, 5, 12])
def test_oracle_is_exact_on_quadratics_within_the_rounding_bound(k):
    A, m, c0, starts, logpost = lo.quadratic(k, 7, seed=k)
    h = lap.default_step(starts)
    pts = lo.stencil(starts, h)
    vals = logpost(pts.reshape(-1, k)).reshape(7, -1)
    g, H, bad = lo.grad_hess(vals, h)
    bound = 16 * EPS * np.max(np.abs(vals)) / np.min(h) ** 2
    assert np.all(bad == 0)
    assert np.max(np.abs(H + A)) <= bound, (np.max(np.abs(H + A)), bound)
    g_ref = (A @ (m - starts).T).T
    assert np.max(np.abs(g - g_ref)) <= bound * np.max(h), (np.max(np.abs(g - g_ref)), bound * np.max(h))
    # one undamped step lands on the mode
    delta, logdet, ok = lo.newton_step(g, H, np.zeros(7))
    assert ok.all() and np.max(np.abs(starts + delta - m)) < 1e-5
    np.testing.assert_allclose(logdet, np.linalg.slogdet(A)[1], atol=1e-5)


def test_oracle_flags_bad_values_and_indefinite_curvature():
    k = 2
    h = np.array([0.1, 0.1])
    vals = np.ones((3, 9))
    vals[1, 4] = np.nan
    g, H, bad = lo.grad_hess(vals, h)
    assert list(bad) == [0, 1, 0] and np.all(np.isnan(g[1])) and np.all(np.isnan(H[1])) and np.all(np.isfinite(H[[0, 2]]))
    hess = np.stack([-np.eye(k), np.diag([-1.0, 1.0])])
    delta, logdet, ok = lo.newton_step(np.ones((2, k)), hess, np.zeros(2))
    assert list(ok) == [True, False] and np.all(np.isnan(delta[1])) and np.isnan(logdet[1])
    delta, logdet, ok = lo.newton_step(np.ones((2, k)), hess, np.array([0.0, 2.0]))
    assert ok.all()


# ---- refusals: ValueError before any device work (without a GPU a device call would raise RodeoKalmanError instead) ----
def _quad(u):
    return -0.5 * np.sum(np.asarray(u) ** 2, axis=1)


def test_more_than_twelve_parameters_are_refused():
    with pytest.raises(ValueError, match="k <= 12"):
        lap.laplace(_quad, np.zeros(13))
    with pytest.raises(ValueError, match="k <= 12"):
        lap.laplace(_quad, np.zeros((3, 13)))


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_start_is_refused(bad):
    with pytest.raises(ValueError, match="not finite"):
        lap.laplace(_quad, np.array([0.0, bad, 1.0]))


def test_a_start_where_logpost_is_not_finite_is_refused():
    with pytest.raises(ValueError, match="not finite at upars_init"):
        lap.laplace(lambda u: np.log(u[:, 0]), np.array([[1.0, 2.0], [-1.0, 2.0]]))


def test_a_logpost_that_does_not_return_one_value_per_row_is_refused():
    with pytest.raises(ValueError, match="one value per row"):
        lap.laplace(lambda u: np.zeros(len(u) + 1), np.zeros((4, 3)))
    with pytest.raises(ValueError, match="one value per row"):
        lap.laplace(lambda u: 0.0, np.zeros(3))
    with pytest.raises(ValueError, match="one value per row"):
        lap.laplace(lambda u: np.zeros((len(u), 1)), np.zeros(3))


def test_bad_shapes_steps_and_keys_are_refused():
    with pytest.raises(ValueError, match="shape"):
        lap.laplace(_quad, np.zeros((2, 2, 2)))
    with pytest.raises(ValueError, match="shape"):
        lap.laplace(_quad, np.zeros(0))
    for step in (0.0, -1e-3, np.nan, [1e-3, 0.0]):
        with pytest.raises(ValueError, match="step"):
            lap.laplace(_quad, np.zeros(2), step=step)
    with pytest.raises(ValueError, match="key"):
        lap.laplace(_quad, np.zeros(2), n_samples=10)
