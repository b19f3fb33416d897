"""
Pins tests/daltonng_oracle.py (the NumPy restatement of DALTON for non-Gaussian observations,
src/rodeo/inference/dalton.py:550-1039) and records, numerically, where the reference's text cannot be taken literally.
"""
import numpy as np
import pytest
from oracle import odes, priors, interrogations as oi
import dalton_oracle as dal
import daltonng_oracle as ng

THETA = np.array([0.2, 0.2, 3.0])
ITG = {"kramer": oi.interrogate_kramer, "rodeo": oi.interrogate_rodeo, "schober": oi.interrogate_schober}


def _fhn(p, N=40, t_max=2.0, sigma=0.1):
    W = np.zeros((2, 1, p))
    W[:, :, 1] = 1.0
    x = np.array([-1.0, 1.0])
    X = np.zeros((2, p))
    X[:, 0] = x
    X[:, 1] = odes.fitzhugh_nagumo(X, 0.0, theta=THETA)[:, 0]
    return W, X, priors.ibm_init(t_max / N, p, np.array([sigma, sigma]))


def _counts(n, d=2, seed=0):
    return np.random.default_rng(seed).poisson(1.5, size=(n, d, 1)).astype(np.float64)


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1.0, np.max(np.abs(b)))


def test_literal_equals_repaired_where_the_literal_text_is_well_defined():
    """(a) every state component of every block is read and the Hessian is diagonal: weight pattern = identity."""
    p, N, t_max = 2, 30, 1.5
    W, X0, prior = _fhn(p, N, t_max)
    times = np.array([0.3, 0.75, 1.5])
    y = np.random.default_rng(1).standard_normal((3, 2, p)) * 0.3
    fns = ng.gaussian_all([0.05, 0.4])
    args = (odes.fitzhugh_nagumo, W, X0, 0.0, t_max, N, oi.interrogate_rodeo, prior, y, times) + fns
    act = ((0, 1), (0, 1))
    a = ng.daltonng(*args, active=act, theta=THETA)
    b = ng.daltonng(*args, literal=True, theta=THETA)
    assert np.isfinite(a) and abs(a - b) <= 1e-10 * max(1.0, abs(a)), (a, b)
    ma, va = ng.solve_mv_nn(*args, active=act, theta=THETA)
    mb, vb = ng.solve_mv_nn(*args, literal=True, theta=THETA)
    assert _rel(ma, mb) <= 1e-10 and _rel(va, vb) <= 1e-10


def test_literal_text_divides_zero_by_zero_on_the_poisson_example():
    """(b) the reference's own example reads X[:, 0] only: exact zero rows in the stacked innovation variance."""
    W, X0, prior = _fhn(3)
    times = np.array([0.5, 1.0, 2.0])
    args = (odes.fitzhugh_nagumo, W, X0, 0.0, 2.0, 40, oi.interrogate_kramer, prior, _counts(3), times) + ng.poisson()
    try:
        with np.errstate(all="ignore"):
            val = ng.daltonng(*args, literal=True, theta=THETA)
    except np.linalg.LinAlgError:
        return
    assert not np.isfinite(val)
    assert np.isfinite(ng.daltonng(*args, active=((0,), (0,)), theta=THETA))


@pytest.mark.parametrize("itg", ["kramer", "rodeo", "schober"])
def test_gaussian_loglik_solve_mv_nn_equals_dalton_solve_mv(itg):
    """(c) a Gaussian log-likelihood is its own second-order expansion: yhat = y, V = s2."""
    p, N, t_max, s2 = 3, 80, 2.0, 0.05
    W, X0, prior = _fhn(p, N, t_max)
    times = np.array([0.37, 0.9, 1.4, 2.0])
    y = np.random.default_rng(2).standard_normal((4, 2, 1)) * 0.5
    D = np.zeros((4, 2, 1, p))
    D[..., 0] = 1.0
    Om = np.full((4, 2, 1, 1), s2)
    m, v = ng.solve_mv_nn(odes.fitzhugh_nagumo, W, X0, 0.0, t_max, N, ITG[itg], prior, y, times, *ng.gaussian_first(s2),
                          active=((0,), (0,)), theta=THETA)
    mo, vo = dal.solve_mv(odes.fitzhugh_nagumo, W, X0, 0.0, t_max, N, ITG[itg], prior, y, times, D, Om, theta=THETA)
    assert np.max(np.abs(m - mo)) < 1e-8 and np.max(np.abs(v - vo)) < 1e-8


def test_gaussian_loglik_daltonng_equals_dalton_on_the_linear_ode():
    """(c) x'' = sin 2t - x: the Jacobian does not depend on the state, so both filters are exactly linear Gaussian and
    logy_x + logx_z - logx_yhat is Bayes' identity for log p(y | z).  The identity is between DENSITIES: the prior scale is
    chosen so that the non-zero eigenvalues of smooth_sim's conditional variances lie above the 1e-8 threshold of
    utils.py:60-78, below which a direction is dropped from one term and not from another (sigma = 0.5 as in
    test_oracle_dalton.py puts eigenvalues on both sides of it: the two values then differ by 5e-7 relative)."""
    N, t_max, p, s2 = 10, 1.0, 3, 0.05
    W = np.array([[[0.0, 0.0, 1.0]]])
    X0 = np.array([[-1.0, 0.0, 1.0]])
    prior = priors.ibm_init(t_max / N, p, np.array([5.0]))
    times = np.array([0.2, 0.5, 1.0])
    y = np.random.default_rng(0).standard_normal((3, 1, 1)) * 0.3 - 0.5
    D = np.tile(np.array([1.0, 0.0, 0.0])[None, None, None, :], (3, 1, 1, 1))
    val = ng.daltonng(odes.higher_order, W, X0, 0.0, t_max, N, oi.interrogate_kramer, prior, y, times, *ng.gaussian_first(s2),
                      active=((0,),))
    ref = dal.dalton(odes.higher_order, W, X0, 0.0, t_max, N, oi.interrogate_kramer, prior, y, times, D, np.full((3, 1, 1, 1), s2))
    assert abs(val - ref) <= 1e-8 * max(1.0, abs(ref)), (val, ref)


@pytest.mark.parametrize("fns", [ng.poisson(), ng.gaussian_first(0.05), ng.gaussian_all([0.05, 0.4, 0.3]), ng.coupled()],
                         ids=["poisson", "gaussian_first", "gaussian_all", "coupled"])
def test_hand_written_derivatives(fns):
    """(d) complex-step gradients, central second differences of the gradient for the diagonal Hessian blocks."""
    ll, grad, hess = fns
    rng = np.random.default_rng(3)
    X = rng.standard_normal((2, 3)) * 0.5
    y = np.abs(rng.standard_normal((2, 3))).round() + 1.0
    g, H = grad(y, X, 1), hess(y, X, 1)
    for b in range(2):
        for j in range(3):
            Xc = X.astype(complex)
            Xc[b, j] += 1e-30j
            assert abs(np.imag(ll(y, Xc, 1)) / 1e-30 - g[b, j]) <= 1e-12 * max(1.0, abs(g[b, j]))
            h = 1e-5
            Xp, Xm = X.copy(), X.copy()
            Xp[b, j] += h
            Xm[b, j] -= h
            fd = (grad(y, Xp, 1)[b] - grad(y, Xm, 1)[b]) / (2 * h)
            assert np.max(np.abs(fd - H[b, :, j])) <= 1e-8 * max(1.0, np.max(np.abs(H[b])))


def test_an_observation_at_t_min_enters_logy_x_and_not_the_filter():
    """(e)"""
    W, X0, prior = _fhn(3)
    fns = ng.poisson()
    y = _counts(3)
    base = (odes.fitzhugh_nagumo, W, X0, 0.0, 2.0, 40, oi.interrogate_kramer, prior)
    kw = dict(active=((0,), (0,)), theta=THETA)
    with0 = ng.daltonng(*base, y, np.array([0.0, 1.0, 2.0]), *fns, parts=True, **kw)
    without = ng.daltonng(*base, y[1:], np.array([1.0, 2.0]), *fns, parts=True, **kw)
    assert abs(with0[0] - without[0] - fns[0](y[0], X0, 0)) <= 1e-12 * max(1.0, abs(with0[0]))
    assert with0[1] == without[1] and with0[2] == without[2]
    m0 = ng.solve_mv_nn(*base, y, np.array([0.0, 1.0, 2.0]), *fns, **kw)
    m1 = ng.solve_mv_nn(*base, y[1:], np.array([1.0, 2.0]), *fns, **kw)
    assert np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1], m1[1])


def test_a_non_concave_point_gives_nan():
    """H >= 0 by construction: the log-likelihood +x^2 / 2 has H = +1 everywhere."""
    W, X0, prior = _fhn(3)

    def ll(y, X, i, **_):
        return 0.5 * np.sum(X[:, 0] ** 2)

    def grad(y, X, i, **_):
        g = np.zeros_like(X)
        g[:, 0] = X[:, 0]
        return g

    def hess(y, X, i, **_):
        H = np.zeros(X.shape + X.shape[-1:])
        H[:, 0, 0] = 1.0
        return H
    with np.errstate(all="ignore"):
        val = ng.daltonng(odes.fitzhugh_nagumo, W, X0, 0.0, 2.0, 40, oi.interrogate_kramer, prior, _counts(2), np.array([1.0, 2.0]),
                          ll, grad, hess, active=((0,), (0,)), theta=THETA)
    assert np.isnan(val)
