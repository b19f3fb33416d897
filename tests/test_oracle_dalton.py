"""
Pins tests/dalton_oracle.py (the NumPy restatement of DALTON, src/rodeo/inference/dalton.py:39-545): for the LINEAR ODE
x'' = sin 2t - x with the first-order (kramer) interrogation the solver's model is exactly linear Gaussian, so DALTON's value
is the exact log p(y | z_{1:N} = 0) and its solve_mv the exact posterior moments, both computed by dense conditioning
(tests/test_oracle_fenrir.py).  On this model DALTON also equals Fenrir.
"""
import numpy as np
from scipy.stats import multivariate_normal
from oracle import fenrir as ofen, odes, priors, interrogations as oi
import dalton_oracle as dal
from test_oracle_fenrir import _exact_loglik, _exact_posterior

N, T_MIN, T_MAX, P = 10, 0.0, 1.0, 3
W = np.array([[[0.0, 0.0, 1.0]]])
X0 = np.array([[-1.0, 0.0, 1.0]])
D = np.array([1.0, 0.0, 0.0])
OM = 0.05
FORCING = {"a": np.array([-1.0, 0.0, 0.0]), "f": lambda t: np.sin(2 * t)}


def _setup(obs_times):
    Q, R = priors.ibm_init((T_MAX - T_MIN) / N, P, np.array([0.5]))
    n = len(obs_times)
    y = np.random.default_rng(0).standard_normal((n, 1, 1)) * 0.3 - 0.5
    return (Q, R), y, np.tile(D[None, None, None, :], (n, 1, 1, 1)), np.full((n, 1, 1, 1), OM)


def test_dalton_equals_exact_gaussian_loglik_with_an_observation_at_t0():
    obs_times = np.array([0.0, 0.2, 0.5, 1.0])
    (Q, R), y, ow, ov = _setup(obs_times)
    val = dal.dalton(odes.higher_order, W, X0, T_MIN, T_MAX, N, oi.interrogate_kramer, (Q, R), y, obs_times, ow, ov)
    ind = np.searchsorted(np.linspace(T_MIN, T_MAX, N + 1), obs_times)
    ref = multivariate_normal.logpdf(y[0, 0, 0], D @ X0[0], OM) + \
        _exact_loglik(W[0, 0], X0[0], Q[0], R[0], N, T_MIN, T_MAX, FORCING, ind[1:], D, OM, y[1:, 0, 0])
    assert abs(val - ref) < 1e-8 * max(1.0, abs(ref)), (val, ref)


def test_dalton_equals_fenrir_on_the_linear_model():
    obs_times = np.array([0.2, 0.5, 1.0])
    (Q, R), y, ow, ov = _setup(obs_times)
    val = dal.dalton(odes.higher_order, W, X0, T_MIN, T_MAX, N, oi.interrogate_kramer, (Q, R), y, obs_times, ow, ov)
    ref = ofen.fenrir(None, odes.higher_order, W, X0, T_MIN, T_MAX, N, oi.interrogate_kramer, (Q, R), y, obs_times, ow, ov)
    assert abs(val - ref) < 1e-8 * max(1.0, abs(ref)), (val, ref)


def test_dalton_solve_mv_equals_exact_gaussian_posterior():
    obs_times = np.array([0.2, 0.5, 1.0])
    (Q, R), y, ow, ov = _setup(obs_times)
    m, v = dal.solve_mv(odes.higher_order, W, X0, T_MIN, T_MAX, N, oi.interrogate_kramer, (Q, R), y, obs_times, ow, ov)
    assert m.shape == (N + 1, 1, P) and v.shape == (N + 1, 1, P, P)
    ind = np.searchsorted(np.linspace(T_MIN, T_MAX, N + 1), obs_times)
    me, ve = _exact_posterior(W[0, 0], X0[0], Q[0], R[0], N, T_MIN, T_MAX, FORCING, ind, D, OM, y[:, 0, 0])
    np.testing.assert_allclose(m[0, 0], X0[0])
    assert np.all(v[0] == 0)
    assert np.max(np.abs(m[1:, 0] - me)) < 1e-8 and np.max(np.abs(v[1:, 0] - ve)) < 1e-8


def test_dalton_solve_sim_starts_at_x0_and_follows_the_seed():
    obs_times = np.array([0.2, 0.5, 1.0])
    (Q, R), y, ow, ov = _setup(obs_times)
    a = dal.solve_sim(odes.higher_order, W, X0, T_MIN, T_MAX, N, oi.interrogate_kramer, (Q, R), y, obs_times, ow, ov, seed=3)
    b = dal.solve_sim(odes.higher_order, W, X0, T_MIN, T_MAX, N, oi.interrogate_kramer, (Q, R), y, obs_times, ow, ov, seed=4)
    assert a.shape == (N + 1, 1, P) and np.all(a[0] == X0)
    assert np.all(np.isfinite(a)) and np.max(np.abs(a[1:] - b[1:])) > 0
