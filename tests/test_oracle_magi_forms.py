"""
Pins the guidance of DESIGN.md section 7 item 6 on which MAGI form to trust, on the NumPy restatement of the reference
(tests/magi_oracle.py), which the device reproduces.  With n_active >= 2 and a coupled Q, the reference's standard form
loses the symmetry of its covariance and leaves the true log-density over long series, at n_active = p too.  The
square-root form does not.  With n_active = 1 both forms stay together, also under an IBM prior.
"""
import numpy as np
import pytest
from scipy.stats import multivariate_normal
from oracle import priors
import magi_oracle as mo


def _path(rng, Q, R, N):
    d, p = Q.shape[:2]
    L = np.linalg.cholesky(R)
    x = np.zeros((N + 1, d, p))
    x[0] = rng.standard_normal((d, p))
    for n in range(1, N + 1):
        x[n] = np.einsum("kij,kj->ki", Q, x[n - 1]) + np.einsum("kij,kj->ki", L, rng.standard_normal((d, p)))
    return x


def _coupled(seed=0, d=3, p=4, N=150):
    rng = np.random.default_rng(seed)
    Q = np.stack([0.7 * np.eye(p) + 0.1 * rng.standard_normal((p, p)) for _ in range(d)])
    _, R = mo.stable_prior(rng, d, p)
    return _path(rng, Q, R, N), Q, R


def _closed_form(x, Q, R):
    """n_active = p: every state is measured, so the density is sum_n log N(x_n | Q x_{n-1}, R)."""
    return sum(multivariate_normal.logpdf(x[n, k], Q[k] @ x[n - 1, k], R[k])
               for n in range(1, x.shape[0]) for k in range(x.shape[1]))


def test_square_root_form_is_exact_at_full_measurement_with_a_coupled_q():
    x, Q, R = _coupled()
    got = mo.magi_logdens(x, lambda s: s, 4, (Q, np.linalg.cholesky(R)), "square-root")
    assert got == pytest.approx(_closed_form(x, Q, R), rel=1e-9)


def test_standard_form_leaves_the_true_value_at_full_measurement_with_a_coupled_q():
    # the property of the reference's standard.update that the guidance rests on (not a target of this build)
    x, Q, R = _coupled()
    got = mo.magi_logdens(x, lambda s: s, 4, (Q, R), "standard")
    exact = _closed_form(x, Q, R)
    assert abs(got - exact) > 1e-3 * abs(exact)


def test_one_active_component_keeps_both_forms_together_under_an_ibm_prior():
    rng = np.random.default_rng(1)
    Q, R = priors.ibm_init(0.05, 3, np.array([1.0, 1.0]))
    x = _path(rng, Q, R, 600)
    a = mo.magi_logdens(x, lambda s: s, 1, (Q, R), "standard")
    b = mo.magi_logdens(x, lambda s: s, 1, (Q, np.linalg.cholesky(R)), "square-root")
    assert a == pytest.approx(b, rel=1e-9)
