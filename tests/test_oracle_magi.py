"""
Pins tests/magi_oracle.py: MAGI's value is exactly the log-density of the measured components x_{1:N}[:, :, :n_active]
given x_0 under the Gauss-Markov prior X_n = Q X_{n-1} + N(0, R) (the filter only factors that joint density), computed
here from the joint Gaussian built densely, block by block.  The square-root form takes chol(R).
"""
import numpy as np
import pytest
from oracle import priors
import magi_oracle as mo


def _problem(p, d, N, prior, seed):
    rng = np.random.default_rng(seed)
    if prior == "ibm":
        Q, R = priors.ibm_init(2.0, p, 0.5 + rng.random(d))     # (a step of 2: R of p = 5 has condition ~7e5)
    else:
        Q, R = mo.random_prior(rng, d, p)
    # a path drawn from the prior itself, so that every forecast density is moderate
    x = np.zeros((N + 1, d, p))
    x[0] = rng.standard_normal((d, p))
    for n in range(1, N + 1):
        for k in range(d):
            x[n, k] = Q[k] @ x[n - 1, k] + np.linalg.cholesky(R[k]) @ rng.standard_normal(p)
    return x, Q, R


CASES = [(p, na) for p in (2, 3, 5) for na in sorted({1, 2, p}) if na <= p]


@pytest.mark.parametrize("prior", ["ibm", "random"])
@pytest.mark.parametrize("kalman_type", ["standard", "square-root"])
@pytest.mark.parametrize("p,n_active", CASES)
def test_oracle_equals_exact_joint_gaussian(p, n_active, kalman_type, prior):
    x, Q, R = _problem(p, 2, 6, prior, seed=10 * p + n_active)
    exact = mo.exact_logdens(x, n_active, Q, R)
    pars = (Q, R) if kalman_type == "standard" else (Q, np.linalg.cholesky(R))
    got = mo.magi_logdens(x, lambda s: s, n_active, pars, kalman_type)
    assert np.isfinite(exact)
    # the stacked covariance of an IBM prior at p = 5 is conditioned beyond 1e10: the brute-force side itself then carries
    # errors of ~1e-7 (a wrong filter step is off by O(1))
    rel = 1e-6 if (prior == "ibm" and p == 5) else 1e-9
    assert got == pytest.approx(exact, rel=rel, abs=1e-9)


def test_oracle_passes_params_and_refuses_unknown_forms():
    x, Q, R = _problem(3, 1, 4, "random", seed=1)
    seen = {}

    def expand(data, scale):
        seen["scale"] = scale
        return data * scale

    a = mo.magi_logdens(x / 2.0, expand, 2, (Q, R), "standard", scale=2.0)
    assert seen["scale"] == 2.0
    assert a == pytest.approx(mo.exact_logdens(x, 2, Q, R), rel=1e-9)
    with pytest.raises(NotImplementedError):
        mo.magi_logdens(x, lambda s: s, 2, (Q, R), "cholesky")
