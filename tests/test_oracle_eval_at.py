"""
Pins tests/eval_at_oracle.py (the NumPy restatement of ``solve_mv_at``).  For a LINEAR ODE with the first-order (kramer)
interrogation the solver's model is exactly linear Gaussian (z_n = W X_n - f(X_n) = 0, as in tests/test_oracle_fenrir.py), so
the posterior at ANY time is the marginal of one joint Gaussian: the prior's Markov chain over nodes and queries together
(``oracle.joint_gaussian.gauss_markov_mv``), conditioned on the measurements at the nodes (``mvncond``).  The restatement's
two-step recipe must equal it.
"""
import numpy as np
import pytest
from oracle import interrogations as oi, joint_gaussian as jg, odes, priors, scan
import eval_at_oracle as eo

N, T_MIN, T_MAX = 12, 0.0, 1.2
DT = (T_MAX - T_MIN) / N
RATES = np.array([-1.0, 0.4])
# the first, an interior and the last interval; two queries in one interval; one query 1e-3 dt from a node
QUERIES = np.array([0.37 * DT, 5.5 * DT, 11.81 * DT, 7.2 * DT, 7.9 * DT, (3 + 1e-3) * DT])


def _problem(p, d):
    ode = odes.make_linear_block(np.diag(RATES[:d]))
    W = np.zeros((d, 1, p))
    W[:, 0, 1] = 1.0
    x0 = np.zeros((d, p))
    x0[:, 0] = [1.0, -0.5][:d]
    x0[:, 1] = RATES[:d] * x0[:, 0]
    x0[:, 2] = RATES[:d] ** 2 * x0[:, 0]
    sigma = np.array([0.5, 0.2])[:d]
    return ode, W, x0, sigma


def _dense_posterior(p, rate, x0, sigma, queries):
    """One block: the chain X(s_0) .. X(s_K) over the sorted union of nodes and queries, conditioned on
    z_n = (W - rate e_0^T) X(t_n) = 0 at the nodes n = 1 .. N.  Returns mean (len(queries), p) and var (len(queries), p, p)."""
    nodes = T_MIN + (T_MAX - T_MIN) * np.arange(N + 1) / N
    times = np.concatenate([nodes, queries])
    order = np.argsort(times, kind="stable")
    s = times[order]
    K = len(s)
    A, Cf = np.zeros((K - 1, p, p)), np.zeros((K, p, p))
    b = np.zeros((K, p))
    b[0] = x0
    for k in range(1, K):
        Qk, Rk = priors.ibm_init(s[k] - s[k - 1], p, np.array([sigma]))
        A[k - 1], Cf[k] = Qk[0], np.linalg.cholesky(Rk[0])
    mu, S = jg.gauss_markov_mv(A, b, Cf)
    mu, S = mu.reshape(-1), S.reshape(K * p, K * p)
    H = np.zeros(p)
    H[1], H[0] = 1.0, -rate
    where = np.argsort(order)                                   # position of time i (nodes first, then queries) in the chain
    Hz = np.zeros((N, K * p))
    for n in range(1, N + 1):
        Hz[n - 1, where[n] * p:(where[n] + 1) * p] = H
    mu_j = np.concatenate([mu, Hz @ mu])
    S_j = np.block([[S, S @ Hz.T], [Hz @ S, Hz @ S @ Hz.T]])
    icond = np.concatenate([np.zeros(K * p, bool), np.ones(N, bool)])
    Ac, bc, V = jg.mvncond(mu_j, S_j, icond)
    mean = (Ac @ np.zeros(N) + bc).reshape(K, p)
    idx = where[N + 1:]
    return mean[idx], np.stack([V[i * p:(i + 1) * p, i * p:(i + 1) * p] for i in idx])


@pytest.mark.parametrize("p", [3, 4])
@pytest.mark.parametrize("d", [1, 2])
def test_two_step_recipe_equals_dense_conditioning_for_a_linear_ode(p, d):
    ode, W, x0, sigma = _problem(p, d)
    prior = priors.ibm_init(DT, p, sigma)
    m, v = eo.solve_mv_at(None, ode, W, x0, T_MIN, T_MAX, N, oi.interrogate_kramer, prior, QUERIES,
                          lambda h: priors.ibm_init(h, p, sigma))
    assert m.shape == (len(QUERIES), d, p) and v.shape == (len(QUERIES), d, p, p)
    for blk in range(d):
        me, ve = _dense_posterior(p, RATES[blk], x0[blk], sigma[blk], QUERIES)
        em = np.max(np.abs(m[:, blk] - me))
        ev = np.max(np.abs(v[:, blk] - ve)) / np.max(np.abs(ve))
        print(f"p = {p}, d = {d}, block {blk}: |mean - dense| = {em:.3e}, |var - dense| / max|var| = {ev:.3e}")
        assert em <= 1e-8 and ev <= 1e-8, (em, ev)


def test_queries_on_nodes_return_the_grid_values_exactly():
    ode, W, x0, sigma = _problem(3, 2)
    prior = priors.ibm_init(DT, 3, sigma)
    mo, vo = scan.solve_mv(None, ode, W, x0, T_MIN, T_MAX, N, oi.interrogate_kramer, prior)
    nodes = np.array([N, 0, 5, 5, 9])

    def never(h):
        raise AssertionError("prior_at is not needed when every query is a node")
    t = T_MIN + (T_MAX - T_MIN) * nodes / N
    t[2] += 0.9e-10 * DT                                         # within 1e-10 dt of node 5: that node
    m, v = eo.solve_mv_at(None, ode, W, x0, T_MIN, T_MAX, N, oi.interrogate_kramer, prior, t, never)
    assert np.array_equal(m, mo[nodes]) and np.array_equal(v, vo[nodes])


def test_consistency_check_accepts_the_prior_and_rejects_another_sigma():
    sigma = np.array([0.5, 0.2])
    for p in (3, 4, 5):
        prior = priors.ibm_init(DT, p, sigma)
        for frac in (1e-3, 0.37, 0.5, 1.0 - 1e-3):
            res = eo.check_prior_at(lambda h: priors.ibm_init(h, p, sigma), prior, frac * DT, DT - frac * DT)
            assert max(res) <= 1e-14, res
        with pytest.raises(ValueError, match="inconsistent"):
            eo.check_prior_at(lambda h: priors.ibm_init(h, p, 1.01 * sigma), prior, 0.37 * DT, 0.63 * DT)
    with pytest.raises(ValueError, match="inconsistent"):
        ode, W, x0, sigma = _problem(3, 2)
        eo.solve_mv_at(None, ode, W, x0, T_MIN, T_MAX, N, oi.interrogate_kramer, priors.ibm_init(DT, 3, sigma), QUERIES,
                       lambda h: priors.ibm_init(h, 3, 1.01 * sigma))
