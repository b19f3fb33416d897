"""
Pins tests/dalton_grid_oracle.py (the NumPy restatement of ``dalton_grid`` / ``dalton.solve_mv_grid`` / ``dalton.solve_sim_grid``),
without a GPU.

(a) For a LINEAR ODE with the first-order (kramer) interrogation the model is exactly linear Gaussian, so log p(y | z = 0) and the
    moments of p(X | z = 0, y) at every node come from one joint Gaussian: the prior's Markov chain over the nodes, each
    transition over its own step length (``oracle.joint_gaussian``), z_n at nodes 1 .. N and y at the observed nodes.  The linear
    models are tests/test_oracle_dalton_at.py's, the grids tests/test_oracle_grid.py's.  Bar: 1e-8 max(1, |ref|), that of
    tests/test_oracle_dalton.py.
(b) On a uniform grid with observations on nodes the restatement agrees with tests/dalton_oracle.py (the reference's stacked
    measurement) to 1e-8 relative, value and moments: sequential against stacked conditioning.
(c) No observations: the value is 0.0 and the moments are grid_oracle.solve_mv_grid's.
(d) Moving a node, with its observation, changes the value.
(e) The threshold condition of tests/dalton_grid_cases.py holds for every device case.
(f) Every device case's restatement moves by less than its bar under R (1 + 1e-15).
"""
import numpy as np
import pytest
from scipy.stats import multivariate_normal
from oracle import interrogations as oi, joint_gaussian as jg, priors
import dalton_oracle as dal
import dalton_grid_oracle as dgo
import dalton_grid_cases as dc
import grid_cases as gc
import grid_oracle as go
from test_oracle_dalton_at import _problem, SIGMA, OM
from test_oracle_grid import GRIDS

# observations on node 0, node 1, two neighbouring nodes and node N, as far as the grid has them
def _nodes(N):
    return sorted({0, 1, N} | ({N // 2, N // 2 + 1} if N >= 4 else set()))


def _dense_block(p, x0, H, offset, s, nodes, y, sigma):
    """One block: (log p(y | z = 0), mean (K, p), var (K, p, p) of X | z = 0, y) by dense conditioning over the nodes s."""
    K = len(s)
    N = K - 1
    A, Cf, b = np.zeros((K - 1, p, p)), np.zeros((K, p, p)), np.zeros((K, p))
    b[0] = x0
    for k in range(1, K):
        Qk, Rk = priors.ibm_init(s[k] - s[k - 1], p, np.array([sigma]))
        A[k - 1], Cf[k] = Qk[0], np.linalg.cholesky(Rk[0])
    mu, S = jg.gauss_markov_mv(A, b, Cf)
    mu, S = mu.reshape(-1), S.reshape(K * p, K * p)
    M = len(nodes)
    G = np.zeros((N + M, K * p))
    for n in range(1, K):
        G[n - 1, n * p:(n + 1) * p] = H
    for i, k in enumerate(nodes):
        G[N + i, k * p] = 1.0                                        # D = e_0
    noise = np.concatenate([np.zeros(N), np.full(M, OM)])
    mean, cov = G @ mu, G @ S @ G.T + np.diag(noise)
    u = np.concatenate([[offset(t) for t in s[1:]], y])
    value = multivariate_normal.logpdf(u, mean, cov) - multivariate_normal.logpdf(u[:N], mean[:N], cov[:N, :N])
    mu_j = np.concatenate([mu, mean])
    S_j = np.block([[S, S @ G.T], [G @ S, cov]])
    icond = np.concatenate([np.zeros(K * p, bool), np.ones(N + M, bool)])
    Ac, bc, V = jg.mvncond(mu_j, S_j, icond)
    return value, (Ac @ u + bc).reshape(K, p), np.stack([V[i * p:(i + 1) * p, i * p:(i + 1) * p] for i in range(K)])


@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("p", [3, 4])
@pytest.mark.parametrize("d", [1, 2])
def test_restatement_equals_dense_conditioning_for_a_linear_ode(name, p, d):
    t = GRIDS[name]
    nodes = _nodes(len(t) - 1)
    ode, W, x0, model = _problem(p, d)
    # that file's prior scale; ten times it at p = 4, d = 2, where the smallest forecast variance of z is 2.2e-9 on the four-slot
    # grid and 5.9e-8 at N = 3: the restatement then drops or nearly drops (utils.py:60-78) what the dense density keeps
    sigma = np.full(d, SIGMA * (10.0 if (p, d) == (4, 2) else 1.0))
    rng = np.random.default_rng(0)
    y = rng.standard_normal((len(nodes), d, 1)) * 0.3 - 0.5
    D = np.zeros((len(nodes), d, 1, p)); D[..., 0] = 1.0
    Om = np.full((len(nodes), d, 1, 1), OM)
    args = (None, ode, W, x0, t, oi.interrogate_kramer, lambda h: priors.ibm_init(h, p, sigma), y, nodes, D, Om)
    seen = []
    val = dgo.dalton_grid(*args, forecast_vars=seen)
    m, v = dgo.solve_mv_grid(*args)
    smallest = min(float(np.min(w)) for w in seen)
    ref = [_dense_block(p, x0[b], model[b][0], model[b][1], t, nodes, y[:, b, 0], sigma[b]) for b in range(d)]
    rv = sum(r[0] for r in ref)
    print(f"{name}, p = {p}, d = {d}: smallest forecast variance {smallest:.3e}; value {val!r}, dense {rv!r}, |diff| {abs(val - rv):.3e}")
    assert smallest > 1e-7, smallest
    assert abs(val - rv) <= 1e-8 * max(1.0, abs(rv)), (val, rv)
    for b in range(d):
        em = np.max(np.abs(m[:, b] - ref[b][1]) / np.maximum(1.0, np.abs(ref[b][1])))
        ev = np.max(np.abs(v[:, b] - ref[b][2])) / max(1.0, np.max(np.abs(ref[b][2])))
        print(f"    block {b}: |mean - dense| = {em:.3e}, |var - dense| = {ev:.3e}")
        assert em <= 1e-8 and ev <= 1e-8, (em, ev)


@pytest.mark.parametrize("itg", ["kramer", "rodeo", "schober"])
def test_uniform_grid_is_the_dalton_oracle(itg):
    c = dc.make(gc.fhn(3, itg, "uniform", t_max=2.0 if itg == "schober" else 4.0))
    N, t = 40, c["t"]
    fn = gc.ITG[itg][1]
    prior = priors.ibm_init(t[1] - t[0], 3, c["sigma"])
    times = t[list(c["nodes"])]
    args = (c["oracle_ode"], c["W"], c["x0"], 0.0, t[-1], N, fn, prior, c["y"], times, c["D"], c["Om"])
    val, ref = c.restate_value(), dal.dalton(*args, **c["params"])
    print(f"{itg}: restatement {val!r}, dalton oracle {ref!r}, relative {abs(val - ref) / max(1.0, abs(ref)):.3e}")
    assert abs(val - ref) <= 1e-8 * max(1.0, abs(ref))
    (m, v), (mo, vo) = c.restate_mv(), dal.solve_mv(*args, **c["params"])
    assert np.max(np.abs(m - mo) / np.maximum(1.0, np.abs(mo))) <= 1e-8 and np.max(np.abs(v - vo)) <= 1e-8 * max(1.0, np.max(np.abs(vo)))
    x, xo = c.restate_sim(5), dal.solve_sim(*args, seed=5, **c["params"])
    assert np.max(np.abs(x - xo) / np.maximum(1.0, np.abs(xo))) <= 1e-8


def test_without_observations_the_value_is_zero_and_the_moments_are_the_grid_solver_s():
    c = dc.make(gc.fhn(3, "kramer", "distinct", B=3), ())
    assert np.all(c.restate_value() == 0.0)
    m, v = c.restate_mv()
    mo, vo = go.solve_mv_grid(None, c["oracle_ode"], c["W"], c["x0"], c["t"], oi.interrogate_kramer, c.prior_at(priors.ibm_init),
                              **c["params"])
    assert np.max(np.abs(m - mo)) <= 1e-12 * np.max(np.abs(mo)) and np.max(np.abs(v - vo)) <= 1e-12 * np.max(np.abs(vo))


def test_moving_an_observed_node_changes_the_value():
    c = dc.make(gc.fhn(3, "kramer", "uniform"))
    t = c["t"].copy()
    t[7] += (t[8] - t[7]) / 3
    moved = dc.DCase(c)
    moved["t"] = t
    a, b = c.restate_value(), moved.restate_value()
    print(f"node 7 moved by a third of a step: {a!r} -> {b!r}")
    assert abs(a - b) > 1e-3


# ---- (e), (f): the device cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", dc.all_cases(), ids=lambda c: c["label"])
def test_no_forecast_variance_near_the_threshold(c):
    seen = []
    val = c.restate_value(forecast_vars=seen)
    s = np.concatenate([np.ravel(w) for w in seen])
    inside = int(np.sum((s > 1e-9) & (s < 1e-7)))
    print(f"{c['label']}: forecast variances {s.min():.3e} .. {s.max():.3e}, {inside} inside (1e-9, 1e-7), {int(np.sum(s <= 1e-9))} dropped "
          f"of {s.size}")
    assert np.all(np.isfinite(val)) and inside == 0


@pytest.mark.parametrize("c", dc.mv_cases() + [c for c, _ in dc.sim_cases()], ids=lambda c: c["label"])
def test_gpu_mv_cases_are_well_conditioned(c):
    _, move_m, move_v = dc.mv_moves(c)
    bar_m, bar_v = gc.mv_bars(c)
    print(f"{c['label']}: the restatement moves by {move_m:.3e} (mean, bar {bar_m:.0e}) and {move_v:.3e} of max|var| (bar {bar_v:.0e})")
    assert move_m < bar_m and move_v < bar_v


@pytest.mark.parametrize("c,key", dc.sim_cases(), ids=lambda v: v["label"] if isinstance(v, dict) else str(v))
def test_gpu_sim_cases_are_well_conditioned(c, key):
    a, b = c.restate_sim(key), c.restate_sim(key, 1.0 + 1e-15)
    move, bar = float(np.max(np.abs(a - b)) / np.max(np.abs(a))), gc.sim_bar(c["p"])
    print(f"{c['label']} key={key}: the restated path moves by {move:.3e} of max|x| (bar {bar:.0e})")
    assert move < bar


@pytest.mark.parametrize("c", dc.value_cases(), ids=lambda c: c["label"])
def test_gpu_value_cases_are_well_conditioned(c):
    a, b = np.asarray(c.restate_value()), np.asarray(c.restate_value(1.0 + 1e-15))
    move = float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(a))))
    print(f"{c['label']}: the restated value moves by {move:.3e} relative (bar 1e-7)")
    assert move < 1e-7
