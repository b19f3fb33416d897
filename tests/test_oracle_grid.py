"""
Pins tests/grid_oracle.py (the NumPy restatement of ``solve_mv_grid`` / ``solve_sim_grid``), without a GPU.

(a) For a LINEAR ODE with the first-order (kramer) interrogation the solver's model is exactly linear Gaussian (as in
    tests/test_oracle_eval_at.py, whose blocks these are), so the posterior on ANY grid is the marginal of one joint Gaussian:
    the prior's Markov chain over the nodes, each transition over its own step length, conditioned on z_n = 0 at the nodes.
    Bar: that file's 1e-8 on the mean and on var / max|var| (the restatement alone gives <= 4.9e-10 and <= 1.8e-9 at p = 4,
    <= 3.4e-11 at p = 3).
(b) On a uniform grid the restatement is oracle/scan.py's solve_mv / solve_sim, and prior_at is called exactly once.
(c) x'' = sin 2t - x: moving one interior node changes the result -- the table's times reach the right-hand side.
(d) Every case of tests/test_gpu_grid.py is one its bar can judge: the restatement moves by less than the bar when R is
    perturbed by 1e-15, relative.  The exceptions are named in grid_cases.Case.yardstick.
"""
import numpy as np
import pytest
from oracle import interrogations as oi, joint_gaussian as jg, odes, priors, scan
from rodeo_amd.grid import grid_slots
from test_oracle_eval_at import _problem, RATES
import grid_oracle as go
import grid_cases as gc

GRIDS = {
    "four slots": np.concatenate([[0.0], np.cumsum([.1, .05, .05, .1, .1, .025, .025, .05, .1, .2, .1, .1])]),
    "irregular": np.concatenate([[0.0], np.cumsum(0.1 * 2.0 ** np.random.default_rng(3).uniform(-1.5, 1.5, 12))]),
    "N=1": np.array([0.0, 0.13]), "N=2": np.array([0.0, 0.1, 0.17]), "N=3": np.array([0.0, 0.1, 0.15, 0.3]),
}


def _dense_posterior(p, rate, x0, sigma, s):
    """One block of test_oracle_eval_at._dense_posterior without queries and on the nodes s: the chain X(s_0) .. X(s_N),
    conditioned on z_n = (W - rate e_0^T) X(s_n) = 0 for n = 1 .. N.  Returns mean (N+1, p) and var (N+1, p, p)."""
    K = len(s)
    N = K - 1
    A, Cf, b = np.zeros((K - 1, p, p)), np.zeros((K, p, p)), np.zeros((K, p))
    b[0] = x0
    for k in range(1, K):
        Qk, Rk = priors.ibm_init(s[k] - s[k - 1], p, np.array([sigma]))
        A[k - 1], Cf[k] = Qk[0], np.linalg.cholesky(Rk[0])
    mu, S = jg.gauss_markov_mv(A, b, Cf)
    mu, S = mu.reshape(-1), S.reshape(K * p, K * p)
    H = np.zeros(p)
    H[1], H[0] = 1.0, -rate
    Hz = np.zeros((N, K * p))
    for n in range(1, K):
        Hz[n - 1, n * p:(n + 1) * p] = H
    mu_j = np.concatenate([mu, Hz @ mu])
    S_j = np.block([[S, S @ Hz.T], [Hz @ S, Hz @ S @ Hz.T]])
    icond = np.concatenate([np.zeros(K * p, bool), np.ones(N, bool)])
    Ac, bc, V = jg.mvncond(mu_j, S_j, icond)
    return (Ac @ np.zeros(N) + bc).reshape(K, p), np.stack([V[i * p:(i + 1) * p, i * p:(i + 1) * p] for i in range(K)])


def test_the_four_slot_grid_has_four_slots():
    h_rep, slot = grid_slots(GRIDS["four slots"])
    assert len(h_rep) == 4 and list(slot) == [0, 1, 1, 0, 0, 2, 2, 1, 0, 3, 0, 0]
    assert len(grid_slots(GRIDS["irregular"])[0]) == 12


@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("p", [3, 4])
@pytest.mark.parametrize("d", [1, 2])
def test_restatement_equals_dense_conditioning_for_a_linear_ode(name, p, d):
    t = GRIDS[name]
    ode, W, x0, sigma = _problem(p, d)
    m, v = go.solve_mv_grid(None, ode, W, x0, t, oi.interrogate_kramer, lambda h: priors.ibm_init(h, p, sigma))
    assert m.shape == (len(t), d, p) and v.shape == (len(t), d, p, p)
    for blk in range(d):
        me, ve = _dense_posterior(p, RATES[blk], x0[blk], sigma[blk], t)
        em = np.max(np.abs(m[:, blk] - me))
        ev = np.max(np.abs(v[:, blk] - ve)) / np.max(np.abs(ve))
        print(f"{name}, p = {p}, d = {d}, block {blk}: |mean - dense| = {em:.3e}, |var - dense| / max|var| = {ev:.3e}")
        assert em <= 1e-8 and ev <= 1e-8, (em, ev)


@pytest.mark.parametrize("t_max,n", [(4.0, 73), (40.0, 801)])
def test_linspace_grids_are_one_slot(t_max, n):
    h_rep, slot = grid_slots(np.linspace(0.0, t_max, n))
    assert len(h_rep) == 1 and not slot.any()


@pytest.mark.parametrize("itg", ["kramer", "rodeo", "chkrebtii"])
def test_uniform_grid_is_the_solver(itg):
    N, t_max, p = 40, 4.0, 3
    c = gc.fhn(p, itg, "uniform", N=N, t_max=t_max, B=3, key=11 if itg == "chkrebtii" else None)
    calls = []

    def prior_at(h):
        calls.append(h)
        return priors.ibm_init(h, p, gc.SIGMA)
    fn = gc.ITG[itg][1]
    args = (c["oracle_ode"], c["W"], c["x0"])
    m, v = go.solve_mv_grid(c["key"], *args, c["t"], fn, prior_at, **c["params"])
    assert len(calls) == 1
    prior = priors.ibm_init(calls[0], p, gc.SIGMA)
    mo, vo = scan.solve_mv(c["key"], *args, 0.0, t_max, N, fn, prior, **c["params"])
    assert m.shape == mo.shape == (3, N + 1, 2, p)
    assert np.max(np.abs(m - mo)) <= 1e-12 * np.max(np.abs(mo)) and np.max(np.abs(v - vo)) <= 1e-12 * np.max(np.abs(vo))
    calls.clear()
    x = go.solve_sim_grid(5, *args, c["t"], fn, prior_at, **c["params"])
    xo = scan.solve_sim(5, *args, 0.0, t_max, N, fn, prior, **c["params"])
    assert len(calls) == 1 and x.shape == xo.shape == (3, N + 1, 2, p)
    assert np.max(np.abs(x - xo)) <= 1e-12 * np.max(np.abs(xo))
    np.testing.assert_array_equal(x[:, 0], c["x0"])


def test_the_table_s_times_reach_the_right_hand_side():
    """Node 7 of a uniform grid moved by a third of a step: were the right-hand side still evaluated at step_time(n), only the
    two step lengths would change.  Compared with a run that takes the moved node's PRIORS but the uniform grid's TIMES."""
    c = gc.higher(3, "kramer", "uniform", N=12, t_max=1.2)
    t = c["t"].copy()
    t[7] += 0.1 / 3
    at = c.prior_at(priors.ibm_init)
    args = (None, c["oracle_ode"], c["W"], c["x0"])
    moved = go.solve_mv_grid(*args, t, oi.interrogate_kramer, at)[0]
    plain = go.solve_mv_grid(*args, c["t"], oi.interrogate_kramer, at)[0]
    assert np.max(np.abs(moved - plain)) > 1e-4

    step = iter(range(1, 13))

    def uniform_times(key, ode_fun, ode_weight, t, **kw):            # call n interrogates at the uniform grid's node n + 1
        return oi.interrogate_kramer(key=key, ode_fun=ode_fun, ode_weight=ode_weight, t=c["t"][next(step)], **kw)
    stale = go.solve_mv_grid(*args, t, uniform_times, at)[0]
    print(f"node 7 moved: |moved - uniform| = {np.max(np.abs(moved - plain)):.3e}, |moved - stale times| = "
          f"{np.max(np.abs(moved - stale)):.3e}")
    assert np.max(np.abs(moved - stale)) > 1e-4


# ---- (d) the device cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", gc.mv_cases(), ids=lambda c: c["label"])
def test_gpu_mv_cases_are_well_conditioned(c):
    """Below the plain bars, except the named cases that lean on the perturbation yardstick (``Case.yardstick``: n_bstate 6),
    which must be finite and are held to 20 x their own move on the device."""
    h = np.diff(c["t"])
    assert h.max() / h.min() <= 8.0
    (m, v), dm, dv = gc.mv_moves(c)
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(v))
    print(f"grid-case {c['label']}: restatement moves by mean {dm:.3e} (absolute), var {dv:.3e} of max|var| under R (1 + 1e-15)"
          f"{' [yardstick]' if c.yardstick else ''}")
    if not c.yardstick:
        assert dm < gc.mv_bars(c)[0] and dv < gc.mv_bars(c)[1], (c["label"], dm, dv)


@pytest.mark.parametrize("c,key", gc.sim_cases(), ids=lambda v: v["label"] if isinstance(v, dict) else str(v))
def test_gpu_sim_cases_are_well_conditioned(c, key):
    x, x2 = c.restate_sim(key), c.restate_sim(key, 1.0 + 1e-15)
    dx = float(np.max(np.abs(x2 - x)) / np.max(np.abs(x)))
    print(f"grid-case sim {c['label']}: restatement moves by {dx:.3e} of max|x| under R (1 + 1e-15)")
    assert np.all(np.isfinite(x)) and dx < gc.sim_bar(c["p"]), (c["label"], dx)
