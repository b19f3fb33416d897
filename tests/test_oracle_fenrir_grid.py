"""
Pins tests/fenrir_grid_oracle.py (the NumPy restatement of ``fenrir_grid`` / ``fenrir.solve_mv_grid``), without a GPU.

(a) For a LINEAR ODE with the first-order (kramer) interrogation the model is exactly linear Gaussian, so log p(y | z = 0) and the
    moments of p(X | z = 0, y) at every node come from one joint Gaussian: tests/test_oracle_dalton_grid.py's dense conditioning,
    linear models, grids and helpers (Fenrir and DALTON approximate the same quantities and are exact here).  Observations on
    node 0, node 1, two neighbours and node N; N = 1, 2, 3 among the grids.  Bar: 1e-8 max(1, |ref|).
(b) On a uniform grid the restatement equals oracle.fenrir (value and moments) to 1e-12.
(c) No observations: the value is 0.0 and the moments are grid_oracle.solve_mv_grid's to 1e-8 -- the same posterior reached by
    another recursion.
(d) Moving an observed node changes the value.
(e) For every device case no y forecast variance lies in (1e-9, 1e-7).
(f) For every device case the restatement's move under R (1 + 1e-15) is at most a tenth of the case's bar.
"""
import numpy as np
import pytest
from oracle import fenrir as of, interrogations as oi, priors
import fenrir_grid_oracle as fgo
import fenrir_grid_cases as fc
import grid_cases as gc
import grid_oracle as go
import test_oracle_dalton_grid as todg
from test_oracle_dalton_at import _problem, SIGMA, OM
from test_oracle_grid import GRIDS


@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("p", [3, 4])
@pytest.mark.parametrize("d", [1, 2])
def test_restatement_equals_dense_conditioning_for_a_linear_ode(name, p, d):
    t = GRIDS[name]
    nodes = todg._nodes(len(t) - 1)
    ode, W, x0, model = _problem(p, d)
    sigma = np.full(d, SIGMA)
    rng = np.random.default_rng(0)
    y = rng.standard_normal((len(nodes), d, 1)) * 0.3 - 0.5
    D = np.zeros((len(nodes), d, 1, p)); D[..., 0] = 1.0
    Om = np.full((len(nodes), d, 1, 1), OM)
    args = (None, ode, W, x0, t, oi.interrogate_kramer, lambda h: priors.ibm_init(h, p, sigma), y, nodes, D, Om)
    seen = []
    val = fgo.fenrir_grid(*args, forecast_vars=seen)
    m, v = fgo.solve_mv_grid(*args)
    smallest = min(float(np.min(w)) for w in seen)
    ref = [todg._dense_block(p, x0[b], model[b][0], model[b][1], t, nodes, y[:, b, 0], sigma[b]) for b in range(d)]
    rv = sum(r[0] for r in ref)
    print(f"{name}, p = {p}, d = {d}: smallest y forecast variance {smallest:.3e}; value {val!r}, dense {rv!r}, |diff| {abs(val - rv):.3e}")
    assert smallest > 1e-7, smallest
    assert abs(val - rv) <= 1e-8 * max(1.0, abs(rv)), (val, rv)
    for b in range(d):
        em = np.max(np.abs(m[:, b] - ref[b][1]) / np.maximum(1.0, np.abs(ref[b][1])))
        ev = np.max(np.abs(v[:, b] - ref[b][2])) / max(1.0, np.max(np.abs(ref[b][2])))
        print(f"    block {b}: |mean - dense| = {em:.3e}, |var - dense| = {ev:.3e}")
        assert em <= 1e-8 and ev <= 1e-8, (em, ev)


@pytest.mark.parametrize("itg,n_bobs", [("rodeo", 1), ("rodeo", 2), ("kramer", 1), ("schober", 1)])
def test_uniform_grid_is_the_fenrir_oracle(itg, n_bobs):
    c = fc.make(gc.fhn(3, itg, "uniform", t_max=2.0 if itg == "schober" else 4.0), n_bobs=n_bobs)
    N, t = 40, c["t"]
    prior = priors.ibm_init(t[1] - t[0], 3, c["sigma"])
    args = (None, c["oracle_ode"], c["W"], c["x0"], 0.0, t[-1], N, gc.ITG[itg][1], prior, c["y"], t[list(c["nodes"])], c["D"], c["Om"])
    val, ref = c.restate_value(), of.fenrir(*args, **c["params"])
    print(f"{itg}, n_bobs = {n_bobs}: restatement {val!r}, fenrir oracle {ref!r}, |diff| {abs(val - ref):.3e}")
    assert abs(val - ref) <= 1e-12 * max(1.0, abs(ref))
    if itg == "rodeo":                                              # (kramer, schober: the sweep is singular, in both)
        (m, v), (mo, vo) = c.restate_mv(), of.solve_mv(*args, **c["params"])
        em, ev = np.max(np.abs(m - mo) / np.maximum(1.0, np.abs(mo))), np.max(np.abs(v - vo)) / np.max(np.abs(vo))
        print(f"    moments: |mean - oracle| = {em:.3e}, |var - oracle| = {ev:.3e} of max|var|")
        assert em <= 1e-12 and ev <= 1e-12


def test_without_observations_the_value_is_zero_and_the_moments_are_the_grid_solver_s():
    c = fc.make(gc.fhn(3, "rodeo", "distinct", B=3), ())
    assert np.all(c.restate_value() == 0.0)
    m, v = c.restate_mv()
    mo, vo = go.solve_mv_grid(None, c["oracle_ode"], c["W"], c["x0"], c["t"], oi.interrogate_rodeo, c.prior_at(priors.ibm_init),
                              **c["params"])
    em, ev = np.max(np.abs(m - mo) / np.maximum(1.0, np.abs(mo))), np.max(np.abs(v - vo)) / np.max(np.abs(vo))
    print(f"no observations: |mean - solve_mv_grid| = {em:.3e}, |var - solve_mv_grid| = {ev:.3e} of max|var|")
    assert em <= 1e-8 and ev <= 1e-8


def test_moving_an_observed_node_changes_the_value():
    c = fc.make(gc.fhn(3, "rodeo", "uniform"))
    t = c["t"].copy()
    t[7] += (t[8] - t[7]) / 3
    moved = fc.FCase(c)
    moved["t"] = t
    a, b = c.restate_value(), moved.restate_value()
    print(f"node 7 moved by a third of a step: {a!r} -> {b!r}")
    assert abs(a - b) > 1e-3


# ---- (e), (f): the device cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fc.value_cases(), ids=lambda c: c["label"])
def test_no_forecast_variance_near_the_threshold(c):
    seen = []
    val = c.restate_value(forecast_vars=seen)
    assert np.all(np.isfinite(val))
    if not c["nodes"]:
        assert not seen
        return
    s = np.concatenate([np.ravel(w) for w in seen])
    inside = int(np.sum((s > 1e-9) & (s < 1e-7)))
    print(f"{c['label']}: y forecast variances {s.min():.3e} .. {s.max():.3e}, {inside} inside (1e-9, 1e-7) of {s.size}")
    assert inside == 0


@pytest.mark.parametrize("c", fc.value_cases(), ids=lambda c: c["label"])
def test_gpu_value_cases_are_well_conditioned(c):
    a, b = np.asarray(fc.value_ref(c)), np.asarray(c.restate_value(1.0 + 1e-15))
    move = float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(a))))
    print(f"{c['label']}: the restated value moves by {move:.3e} relative (a tenth of the bar: {fc.VALUE_BAR / 10:.0e})")
    assert move <= fc.VALUE_BAR / 10


@pytest.mark.parametrize("c", fc.mv_cases(), ids=lambda c: c["label"])
def test_gpu_mv_cases_are_well_conditioned(c):
    (m, v), (m2, v2) = fc.mv_ref(c), c.restate_mv(1.0 + 1e-15)
    move_m = float(np.max(np.abs(m2 - m)) / max(1.0, np.max(np.abs(m))))
    move_v = float(np.max(np.abs(v2 - v)) / np.max(np.abs(v)))
    print(f"{c['label']}: the restatement moves by {move_m:.3e} (mean, a tenth of the bar: {fc.MEAN_BAR / 10:.0e}) and {move_v:.3e} of "
          f"max|var| (a tenth of the bar: {fc.VAR_BAR / 10:.0e})")
    assert move_m <= fc.MEAN_BAR / 10 and move_v <= fc.VAR_BAR / 10
