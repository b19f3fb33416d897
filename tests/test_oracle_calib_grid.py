"""
Pins tests/calib_grid_oracle.py (the NumPy restatement of ``solve_evidence_grid`` / ``solve_mv_dynamic_grid`` /
``solve_sim_dynamic_grid``), without a GPU.

(1) Dense conditioning: for x'' = sin 2t - x the model is linear Gaussian once the scales are given, on ANY grid: the chain
    X_{n+1} = Q_n X_n + chol(c_n R_n) e over the nodes of tests/test_oracle_grid.py's four-slot grid, conditioned on Z_n = 0
    (oracle/joint_gaussian.py).  Log-evidence, smoothed mean and smoothed variance, with the scales fixed at 1 (the evidence)
    and at the dynamic estimates; kramer and schober.  Bar: 1e-8 of max(1, |ref|) (measured <= 1.4e-12).
(2) On a ``np.linspace`` grid the restatement is tests/evidence_oracle.py and tests/dynamic_oracle.py, to 1e-12 of the largest
    entry (measured 0.0), and prior_at is called once.
(3) The scale law on the "levels" and "distinct" grids: ``evidence_at(ev, 3)`` is the evidence under 3 R_n (bars of
    tests/test_oracle_evidence.py (b): 1e-10, relative).
(4) Scale invariance of the dynamic solver: 9 R_n leaves the moments where they were and divides every scale by 9 (bars of
    tests/test_oracle_dynamic.py (c)).
(5) With a floor above every estimate the dynamic run is tests/grid_oracle.py's solver under (Q_n, scale_min R_n) and its logdens
    the grid evidence under that prior (bar of tests/test_oracle_dynamic.py (d): 1e-12, relative).
(6) Every case of tests/test_gpu_calib_grid.py is one its bar can judge: the restatement moves by less than the bar when every
    R_n is perturbed by 1e-15, relative.
"""
import numpy as np
import pytest
from scipy.stats import multivariate_normal
from oracle import interrogations as oi, joint_gaussian as jg, odes, priors
from rodeo_amd.evidence import Evidence, evidence_at
from test_gpu_evidence import _bar
from test_oracle_dynamic import _higher, _worst
from test_oracle_grid import GRIDS
import calib_grid_cases as cc
import calib_grid_oracle as cgo
import dynamic_oracle as dyo
import evidence_oracle as evo
import grid_cases as gc
import grid_oracle as go

FOUR = GRIDS["four slots"]
ITG = {"rodeo": oi.interrogate_rodeo, "schober": oi.interrogate_schober, "kramer": oi.interrogate_kramer}


# ---- (1) -----------------------------------------------------------------------------------------------------------------
def _dense(p, name, x0, pairs, scale, mean_pred):
    """Log-density of Z_{1:N} = 0 and the moments of every X_n given Z_{1:N} = 0 under the chain with noise c_n R_n."""
    N = len(pairs)
    ts = FOUR[1:]
    A, Cf, b = np.stack([Q[0] for Q, _ in pairs]), np.zeros((N + 1, p, p)), np.zeros((N + 1, p))
    b[0] = x0[0]
    for n in range(N):
        Cf[n + 1] = np.linalg.cholesky(scale[n] * pairs[n][1][0])
    mu, S = jg.gauss_markov_mv(A, b, Cf)
    nx = (N + 1) * p
    mu, S = mu.reshape(-1), S.reshape(nx, nx)
    G = np.zeros((N, nx))
    for n in range(1, N + 1):
        G[n - 1, n * p + 2] = 1.0
        if name == "kramer":                            # H = W - J = e_2 + e_0, a_n = -sin 2 t_n whatever the linearisation point
            G[n - 1, n * p] = 1.0
    a = -np.sin(2 * ts) if name == "kramer" else -(np.sin(2 * ts) - mean_pred[1:, 0])   # schober: a_n = -f(mu-_n)
    ld = multivariate_normal.logpdf(np.zeros(N), G @ mu + a, G @ S @ G.T, allow_singular=False)
    jm = np.concatenate([mu, G @ mu + a])
    jS = np.block([[S, S @ G.T], [G @ S, G @ S @ G.T]])
    _, bc, V = jg.mvncond(jm, jS, np.r_[np.zeros(nx, bool), np.ones(N, bool)])
    V = V.reshape(N + 1, p, N + 1, p)
    return ld, bc.reshape(N + 1, p), np.stack([V[n, :, n, :] for n in range(N + 1)])


@pytest.mark.parametrize("name", ["kramer", "schober"])
@pytest.mark.parametrize("p", [3, 4])
def test_restatement_equals_dense_conditioning_on_the_four_slot_grid(p, name):
    W, x0, _ = _higher(p, 1, 1.0)
    at = lambda h: priors.ibm_init(h, p, np.array([0.5]))
    N = len(FOUR) - 1
    # scales fixed at 1: the evidence (and the grid solver's smoothed moments, which share its filter)
    ld, quad, logdet = cgo.evidence(odes.higher_order, W, x0, FOUR, ITG[name], at)
    (mp, _, _, _), pairs, _ = go.grid_filter(None, odes.higher_order, W, x0, FOUR, ITG[name], at)
    ms, vs = go.solve_mv_grid(None, odes.higher_order, W, x0, FOUR, ITG[name], at)
    ref_ld, sm, sV = _dense(p, name, x0, pairs, np.ones(N), mp[0, :, 0])
    errs = {"evidence logdens": _worst(ld, ref_ld), "mean at c = 1": _worst(ms[:, 0], sm), "var at c = 1": _worst(vs[:, 0], sV)}
    assert abs(ld - (-0.5 * (quad.sum() + logdet.sum()) - N * evo.LOG_2PI / 2)) <= 1e-12 * abs(ld)
    # scales at the dynamic estimates
    f, pairs = cgo.dynamic_filter(odes.higher_order, W, x0, FOUR, ITG[name], at)
    md, vd, scale, ldd = cgo.solve_mv_dynamic_grid(odes.higher_order, W, x0, FOUR, ITG[name], at)
    assert scale.shape == (N, 1) and np.all(np.isfinite(scale)) and np.all(scale > 0)
    ref_ld, sm, sV = _dense(p, name, x0, pairs, scale[:, 0], f.mean_pred[0, :, 0])
    errs.update({"dynamic logdens": _worst(ldd, ref_ld), "dynamic mean": _worst(md[:, 0], sm), "dynamic var": _worst(vd[:, 0], sV)})
    print(f"{name} p = {p}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f"; scales {scale.min():.2e} .. {scale.max():.2e}")
    assert max(errs.values()) <= 1e-8, errs


# ---- (2) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,itg", [(3, "kramer"), (3, "rodeo"), (4, "kramer"), (5, "rodeo")])
def test_uniform_grid_is_the_uniform_restatement(p, itg):
    N, t_max = 40, 1.0
    c = gc.fhn(p, itg, "uniform", N=N, t_max=t_max, B=3)
    calls = []

    def prior_at(h):
        calls.append(h)
        return priors.ibm_init(h, p, gc.SIGMA)
    fn = gc.ITG[itg][1]
    args = (c["oracle_ode"], c["W"], c["x0"])
    ev = cgo.evidence(*args, c["t"], fn, prior_at, **c["params"])
    assert len(calls) == 1
    prior = priors.ibm_init(calls[0], p, gc.SIGMA)
    worst = cc.evidence_worst(ev, evo.evidence(*args, 0.0, t_max, N, fn, prior, **c["params"]))
    calls.clear()
    got = cgo.solve_mv_dynamic_grid(*args, c["t"], fn, prior_at, **c["params"])
    assert len(calls) == 1
    d_mv = cc.dynamic_diffs(got, dyo.solve_mv_dynamic(*args, 0.0, t_max, N, fn, prior, **c["params"]))
    calls.clear()
    x, s, ld = cgo.solve_sim_dynamic_grid(5, *args, c["t"], fn, prior_at, **c["params"])
    xo, so, ldo = dyo.solve_sim_dynamic(5, *args, 0.0, t_max, N, fn, prior, **c["params"])
    assert len(calls) == 1 and x.shape == xo.shape == (3, N + 1, 2, p)
    dx = float(np.max(np.abs(x - xo)) / np.max(np.abs(xo)))
    print(f"uniform {itg} p = {p}: evidence {worst:.1e}, dynamic mean/var/sqrt(scale)/logdens {d_mv}, path {dx:.1e}")
    assert worst <= 1e-12 and max(d_mv) <= 1e-12 and dx <= 1e-12
    np.testing.assert_array_equal(s, so)
    np.testing.assert_array_equal(x[:, 0], c["x0"])


# ---- (3) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["levels", "distinct"])
@pytest.mark.parametrize("p,itg", [(2, "kramer"), (3, "kramer"), (3, "rodeo"), (3, "schober"), (4, "rodeo"), (5, "kramer"), (6, "rodeo")])
def test_scale_law_on_the_grid(p, itg, kind):
    c = gc.fhn(p, itg, kind, t_max=2.0 if itg == "schober" else gc.T_MAX[p])
    N = len(c["t"]) - 1
    one = Evidence(*cc.restate_evidence(c), N)
    two = Evidence(*cc.restate_evidence(c, 3.0), N)
    rel = lambda got, want: float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.abs(want)))
    errs = (rel(two.quad, one.quad / 3.0), rel(two.logdet, one.logdet + N * np.log(3.0)), rel(two.logdens, evidence_at(one, 3.0)))
    print(f"{c['label']}: quad {errs[0]:.2e} logdet {errs[1]:.2e} logdens {errs[2]:.2e}")
    assert np.all(np.isfinite(one.quad)) and max(errs) <= 1e-10, errs
    assert evidence_at(one, 1.0) == pytest.approx(one.logdens, rel=1e-15)


# ---- (4) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["levels", "distinct"])
@pytest.mark.parametrize("p,itg", [(2, "kramer"), (3, "kramer"), (3, "rodeo"), (3, "schober"), (4, "kramer"), (5, "rodeo")])
def test_scale_invariance_on_the_grid(p, itg, kind):
    c = gc.fhn(p, itg, kind, t_max=2.0 if itg == "schober" else gc.T_MAX[p])
    (m1, v1, s1, l1), (m9, v9, s9, l9) = cc.restate_mv(c), cc.restate_mv(c, 9.0)
    assert np.all(np.isfinite(m1)) and np.all(np.isfinite(v1)) and np.all(s1 > 0)
    dm = float(np.max(np.abs(m9 - m1)) / np.max(np.abs(m1)))
    dv = float(np.max(np.abs(v9 - v1)) / np.max(np.abs(v1)))
    ds = float(np.max(np.abs(s9 / s1 * 9.0 - 1.0)))
    dl = abs(l9 - l1) / max(1.0, abs(l1))
    print(f"{c['label']}: mean {dm:.2e} var {dv:.2e} of the largest entry, scale ratio off by {ds:.2e}, logdens {dl:.2e}")
    assert dm <= 1e-9 and dv <= 1e-9 and ds <= 1e-5 and dl <= 1e-9, (dm, dv, ds, dl)


# ---- (5) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["levels", "distinct"])
@pytest.mark.parametrize("itg,floor", [("kramer", 2.0 ** 14), ("schober", 2.0 ** 14), ("rodeo", 2.0 ** 22)])
def test_floor_above_every_estimate_is_the_grid_solver(itg, floor, kind):
    c = gc.fhn(3, itg, kind, t_max=1.0)
    assert cc.restate_mv(c)[2].max() < floor                        # (the floor is above every estimate of the free run)
    m, v, s, ld = cc.restate_mv(c, 1.0, floor)
    assert np.all(s == floor)
    mo, vo = c.restate_mv(floor)
    eld = cc.restate_evidence(c, floor)[0]
    errs = (float(np.max(np.abs(m - mo)) / np.max(np.abs(mo))), float(np.max(np.abs(v - vo)) / np.max(np.abs(vo))), abs(ld - eld) / abs(eld))
    print(f"{c['label']} floor 2^{int(np.log2(floor))}: mean {errs[0]:.2e} var {errs[1]:.2e} logdens {errs[2]:.2e}")
    assert max(errs) <= 1e-12, errs


# ---- (6) the device cases --------------------------------------------------------------------------------------------------
def _label(v):
    return v["label"] if isinstance(v, dict) else str(v)


@pytest.mark.parametrize("c", cc.evidence_cases(), ids=_label)
def test_gpu_evidence_cases_are_well_conditioned(c):
    ref, moved = cc.restate_evidence(c), cc.restate_evidence(c, 1.0 + 1e-15)
    assert all(np.all(np.isfinite(a)) for a in ref)
    worst = cc.evidence_worst(moved, ref)
    print(f"calib-grid-case evidence {c['label']}: restatement moves by {worst:.3e} of max(1, |ref|) under R (1 + 1e-15)")
    assert worst < _bar(c["p"]), (c["label"], worst)


@pytest.mark.parametrize("c", cc.dynamic_cases(), ids=_label)
def test_gpu_dynamic_cases_are_well_conditioned(c):
    ref, moved = cc.restate_mv(c), cc.restate_mv(c, 1.0 + 1e-15)
    assert all(np.all(np.isfinite(a)) for a in ref)
    d = cc.dynamic_diffs(moved, ref)
    print(f"calib-grid-case dynamic {c['label']}: restatement moves by mean {d[0]:.3e} var {d[1]:.3e} sqrt(scale) {d[2]:.3e} "
          f"logdens {d[3]:.3e} under R (1 + 1e-15)")
    assert max(d) < _bar(c["p"]), (c["label"], d)


@pytest.mark.parametrize("c,key", cc.sim_cases(), ids=_label)
def test_gpu_sim_cases_are_well_conditioned(c, key):
    x, x2 = cc.restate_sim(c, key)[0], cc.restate_sim(c, key, 1.0 + 1e-15)[0]
    dx = float(np.max(np.abs(x2 - x)))
    print(f"calib-grid-case sim {c['label']}: restatement's path moves by {dx:.3e} (absolute) under R (1 + 1e-15)")
    assert np.all(np.isfinite(x)) and dx < 1e-7, (c["label"], dx)
