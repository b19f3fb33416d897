"""
``rodeo_amd.solve_evidence_grid`` / ``solve_mv_dynamic_grid`` / ``solve_sim_dynamic_grid`` on the device against the NumPy
restatement tests/calib_grid_oracle.py, against their uniform counterparts bit for bit on a uniform grid, and against the
identities they must keep (scale law, scale invariance, floor limit).

The cases are tests/calib_grid_cases.py's (tests/test_oracle_calib_grid.py (6) checks on the CPU that each is one its bar can
judge).  Bars, all the project's: ``test_gpu_evidence._bar`` (1e-7 for n_bstate <= 4, 1e-5 for 5 and 6) in units of
max(1, |ref|) for logdens, quad, logdet; tests/test_gpu_dynamic.py's for mean, var (of the largest entry), sqrt(scale) (of the
block's largest) and logdens; 1e-7 absolute for sample paths.  Every comparison prints its largest difference
("calib-grid-check ..." lines: profiles/grid_calib_checks.txt keeps them).
"""
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd.evidence import evidence_at
from test_gpu_evidence import _bar, _fitz, _kernels
import calib_grid_cases as cc
import grid_cases as gc

pytestmark = pytest.mark.gpu


def _label(v):
    return v["label"] if isinstance(v, dict) else str(v)


def _evidence(c, ode=None, r_scale=1.0):
    args = list(c.device_args(ode))
    args[-1] = c.prior_at(r_scale=r_scale)
    return ra.solve_evidence_grid(None, *args, **c["params"])


def _dynamic(c, ode=None, r_scale=1.0, **kw):
    args = list(c.device_args(ode))
    args[-1] = c.prior_at(r_scale=r_scale)
    return ra.solve_mv_dynamic_grid(None, *args, **c["params"], **kw)


def _sim(c, key, **kw):
    return ra.solve_sim_dynamic_grid(key, *c.device_args(), **c["params"], **kw)


def _check_evidence(ev, c, label):
    ref = cc.restate_evidence(c)
    for got, want in zip(ev[:3], ref):
        assert np.shape(got) == np.shape(want), (np.shape(got), np.shape(want))
    assert ev.n_steps == len(c["t"]) - 1
    worst, bar = cc.evidence_worst(ev[:3], ref), _bar(c["p"])
    print(f"calib-grid-check evidence {label}: largest difference {worst:.3e} of max(1, |ref|), bar {bar:.0e}")
    assert worst <= bar, (label, worst)


def _check_dynamic(got, c, label):
    ref = cc.restate_mv(c)
    for a, b in zip(got, ref):
        assert np.shape(a) == np.shape(b), (np.shape(a), np.shape(b))
    dm, dv, ds, dl = cc.dynamic_diffs(tuple(got), ref)
    bar = _bar(c["p"])
    print(f"calib-grid-check dynamic {label}: mean {dm:.3e} var {dv:.3e} of the largest entry, sqrt(scale) {ds:.3e} of the block's "
          f"largest, logdens {dl:.3e} of max(1, |ref|), bar {bar:.0e}")
    assert max(dm, dv, ds, dl) <= bar, (label, dm, dv, ds, dl)


# ---- parity with the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cc.evidence_cases(), ids=_label)
def test_evidence_parity(c):
    ev = _evidence(c)
    if c["B"] is None:
        assert isinstance(ev.logdens, float) and ev.quad.shape == ev.logdet.shape == (c["W"].shape[0],)
    _check_evidence(ev, c, c["label"])


@pytest.mark.parametrize("c", cc.dynamic_cases(), ids=_label)
def test_dynamic_parity(c):
    got = _dynamic(c)
    N, (d, _, p) = len(c["t"]) - 1, c["W"].shape
    lead = () if c["B"] is None else (c["B"],)
    assert got.mean.shape == lead + (N + 1, d, p) and got.scale.shape == lead + (N, d) and np.shape(got.logdens) == lead
    _check_dynamic(got, c, c["label"])


@pytest.mark.parametrize("p", [3, 4])
def test_traced_python_right_hand_side(p):
    """The README's plain-Python ode_fun: the hiprtc builds of the two forward kernels."""
    c = gc.fhn(p, "kramer", "distinct", B=3)
    _check_evidence(_evidence(c, ode=_fitz), c, f"traced {c['label']}")
    _check_dynamic(_dynamic(c, ode=_fitz), c, f"traced {c['label']}")


@pytest.mark.parametrize("c,key", cc.sim_cases(), ids=_label)
def test_sim_parity(c, key):
    """Same Philox stream on both sides; x[0] is ode_init; another key changes the path after node 0 and leaves scale alone."""
    got = _sim(c, key)
    x, scale, ld = cc.restate_sim(c, key)
    assert got.x.shape == x.shape and got.scale.shape == scale.shape and got.logdens.shape == ld.shape
    np.testing.assert_array_equal(got.x[:, 0], c["x0"])
    dx = float(np.max(np.abs(got.x - x)))
    ds = float(np.max(np.abs(np.sqrt(got.scale) - np.sqrt(scale)) / np.max(np.sqrt(scale), axis=-2, keepdims=True)))
    dl = float(np.max(np.abs(got.logdens - ld) / np.maximum(1.0, np.abs(ld))))
    print(f"calib-grid-check sim {c['label']}: x {dx:.3e} (absolute, bar 1e-07), sqrt(scale) {ds:.3e}, logdens {dl:.3e} (bar 1e-07)")
    assert dx < 1e-7 and ds <= 1e-7 and dl <= 1e-7
    other = _sim(c, key + 1)
    np.testing.assert_array_equal(other.x[:, 0], c["x0"])
    assert np.all(np.max(np.abs(other.x[:, 1:] - got.x[:, 1:]), axis=(2, 3)) > 0)            # every node after 0, every trajectory
    np.testing.assert_array_equal(other.scale, got.scale)                                    # (the filter draws nothing)


# ---- a uniform t_grid, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,itg,B", [(2, "kramer", 3), (3, "kramer", 65), (3, "rodeo", None), (4, "kramer", 3), (5, "rodeo", 3),
                                     (6, "rodeo", None)])
def test_uniform_grid_evidence_has_solve_evidence_s_bits(p, itg, B, monkeypatch):
    """FitzHugh-Nagumo is autonomous, the pieces and their order are shared: the same bits as the lanes of solve_evidence."""
    monkeypatch.setenv("RK_EVIDENCE_LANES", "1")
    N, t_max = 40, 1.0
    c = gc.fhn(p, itg, "uniform", N=N, t_max=t_max, B=B)
    ev = _evidence(c)
    ref = ra.solve_evidence(None, c["ode"], c["W"], c["x0"], 0.0, t_max, N, gc.ITG[itg][0], c.prior_at()(c["t"][1] - c["t"][0]),
                            **c["params"])
    print(f"calib-grid-check uniform evidence {c['label']}: largest difference {cc.evidence_worst(ev[:3], ref[:3]):.3e}")
    for a, b in zip(ev, ref):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("p,itg,B", [(2, "kramer", 3), (3, "kramer", 65), (3, "rodeo", None), (4, "kramer", 3), (5, "rodeo", 3)])
def test_uniform_grid_dynamic_has_solve_dynamic_s_bits(p, itg, B):
    N, t_max = 40, 1.0
    c = gc.fhn(p, itg, "uniform", N=N, t_max=t_max, B=B)
    prior = c.prior_at()(c["t"][1] - c["t"][0])
    args = (c["ode"], c["W"], c["x0"], 0.0, t_max, N, gc.ITG[itg][0], prior)
    got, ref = _dynamic(c), ra.solve_mv_dynamic(None, *args, **c["params"])
    print(f"calib-grid-check uniform dynamic {c['label']}: mean/var/sqrt(scale)/logdens differ by {cc.dynamic_diffs(tuple(got), tuple(ref))}")
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)
    got, ref = _sim(c, 7), ra.solve_sim_dynamic(7, *args, **c["params"])
    print(f"calib-grid-check uniform sim {c['label']}: x differs by {float(np.max(np.abs(got.x - ref.x))):.3e}")
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)


# ---- identities on the device --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,itg,kind", [(3, "kramer", "distinct"), (4, "rodeo", "levels"), (5, "kramer", "distinct")])
def test_scale_law_on_the_device(p, itg, kind):
    c = gc.fhn(p, itg, kind, B=3)
    one, three = _evidence(c), _evidence(c, r_scale=3.0)
    worst = float(np.max(np.abs(three.logdens - evidence_at(one, 3.0)) / np.maximum(1.0, np.abs(three.logdens))))
    wq = float(np.max(np.abs(three.quad - one.quad / 3.0) / np.maximum(1.0, np.abs(three.quad))))
    print(f"calib-grid-check scale law {c['label']}: evidence_at(ev, 3) off by {worst:.3e}, quad / 3 by {wq:.3e} of max(1, |ref|), "
          f"bar {_bar(p):.0e}")
    assert worst <= _bar(p) and wq <= _bar(p)


@pytest.mark.parametrize("p,itg,kind", [(3, "kramer", "distinct"), (3, "rodeo", "levels"), (4, "kramer", "levels")])
def test_scale_invariance_on_the_device(p, itg, kind):
    c = gc.fhn(p, itg, kind, B=3)
    one, nine = _dynamic(c), _dynamic(c, r_scale=9.0)
    dm = float(np.max(np.abs(nine.mean - one.mean)) / np.max(np.abs(one.mean)))
    dv = float(np.max(np.abs(nine.var - one.var)) / np.max(np.abs(one.var)))
    ds = float(np.max(np.abs(nine.scale / one.scale * 9.0 - 1.0)))
    print(f"calib-grid-check invariance {c['label']}: mean {dm:.3e} var {dv:.3e} of the largest entry (bar 1e-09), scale ratio off by "
          f"{ds:.3e} (bar 1e-05)")
    assert dm <= 1e-9 and dv <= 1e-9 and ds <= 1e-5


@pytest.mark.parametrize("itg,floor", [("kramer", 2.0 ** 14), ("schober", 2.0 ** 14), ("rodeo", 2.0 ** 22)])
def test_floor_limit_against_solve_mv_grid(itg, floor):
    """With a floor above every estimate every scale is the floor and the result is ``solve_mv_grid``'s under
    (Q_n, floor R_n), the logdens ``solve_evidence_grid``'s: the existing solver as the yardstick."""
    c = gc.fhn(3, itg, "distinct", t_max=1.0, B=3)
    got = _dynamic(c, scale_min=floor)
    assert np.all(got.scale == floor)
    args = list(c.device_args())
    args[-1] = c.prior_at(r_scale=floor)
    mean, var = ra.solve_mv_grid(None, *args, **c["params"])
    dm = float(np.max(np.abs(got.mean - mean)) / np.max(np.abs(mean)))
    dv = float(np.max(np.abs(got.var - var)) / np.max(np.abs(var)))
    ev = _evidence(c, r_scale=floor)
    dl = float(np.max(np.abs(got.logdens - ev.logdens) / np.abs(ev.logdens)))
    print(f"calib-grid-check floor 2^{int(np.log2(floor))} {c['label']}: mean {dm:.3e} var {dv:.3e} of the largest entry, logdens "
          f"{dl:.3e}, bar 1e-09")
    assert dm <= 1e-9 and dv <= 1e-9 and dl <= 1e-9


# ---- behaviour -------------------------------------------------------------------------------------------------------------
def test_the_launched_kernels():
    c = gc.fhn(3, "kramer", "distinct", B=3)
    assert _kernels(lambda: _evidence(c)) == ["grid_evidence_kernel"]
    assert _kernels(lambda: _dynamic(c)) == ["grid_dynamic_fwd_kernel", "grid_dynamic_bwd_mv_kernel"]
    assert _kernels(lambda: _sim(c, 1)) == ["grid_dynamic_fwd_kernel", "grid_dynamic_bwd_sim_kernel"]
    assert _kernels(lambda: _evidence(c, ode=_fitz)) == ["grid_evidence_kernel<user>"]
    assert _kernels(lambda: _dynamic(c, ode=_fitz)) == ["grid_dynamic_fwd_kernel<user>", "grid_dynamic_bwd_mv_kernel"]


@pytest.mark.parametrize("c", [gc.fhn(3, "kramer", "levels", B=65, batched_sigma=True), gc.fhn(5, "rodeo", "levels", B=65),
                               gc.lorenz(3, "rodeo", "distinct", B=5)], ids=_label)
def test_two_calls_give_identical_bits(c):
    for call in (lambda: _evidence(c)[:3], lambda: _dynamic(c), lambda: _sim(c, 5)):
        for a, b in zip(call(), call()):
            np.testing.assert_array_equal(a, b)
