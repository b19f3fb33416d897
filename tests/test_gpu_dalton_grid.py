"""
``dalton_grid`` / ``dalton.solve_mv_grid`` / ``dalton.solve_sim_grid`` (``rodeo_amd.inference.dalton``) on the device against the
NumPy restatement tests/dalton_grid_oracle.py, and against ``dalton`` / ``dalton.solve_mv`` / ``dalton.solve_sim`` on the lanes where
the grid is uniform and the two are the same filter.

Cases: tests/dalton_grid_cases.py (FitzHugh-Nagumo at N = 40 on grid_cases' three-level and 40-distinct-step grids with
observations on nodes 1, 7, 8, 19, 33, 40; n_bstate 3 and 4 hold two pair sets in registers, 5 stages a shared pair in LDS and a
batched sigma goes to per-lane LDS rows; B absent, 1, 3, 33 in the log-likelihood form -- a second wave with one live pair of lanes
-- and 65 in the store form -- a second wave with one live lane; N = 1, 2, 3; observations on node 0, node 1, node N, two
neighbours, none; n_bobs 1 .. 3; the lane shapes (2, 1) and (6, 3); kramer / rodeo, schober at t_max = 2; Lorenz63 at 3 and 4;
traced Python right-hand sides).  tests/test_oracle_dalton_grid.py checks every one of them on the CPU: no forecast variance
within ten times of the 1e-8 rule, and the restatement's own move under R (1 + 1e-15) below the bar.

Bars: the value within 1e-7 relative of the restatement (tests/test_gpu_dalton.py's ``_check_ll``), the moments at
tests/test_gpu_solver.py's bars (``grid_cases.mv_bars``), the paths at ``grid_cases.sim_bar``.  Every comparison prints its largest
difference ("dalton-grid-check ..." lines).
"""
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401
import grid_cases as gc
import dalton_grid_cases as dc

pytestmark = pytest.mark.gpu
dmod = sys.modules["rodeo_amd.inference.dalton"]         # (rodeo_amd.inference.dalton, the attribute, is the function)


def _kernels(call):
    """Names of the kernels that `call` launched (the handle's per-launch profile)."""
    dev = ra.default_device()
    dev.profile_enable(True)
    try:
        call()
        return [name for name, _ in dev.profile_last()]
    finally:
        dev.profile_enable(False)


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


_refs = {}


def _ref(c, what, make):
    """A restatement, computed once per (case, kind) and left unchanged."""
    if (id(c), what) not in _refs:
        _refs[(id(c), what)] = make()
    return _refs[(id(c), what)]


def _check_ll(got, c, label=None):
    ref = np.asarray(_ref(c, "value", c.restate_value))
    got = np.asarray(got)
    assert got.shape == ref.shape == (() if c["B"] is None else (c["B"],))
    rel = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
    print(f"dalton-grid-check value {label or c['label']}: {rel:.3e} relative (bar 1e-7); value {np.ravel(ref)[0]!r}")
    assert np.all(np.isfinite(got)) and rel <= 1e-7, (c["label"], got, ref)


def _check_mv(got, c, label=None):
    mean, var = _ref(c, "mv", c.restate_mv)
    m, v = got
    assert m.shape == mean.shape and v.shape == var.shape
    bar_m, bar_v = gc.mv_bars(c)
    dm, dv = float(np.max(np.abs(m - mean))), float(np.max(np.abs(v - var)) / np.max(np.abs(var)))
    print(f"dalton-grid-check mv {label or c['label']}: mean {dm:.3e} (absolute, bar {bar_m:.1e}), var {dv:.3e} of max|var| (bar {bar_v:.1e})")
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(v))
    assert dm <= bar_m and dv <= bar_v, (c["label"], dm, dv)
    np.testing.assert_array_equal(m[..., 0, :, :], c["x0"])             # node 0 is (ode_init, 0)
    assert np.all(v[..., 0, :, :, :] == 0)


# ---- parity with the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", dc.value_cases(), ids=lambda c: c["label"])
def test_dalton_grid_parity(c):
    _check_ll(c.device_call(dmod.dalton_grid), c)


@pytest.mark.parametrize("c", dc.mv_cases(), ids=lambda c: c["label"])
def test_solve_mv_grid_parity(c):
    _check_mv(c.device_call(dmod.solve_mv_grid), c)


@pytest.mark.parametrize("c,key", dc.sim_cases(), ids=lambda v: v["label"] if isinstance(v, dict) else str(v))
def test_solve_sim_grid_parity(c, key):
    """Same Philox stream on both sides; x[0] is ode_init."""
    x = c.device_call(dmod.solve_sim_grid, key)
    ref = _ref(c, ("sim", key), lambda: c.restate_sim(key))
    assert x.shape == ref.shape
    bar = gc.sim_bar(c["p"])
    dx = float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))
    print(f"dalton-grid-check sim {c['label']} key={key}: x {dx:.3e} of max|x| (bar {bar:.0e})")
    assert np.all(np.isfinite(x)) and dx <= bar, (c["label"], dx)
    np.testing.assert_array_equal(x[..., 0, :, :], c["x0"])


@pytest.mark.parametrize("p", [3, 4])
def test_traced_python_right_hand_side(p):
    """The README's plain-Python ode_fun: the hiprtc builds of both forms of the forward kernel."""
    c = dc.make(gc.fhn(p, "kramer", "distinct", B=3))
    _check_ll(c.device_call(dmod.dalton_grid, ode=_fitz), c, f"traced {c['label']}")
    _check_mv(c.device_call(dmod.solve_mv_grid, ode=_fitz), c, f"traced {c['label']}")


# ---- a uniform grid with observations on nodes is dalton on the lanes -------------------------------------------------------
@pytest.mark.parametrize("p,itg,B,n_bobs", [(3, "kramer", 33, 1), (3, "rodeo", None, 2), (4, "kramer", 3, 1), (5, "rodeo", 3, 1),
                                            (2, "rodeo", 3, 1)])
def test_uniform_grid_against_dalton_on_the_lanes(p, itg, B, n_bobs, monkeypatch):
    """``dalton`` / ``dalton.solve_mv`` / ``dalton.solve_sim`` under RK_DALTON_LANES=1: dalton_fwd_kernel with one (Q, R), then
    bwd_mv_kernel / bwd_sim_kernel.  The step is dalton_fwd_kernel's, helper for helper in the same order, and FitzHugh-Nagumo
    does not read the time, so equality is asserted (after a 1e-12 bar, whose figures are printed first)."""
    monkeypatch.setenv("RK_DALTON_LANES", "1")
    c = dc.make(gc.fhn(p, itg, "uniform", B=B), n_bobs=n_bobs)
    t = c["t"]
    N = len(t) - 1
    times = t[list(c["nodes"])]
    obs = (c["y"], times, c["D"], c["Om"])
    args = (c["ode"], c["W"], c["x0"])
    fn = gc.ITG[itg][0]
    prior = ra.ibm_init(t[1] - t[0], p, c["sigma"])
    grid_args = args + (t, fn, c.prior_at()) + obs
    unif_args = args + (t[0], t[-1], N, fn, prior) + obs
    ll, (m, v), x = (dmod.dalton_grid(None, *grid_args, **c["params"]), dmod.solve_mv_grid(None, *grid_args, **c["params"]),
                     dmod.solve_sim_grid(5, *grid_args, **c["params"]))
    assert _kernels(lambda: dmod.solve_mv(None, *unif_args, **c["params"]))[0] == "dalton_fwd_kernel<store>"
    llo, (mo, vo), xo = (dmod.dalton(None, *unif_args, **c["params"]), dmod.solve_mv(None, *unif_args, **c["params"]),
                         dmod.solve_sim(5, *unif_args, **c["params"]))
    rel = [float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1.0, float(np.max(np.abs(b)))))
           for a, b in ((ll, llo), (m, mo), (v, vo), (x, xo))]
    bits = all(np.array_equal(a, b) for a, b in ((ll, llo), (m, mo), (v, vo), (x, xo)))
    print(f"dalton-grid-check uniform {itg} p={p} B={B} n_bobs={n_bobs} against dalton on the lanes: value {rel[0]:.3e} mean {rel[1]:.3e} "
          f"var {rel[2]:.3e} x {rel[3]:.3e} (bar 1e-12); bits equal: {bits}")
    assert max(rel) <= 1e-12
    np.testing.assert_array_equal(ll, llo)
    np.testing.assert_array_equal(m, mo)
    np.testing.assert_array_equal(v, vo)
    np.testing.assert_array_equal(x, xo)


# ---- no observations ------------------------------------------------------------------------------------------------------
def test_without_observations():
    """The value is 0.0 (both halves of a wave run the same filter) and the two solvers are rodeo_amd.solve_mv_grid /
    solve_sim_grid bit for bit."""
    c = dc.make(gc.fhn(3, "kramer", "distinct", B=3), ())
    c5 = dc.make(gc.fhn(5, "rodeo", "levels", B=3), ())
    for case in (c, c5):
        ll = case.device_call(dmod.dalton_grid)
        assert ll.shape == (3,) and np.all(ll == 0.0)
        m, v = case.device_call(dmod.solve_mv_grid)
        mo, vo = ra.solve_mv_grid(None, *case.device_args(), **case["params"])
        np.testing.assert_array_equal(m, mo)
        np.testing.assert_array_equal(v, vo)
        np.testing.assert_array_equal(case.device_call(dmod.solve_sim_grid, 5), ra.solve_sim_grid(5, *case.device_args(), **case["params"]))


# ---- launch and determinism ----------------------------------------------------------------------------------------------
def test_the_launched_kernels():
    c, c5 = dc.make(gc.fhn(3, "kramer", "distinct", B=3)), dc.make(gc.fhn(5, "rodeo", "levels", B=3))
    lz = dc.make(gc.lorenz(3, "rodeo", "distinct", B=5))
    for case in (c, c5, lz):
        assert _kernels(lambda: case.device_call(dmod.dalton_grid)) == ["dalton_grid_fwd_kernel<loglik>"]
        assert _kernels(lambda: case.device_call(dmod.solve_mv_grid)) == ["dalton_grid_fwd_kernel<store>", "grid_bwd_mv_kernel"]
    assert _kernels(lambda: c.device_call(dmod.solve_sim_grid, 1)) == ["dalton_grid_fwd_kernel<store>", "grid_bwd_sim_kernel"]
    assert _kernels(lambda: c.device_call(dmod.dalton_grid, ode=_fitz)) == ["dalton_grid_fwd_kernel<loglik, user>"]
    assert _kernels(lambda: c.device_call(dmod.solve_mv_grid, ode=_fitz)) == ["dalton_grid_fwd_kernel<store, user>", "grid_bwd_mv_kernel"]
    assert _kernels(lambda: c.device_call(dmod.solve_sim_grid, 1, ode=_fitz)) == ["dalton_grid_fwd_kernel<store, user>",
                                                                                   "grid_bwd_sim_kernel"]


@pytest.mark.parametrize("c", [dc.make(gc.fhn(3, "kramer", "distinct", B=33)), dc.make(gc.fhn(5, "rodeo", "levels", B=33)),
                               dc.make(gc.fhn(5, "rodeo", "levels", B=33, batched_sigma=True)),
                               dc.make(gc.lorenz(3, "rodeo", "distinct", B=5))], ids=lambda c: c["label"])
def test_two_calls_give_identical_bytes(c):
    assert c.device_call(dmod.dalton_grid).tobytes() == c.device_call(dmod.dalton_grid).tobytes()
    for a, b in zip(c.device_call(dmod.solve_mv_grid), c.device_call(dmod.solve_mv_grid)):
        assert a.tobytes() == b.tobytes()
    assert c.device_call(dmod.solve_sim_grid, 5).tobytes() == c.device_call(dmod.solve_sim_grid, 5).tobytes()


def test_grid_with_times_puts_the_observation_times_on_nodes():
    """Off-node times through grid_with_times: the value is the restatement's on the grid it returns, and prior_at is called
    once per slot of that grid."""
    c = dc.times_case()
    t, times = c["t"], c["times"]
    assert len(t) == 43 and list(c["nodes"]) == [4, 9, 22]
    calls = []

    def prior_at(h):
        calls.append(h)
        return ra.ibm_init(h, 3, c["sigma"])
    ll = dmod.dalton_grid(None, c["ode"], c["W"], c["x0"], t, gc.ITG["kramer"][0], prior_at, c["y"], times, c["D"], c["Om"], **c["params"])
    assert len(calls) == len(ra.grid_slots(t)[0]) == 4
    _check_ll(ll, c, "grid_with_times")
