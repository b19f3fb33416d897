"""
``daltonng_grid`` / ``solve_mv_nn_grid`` (``rodeo_amd.inference.dalton``) on the device against the NumPy restatement
tests/daltonng_grid_oracle.py, and against ``daltonng`` / ``solve_mv_nn`` where the grid is uniform and the two are the same filter.

Cases: tests/daltonng_grid_cases.py (FitzHugh-Nagumo with Poisson counts at N = 40 on grid_cases' three-level and
40-distinct-step grids, observed on nodes 1, 7, 8, 19, 33, 40; n_bstate 2 .. 4 hold two pair sets in registers, 5 and 6 stage a
shared pair in LDS and a batched sigma goes to per-lane LDS rows; B absent, 1, 3, 33 and 65 in both forms -- with both
filters in a wave 33 is a second wave with one live pair of lanes, in the store form 65 is a second wave with one live lane; N = 1, 2, 3; observations on node 0,
node 1, node N, two neighbours, none; the coupled model; Lorenz63; traced Python right-hand sides).
tests/test_oracle_daltonng_grid.py checks every one of them on the CPU.

Bars: tests/test_gpu_daltonng.py's -- the value within 1e-7 relative of the restatement, mean and variance within 1e-8 of
max(1, max|.|); at n_bstate = 6 mean and variance are held to 20 x the restatement's own move under R (1 + 1e-15) (DESIGN.md
section 2's yardstick).  Every comparison prints its largest difference ("daltonng-grid-check ..." lines).

hiprtc builds (right-hand side, model, n_bstate, interrogation, kind): the ten single cases and n_bstate = 6 need both forward
kinds at eight (n_bstate, interrogation) pairs and the observation kernel at five n_bstate; everything else reuses them except the
coupled model, Lorenz63, the traced right-hand sides, the non-concave and Gaussian models and daltonng's own kinds on the uniform
grid -- about forty builds of half a second to three seconds each.
"""
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401
import grid_cases as gc
import dalton_grid_cases as dc
import daltonng_grid_cases as nc

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


def _pick(c, a):
    """The trajectories the restatement was made for."""
    return a if c["B"] is None else a[c.picked()]


def _check_ll(got, c, label=None):
    ref = np.asarray(_ref(c, "value", c.restate_value))
    got = np.asarray(got)
    assert got.shape == (() if c["B"] is None else (c["B"],))
    rel = nc.value_rel(_pick(c, got), ref)
    print(f"daltonng-grid-check value {label or c['label']}: {rel:.3e} relative (bar {nc.VALUE_BAR:.0e}); value {np.ravel(ref)[0]!r}")
    assert np.all(np.isfinite(got)) and rel <= nc.VALUE_BAR, (c["label"], got, ref)


def _check_mv(got, c, label=None, bars=None):
    mean, var = _ref(c, "mv", c.restate_mv)
    m, v = got
    N, d, p = len(c["t"]) - 1, c["W"].shape[-3], c["p"]
    lead = () if c["B"] is None else (c["B"],)
    assert m.shape == lead + (N + 1, d, p) and v.shape == lead + (N + 1, d, p, p)
    dm, dv = nc.rel(_pick(c, m), mean), nc.rel(_pick(c, v), var)
    bar_m, bar_v = bars or (nc.MOMENT_BAR, nc.MOMENT_BAR)
    print(f"daltonng-grid-check mv {label or c['label']}: mean {dm:.3e} (bar {bar_m:.1e}), var {dv:.3e} (bar {bar_v:.1e})")
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(v))
    assert dm <= bar_m and dv <= bar_v, (c["label"], dm, dv)
    np.testing.assert_array_equal(m[..., 0, :, :], c["x0"])             # node 0 is (ode_init, 0)
    assert np.all(v[..., 0, :, :, :] == 0)


# ---- parity with the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", nc.single_cases(), ids=lambda c: c["label"])
def test_single_trajectory_parity(c):
    val = c.device_call(dmod.daltonng_grid)
    assert isinstance(val, float)
    _check_ll(val, c)
    _check_mv(c.device_call(dmod.solve_mv_nn_grid), c)


def test_n_bstate_6_on_the_perturbation_yardstick():
    """The value at the plain bar; mean and variance within 20 x the restatement's own move under R (1 + 1e-15)."""
    c = nc.yardstick_case()
    _, _, (_, move_m, move_v) = nc.moves(c)
    _check_ll(c.device_call(dmod.daltonng_grid), c)
    _check_mv(c.device_call(dmod.solve_mv_nn_grid), c, bars=(max(nc.MOMENT_BAR, 20.0 * move_m), max(nc.MOMENT_BAR, 20.0 * move_v)))


@pytest.mark.parametrize("c", nc.value_cases(), ids=lambda c: c["label"])
def test_daltonng_grid_parity_batched(c):
    _check_ll(c.device_call(dmod.daltonng_grid), c)


@pytest.mark.parametrize("c", nc.mv_cases(), ids=lambda c: c["label"])
def test_solve_mv_nn_grid_parity_batched(c):
    _check_mv(c.device_call(dmod.solve_mv_nn_grid), c)


@pytest.mark.parametrize("p", [3, 4])
def test_traced_python_right_hand_side(p):
    """The README's plain-Python ode_fun: both kinds of the forward kernel around a user right-hand side."""
    c = nc.make(gc.fhn(p, "kramer", "distinct", B=3))
    _check_ll(c.device_call(dmod.daltonng_grid, ode=_fitz), c, f"traced {c['label']}")
    _check_mv(c.device_call(dmod.solve_mv_nn_grid, ode=_fitz), c, f"traced {c['label']}")


# ---- a uniform grid with observations on nodes is daltonng ---------------------------------------------------------------------
@pytest.mark.parametrize("p,itg", [(2, "rodeo"), (3, "kramer"), (4, "kramer"), (5, "rodeo")])
@pytest.mark.parametrize("B", [3, 33])
def test_uniform_grid_against_daltonng(p, itg, B):
    """``daltonng`` / ``solve_mv_nn``: daltonng_fwd_kernel with one (Q, R), daltonng_gain_kernel, then the same chain and
    observation kernels, or bwd_mv_kernel.  The helpers and operands are the same and FitzHugh-Nagumo does not read the time, so
    equality is asserted (after a 1e-12 bar, whose figures are printed first)."""
    c = nc.make(gc.fhn(p, itg, "uniform", B=B))
    t = c["t"]
    N = len(t) - 1
    obs = (c["y"], t[list(c["nodes"])], nc.poisson_loglik)
    fn = gc.ITG[itg][0]
    prior = ra.ibm_init(t[1] - t[0], p, c["sigma"])
    grid_args = (c["ode"], c["W"], c["x0"], t, fn, lambda h: prior) + obs
    unif_args = (c["ode"], c["W"], c["x0"], t[0], t[-1], N, fn, prior) + obs
    ll, (m, v) = dmod.daltonng_grid(None, *grid_args, **c["params"]), dmod.solve_mv_nn_grid(None, *grid_args, **c["params"])
    llo, (mo, vo) = dmod.daltonng(None, *unif_args, **c["params"]), dmod.solve_mv_nn(None, *unif_args, **c["params"])
    rel = [nc.value_rel(ll, llo), nc.rel(m, mo), nc.rel(v, vo)]
    bits = all(np.array_equal(a, b) for a, b in ((ll, llo), (m, mo), (v, vo)))
    print(f"daltonng-grid-check uniform {itg} p={p} B={B} against daltonng: value {rel[0]:.3e} mean {rel[1]:.3e} var {rel[2]:.3e} "
          f"(bar 1e-12); bits equal: {bits}")
    assert np.all(np.isfinite(llo)) and max(rel) <= 1e-12
    np.testing.assert_array_equal(ll, llo)
    np.testing.assert_array_equal(m, mo)
    np.testing.assert_array_equal(v, vo)


# ---- no observations ------------------------------------------------------------------------------------------------------
def test_without_observations_solve_mv_nn_grid_is_solve_mv_grid():
    """The rule of dalton.solve_mv_grid: rodeo_amd.solve_mv_grid itself, bit for bit (the value without observations is a parity
    case: tests/daltonng_grid_cases.py)."""
    for case in (nc.make(gc.fhn(3, "kramer", "distinct", B=3), ()), nc.make(gc.fhn(5, "rodeo", "levels", B=3), ())):
        assert _kernels(lambda: case.device_call(dmod.solve_mv_nn_grid)) == ["grid_fwd_kernel", "grid_bwd_mv_kernel"]
        m, v = case.device_call(dmod.solve_mv_nn_grid)
        mo, vo = ra.solve_mv_grid(None, *case.device_args(), **case["params"])
        np.testing.assert_array_equal(m, mo)
        np.testing.assert_array_equal(v, vo)


# ---- launch and determinism ----------------------------------------------------------------------------------------------
def test_the_launched_kernels():
    c, c5 = nc.make(gc.fhn(3, "kramer", "distinct", B=3)), nc.make(gc.fhn(5, "rodeo", "levels", B=3))
    for case in (c, c5):
        assert _kernels(lambda: case.device_call(dmod.daltonng_grid)) == [
            "daltonng_grid_fwd_kernel<both>", "daltonng_grid_gain_kernel", "daltonng_chain_kernel", "daltonng_obs_kernel"]
        assert _kernels(lambda: case.device_call(dmod.solve_mv_nn_grid)) == ["daltonng_grid_fwd_kernel<store>", "grid_bwd_mv_kernel"]
    one = nc.make(nc._short(3, "kramer", 1, B=33), nc.SHORT_NODES[1])        # N = 1 launches no gain item
    assert _kernels(lambda: one.device_call(dmod.daltonng_grid)) == [
        "daltonng_grid_fwd_kernel<both>", "daltonng_chain_kernel", "daltonng_obs_kernel"]
    assert _kernels(lambda: c.device_call(dmod.daltonng_grid, ode=_fitz))[0] == "daltonng_grid_fwd_kernel<both>"


@pytest.mark.parametrize("c", [nc.make(gc.fhn(3, "kramer", "distinct", B=33)), nc.make(gc.fhn(5, "rodeo", "levels", B=33)),
                               nc.make(gc.fhn(5, "rodeo", "levels", B=33, batched_sigma=True))], ids=lambda c: c["label"])
def test_two_calls_give_identical_bytes(c):
    assert c.device_call(dmod.daltonng_grid).tobytes() == c.device_call(dmod.daltonng_grid).tobytes()
    for a, b in zip(c.device_call(dmod.solve_mv_nn_grid), c.device_call(dmod.solve_mv_nn_grid)):
        assert a.tobytes() == b.tobytes()


def test_the_plan_keeps_no_output_buffers():
    """tests/test_gpu_daltonng.py's pattern: daltonng_grid leaves the plan's outputs alone and its workspace lives for the call."""
    from rodeo_amd.solve import _plan_cache
    c = nc.make(gc.fhn(3, "kramer", "distinct", N=23, t_max=2.3, B=7), (1, 7, 8, 23))
    a = c.device_call(dmod.daltonng_grid)
    plans = [pl for pl in _plan_cache.values() if pl.N == 23]
    assert plans and all(pl._bufs == {} and pl.mean_state is None and pl.var_state is None for pl in plans)
    assert a.tobytes() == c.device_call(dmod.daltonng_grid).tobytes()
    n_plans = len(_plan_cache)
    m, _ = c.device_call(dmod.solve_mv_nn_grid)                          # the same plan, now with outputs
    assert len(_plan_cache) == n_plans and m.shape == (7, 24, 2, 3)


# ---- the model --------------------------------------------------------------------------------------------------------------
def test_a_non_concave_likelihood_returns_nan_without_a_fault():
    """+x^2 / 2 has H = +1 at every point: known from the formula."""
    c = nc.make(gc.fhn(3, "kramer", "distinct", B=3))
    args = (None, *c.device_args(), c["y"], c["t"][list(c["nodes"])], lambda y, X, i, **kw: 0.5 * np.sum(X[:, 0] ** 2))
    vals = dmod.daltonng_grid(*args, **c["params"])
    assert vals.shape == (3,) and np.all(np.isnan(vals))
    m, _ = dmod.solve_mv_nn_grid(*args, **c["params"])
    assert np.all(np.isnan(m[:, -1])) and np.all(np.isfinite(m[:, 0]))
    assert np.all(np.isfinite(c.device_call(dmod.daltonng_grid)))        # the device still answers


def gauss_loglik(y, X, ind, **params):
    r = y[:, 0] - X[:, 0]
    return np.sum(-0.5 * r * r / dc.OMEGA - 0.5 * np.log(2 * np.pi * dc.OMEGA))


@pytest.mark.parametrize("kind", ["levels", "distinct"])
def test_gaussian_loglik_solve_mv_nn_grid_equals_dalton_solve_mv_grid_on_the_device(kind):
    """A Gaussian log-likelihood is its own second-order expansion: yhat = y, V = Omega."""
    c = dc.make(gc.fhn(3, "kramer", kind, B=3))
    times = c["t"][list(c["nodes"])]
    m, v = dmod.solve_mv_nn_grid(None, *c.device_args(), c["y"], times, gauss_loglik, **c["params"])
    mo, vo = c.device_call(dmod.solve_mv_grid)
    print(f"daltonng-grid-check gaussian {kind}: mean {nc.rel(m, mo):.3e} var {nc.rel(v, vo):.3e} (bar 1e-9)")
    assert nc.rel(m, mo) <= 1e-9 and nc.rel(v, vo) <= 1e-9
