"""
``fenrir_grid`` / ``fenrir.solve_mv_grid`` (``rodeo_amd.inference.fenrir``) on the device against the NumPy restatement
tests/fenrir_grid_oracle.py, and against ``fenrir`` / ``fenrir.solve_mv`` where the grid is uniform.

Cases: tests/fenrir_grid_cases.py (FitzHugh-Nagumo at N = 40 on grid_cases' three-level, 40-distinct-step and uniform grids with
observations on nodes 1, 7, 8, 19, 33, 40; n_bstate 2 .. 6 for the value, 2 .. 5 for the moments; B absent, 1, 3 and 65 -- a second
wave with one live lane per block; a batched sigma at 3 and 5; N = 1, 2, 3 with observations on node 0, node 1, node N and two
neighbours; no observations; n_bobs 1 .. 3; Lorenz63 at 3 and 4, whose three blocks go through the ordered sum; kramer, schober
at t_max = 2 and chkrebtii with a key for the value only; traced Python right-hand sides; a ``grid_with_times`` grid of four
slots).  tests/test_oracle_fenrir_grid.py checks every one of them on the CPU: no y forecast variance within ten times of the
1e-8 rule, and the restatement's own move under R (1 + 1e-15) at most a tenth of the bar.

Bars: the value within 1e-7 max(1, |ref|) (tests/test_gpu_inference.py), the mean within 1e-8 max(1, max|ref|) and the variance
within 1e-7 max|ref| (``test_fenrir_solve_mv_parity``).  Every comparison prints its largest difference ("fenrir-grid-check ..."
lines; profiles/fenrir_grid_checks.txt holds those of one run).
"""
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.fenrir  # noqa: F401
import grid_cases as gc
import fenrir_grid_cases as fc

pytestmark = pytest.mark.gpu
fmod = sys.modules["rodeo_amd.inference.fenrir"]         # (rodeo_amd.inference.fenrir, the attribute, is the function)


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


def _value(c, ode=None):
    return c.device_call(fmod.fenrir_grid, c["key"], ode)


def _mv(c, ode=None):
    return c.device_call(fmod.solve_mv_grid, c["key"], ode)


def _value_diff(got, ref):
    return float(np.max(np.abs(np.asarray(got) - ref) / np.maximum(1.0, np.abs(ref))))


def _mv_diff(got, ref):
    (m, v), (mean, var) = got, ref
    return (float(np.max(np.abs(m - mean)) / max(1.0, float(np.max(np.abs(mean))))),
            float(np.max(np.abs(v - var)) / float(np.max(np.abs(var)))))


def _check_value(got, c, label=None):
    ref = fc.value_ref(c)
    got = np.asarray(got)
    assert got.shape == ref.shape == (() if c["B"] is None else (c["B"],))
    rel = _value_diff(got, ref)
    print(f"fenrir-grid-check value {label or c['label']}: {rel:.3e} of max(1, |ref|) (bar {fc.VALUE_BAR:.0e}); value {np.ravel(ref)[0]!r}")
    assert np.all(np.isfinite(got)) and rel <= fc.VALUE_BAR, (c["label"], got, ref)


def _check_mv(got, c, label=None):
    ref = fc.mv_ref(c)
    m, v = got
    assert m.shape == ref[0].shape and v.shape == ref[1].shape
    dm, dv = _mv_diff(got, ref)
    print(f"fenrir-grid-check mv {label or c['label']}: mean {dm:.3e} of max(1, max|mean|) (bar {fc.MEAN_BAR:.0e}), var {dv:.3e} of "
          f"max|var| (bar {fc.VAR_BAR:.0e})")
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(v))
    assert dm <= fc.MEAN_BAR and dv <= fc.VAR_BAR, (c["label"], dm, dv)


# ---- parity with the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fc.value_cases(), ids=lambda c: c["label"])
def test_fenrir_grid_parity(c):
    _check_value(_value(c), c)


@pytest.mark.parametrize("c", fc.mv_cases(), ids=lambda c: c["label"])
def test_solve_mv_grid_parity(c):
    _check_mv(_mv(c), c)


@pytest.mark.parametrize("p", [3, 4])
def test_traced_python_right_hand_side(p):
    """The README's plain-Python ode_fun: the hiprtc build of the grid solver's forward kernel, then the same backward kernels."""
    c = fc.make(gc.fhn(p, "rodeo", "distinct", B=3))
    _check_value(_value(c, _fitz), c, f"traced {c['label']}")
    _check_mv(_mv(c, _fitz), c, f"traced {c['label']}")


# ---- no observations ------------------------------------------------------------------------------------------------------
def test_without_observations():
    """The value is exactly 0.0; the moments are the restated sweep over a backward filter that never conditions, and
    rodeo_amd.solve_mv_grid's posterior (reached by another recursion) at the same bars."""
    c = fc.make(gc.fhn(3, "rodeo", "distinct", B=3), ())
    ll = _value(c)
    assert ll.shape == (3,) and np.all(ll == 0.0)
    got = _mv(c)
    _check_mv(got, c)
    dm, dv = _mv_diff(got, ra.solve_mv_grid(None, *c.device_args(), **c["params"]))
    print(f"fenrir-grid-check no observations against rodeo_amd.solve_mv_grid: mean {dm:.3e}, var {dv:.3e}")
    assert dm <= fc.MEAN_BAR and dv <= fc.VAR_BAR


# ---- a uniform grid with observations on nodes against fenrir -------------------------------------------------------------
@pytest.mark.parametrize("p,B,n_bobs", [(3, 65, 1), (3, None, 2), (4, 3, 1), (5, 3, 3), (2, 3, 1)])
def test_uniform_grid_against_fenrir(p, B, n_bobs):
    """``fenrir`` / ``fenrir.solve_mv`` on the same nodes.  Bit equality is not promised: those routes read stored predictions (or
    run on the tiles), this one re-evaluates them.  The difference found is printed."""
    c = fc.make(gc.fhn(p, "rodeo", "uniform", B=B), n_bobs=n_bobs)
    t = c["t"]
    obs = (c["y"], t[list(c["nodes"])], c["D"], c["Om"])
    args = (c["ode"], c["W"], c["x0"])
    fn = gc.ITG["rodeo"][0]
    prior = ra.ibm_init(t[1] - t[0], p, c["sigma"])
    unif_args = args + (t[0], t[-1], len(t) - 1, fn, prior) + obs
    ll, got = _value(c), _mv(c)
    llo, ref = fmod.fenrir(None, *unif_args, **c["params"]), fmod.solve_mv(None, *unif_args, **c["params"])
    rel = _value_diff(ll, np.asarray(llo))
    dm, dv = _mv_diff(got, ref)
    bits = np.array_equal(ll, llo) and all(np.array_equal(a, b) for a, b in zip(got, ref))
    print(f"fenrir-grid-check uniform p={p} B={B} n_bobs={n_bobs} against fenrir: value {rel:.3e}, mean {dm:.3e}, var {dv:.3e}; "
          f"bits equal: {bits}")
    assert rel <= fc.VALUE_BAR and dm <= fc.MEAN_BAR and dv <= fc.VAR_BAR


# ---- launch and determinism ----------------------------------------------------------------------------------------------
def test_the_launched_kernels():
    c, c5 = fc.make(gc.fhn(3, "rodeo", "distinct", B=3)), fc.make(gc.fhn(5, "rodeo", "levels", B=3))
    for case in (c, c5):                                             # two blocks: the value goes through the ordered sum
        assert _kernels(lambda: _value(case)) == ["grid_fwd_kernel", "fenrir_grid_bwd_kernel", "magi_sum_kernel"]
        assert _kernels(lambda: _mv(case)) == ["grid_fwd_kernel", "fenrir_grid_bwd_kernel", "fenrir_smooth_kernel"]
    one = fc.FCase(gc.higher(3, "rodeo", "distinct"))                # one block: the lanes write logdens themselves
    y, D, Om = fc.dgc.observations(1, 3, 2)
    one.update(nodes=(0, 40), y=y, D=D, Om=Om, n_bobs=1)
    assert _kernels(lambda: _value(one)) == ["grid_fwd_kernel", "fenrir_grid_bwd_kernel"]
    names = _kernels(lambda: _value(c, _fitz))
    assert names[1:] == ["fenrir_grid_bwd_kernel", "magi_sum_kernel"] and names[0].startswith("grid_fwd_kernel")


@pytest.mark.parametrize("c", [fc.make(gc.fhn(3, "rodeo", "distinct", B=65)), fc.make(gc.fhn(5, "rodeo", "levels", B=65, batched_sigma=True)),
                               fc.make(gc.lorenz(3, "rodeo", "distinct", B=5)), fc.make(gc.lorenz(4, "rodeo", "distinct", B=5))],
                         ids=lambda c: c["label"])
def test_two_calls_give_identical_bytes(c):
    assert _value(c).tobytes() == _value(c).tobytes()
    for a, b in zip(_mv(c), _mv(c)):
        assert a.tobytes() == b.tobytes()


def test_grid_with_times_puts_the_observation_times_on_nodes():
    """Off-node times through grid_with_times: value and moments are the restatement's on the grid it returns, and prior_at is
    called once per slot of that grid."""
    c = fc.times_case("rodeo")
    t, times = c["t"], c["times"]
    assert len(t) == 43 and list(c["nodes"]) == [4, 9, 22]
    calls = []

    def prior_at(h):
        calls.append(h)
        return ra.ibm_init(h, 3, c["sigma"])
    args = (c["ode"], c["W"], c["x0"], t, gc.ITG["rodeo"][0], prior_at, c["y"], times, c["D"], c["Om"])
    ll = fmod.fenrir_grid(None, *args, **c["params"])
    assert len(calls) == len(ra.grid_slots(t)[0]) == 4
    _check_value(ll, c, "grid_with_times")
    _check_mv(fmod.solve_mv_grid(None, *args, **c["params"]), c, "grid_with_times")
