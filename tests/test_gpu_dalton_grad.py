"""
``dalton_grid_jvp`` / ``dalton_grid_grad`` / ``dalton_grad`` (``rodeo_amd.inference.dalton``) on the device against the NumPy
restatement of the tangent recursion, tests/dalton_grad_oracle.py, and the value against ``dalton_grid`` on the same inputs.

Cases: tests/dalton_grad_cases.py (FitzHugh-Nagumo at n_bstate 2 and 3 with the three interrogations, Lorenz63 at 2 and 3, a batched
sigma, N = 1, 2, 3, observations on node 0 / neighbours / node N, times put in by ``grid_with_times``; unit, mixed, per-trajectory
and zero directions; (B, K) = (1, 1), (3, 5), (11, 3) -- 33 items, a second wave with one live pair -- and (33, 1)).
tests/test_oracle_dalton_grad.py checks every one of them on the CPU: the restatement against finite differences, no forecast
variance within ten times of the 1e-8 rule, and the restated gradient's own move under R (1 + 1e-15) below a tenth of the bar.

Bars: ``dvalue`` within 1e-7 max |grad| of the restatement, per trajectory (1e-7 relative is the project's device-against-
restatement bar for ``dalton``); ``value`` within 1e-9 relative of ``dalton_grid`` (the cross-route bar).  Every comparison prints
its largest difference ("dalton-grad-check ..." lines).
"""
import functools
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401
from rodeo_amd import _lib
import grid_cases as gc
import dalton_grid_cases as dc
import dalton_grad_cases as gcs
import dalton_grad_oracle as dgr

pytestmark = pytest.mark.gpu
dmod = sys.modules["rodeo_amd.inference.dalton"]         # (rodeo_amd.inference.dalton, the attribute, is the function)
CASES = gcs.cases()
IDS = [g["label"] for g in CASES]


@functools.lru_cache(maxsize=None)
def _restated(g):
    """The restatement, computed once per case and left unchanged."""
    return g.restate()


@functools.lru_cache(maxsize=None)
def _device(g):
    return g.device_jvp(dmod.dalton_grid_jvp)


def _shapes(g):
    return (() if g["B"] is None else (g["B"],)), ((g["K"],) if g["B"] is None else (g["B"], g["K"]))


@pytest.mark.parametrize("g", CASES, ids=IDS)
def test_dvalue_equals_the_restatement(g):
    value, dvalue = _device(g)
    _, ref = _restated(g)
    assert np.shape(value) == _shapes(g)[0] and dvalue.shape == _shapes(g)[1]
    got = np.reshape(dvalue, ref.shape)
    scale = np.max(np.abs(ref), axis=1, keepdims=True)
    err = float(np.max(np.abs(got - ref) / scale))
    print(f"dalton-grad-check dvalue {g['label']}: {err:.3e} of max|grad| per trajectory (bar 1e-7); max|grad| {scale.min():.3e} .. {scale.max():.3e}")
    assert np.all(np.isfinite(got)) and err <= 1e-7, (g["label"], got, ref)


@pytest.mark.parametrize("g", CASES, ids=IDS)
def test_value_equals_dalton_grid(g):
    value, _ = _device(g)
    ref = np.asarray(g["case"].device_call(dmod.dalton_grid))
    value = np.asarray(value)
    assert value.shape == ref.shape
    rel = float(np.max(np.abs(value - ref) / np.maximum(1.0, np.abs(ref))))
    print(f"dalton-grad-check value {g['label']}: {rel:.3e} relative to dalton_grid (bar 1e-9); bit for bit: {bool(np.all(value == ref))}")
    assert rel <= 1e-9, (g["label"], value, ref)


@pytest.mark.parametrize("g", [g for g in CASES if gcs.zero_directions(g)], ids=lambda g: g["label"])
def test_a_zero_direction_gives_exactly_zero(g):
    _, dvalue = _device(g)
    for k in gcs.zero_directions(g):
        assert np.all(dvalue[..., k] == 0.0), dvalue[..., k]


@pytest.mark.parametrize("g", [CASES[0], CASES[4], CASES[13]], ids=lambda g: g["label"])
def test_two_calls_give_identical_bits(g):
    v1, d1 = _device(g)
    v2, d2 = g.device_jvp(dmod.dalton_grid_jvp)
    np.testing.assert_array_equal(np.asarray(v1), np.asarray(v2))
    np.testing.assert_array_equal(d1, d2)


def _grad_args(c):
    return (None,) + c.device_args() + (c["y"], c["t"][list(c["nodes"])], c["D"], c["Om"])


@pytest.mark.parametrize("B", [None, 3])
def test_grad_is_jvp_with_unit_directions_bit_for_bit(B):
    c = dc.make(gc.fhn(3, "kramer", "distinct", B=B))
    res = dmod.dalton_grid_grad(*_grad_args(c), wrt=("theta", "ode_init"), **c["params"])
    lead = () if B is None else (B,)
    assert isinstance(res, dmod.DaltonGrad) and res.grad["theta"].shape == lead + (3,) and res.grad["ode_init"].shape == lead + (2, 3)
    dth = np.concatenate([np.eye(3), np.zeros((6, 3))])
    dx = np.concatenate([np.zeros((3, 2, 3)), np.eye(6).reshape(6, 2, 3)])
    value, dvalue = dmod.dalton_grid_jvp(*_grad_args(c), dict(theta=dth, ode_init=dx), **c["params"])
    np.testing.assert_array_equal(np.asarray(res.value), np.asarray(value))
    np.testing.assert_array_equal(res.grad["theta"], dvalue[..., :3])
    np.testing.assert_array_equal(res.grad["ode_init"], dvalue[..., 3:].reshape(lead + (2, 3)))
    only = dmod.dalton_grid_grad(*_grad_args(c), **c["params"])                   # wrt = ("theta",), the default
    scale = np.max(np.abs(res.grad["theta"]))
    assert set(only.grad) == {"theta"} and np.max(np.abs(only.grad["theta"] - res.grad["theta"])) <= 1e-12 * scale


def test_grad_with_init_jac_is_the_total_derivative():
    c = dc.make(gc.fhn(3, "kramer", "distinct"))
    J = dgr.fhn_init_jac(np.array([-1.0, 1.0]), gc.THETA, 3)
    res = dmod.dalton_grid_grad(*_grad_args(c), wrt=("theta",), init_jac=dict(theta=J), **c["params"])
    g = gcs.GCase(case=c, dtheta=np.eye(3), dx0=np.moveaxis(J, -1, 0), K=3, B=None, label="init_jac")
    _, ref = g.restate()
    err = float(np.max(np.abs(res.grad["theta"] - ref[0])) / np.max(np.abs(ref)))
    print(f"dalton-grad-check init_jac: {err:.3e} of max|grad| (bar 1e-7); total derivative {res.grad['theta']}")
    assert err <= 1e-7


@pytest.mark.parametrize("itg", ["kramer", "rodeo"])
def test_dalton_grad_on_the_uniform_grid(itg):
    """``dalton_grad`` against ``dalton``'s value (1e-9 relative) and the restatement's gradient on the uniform grid; observation
    times between nodes, mapped by ``dalton``'s rule (the next node), one of them past t_max (it never matches)."""
    base = gc.fhn(3, itg, "uniform", B=3)
    c = dc.make(base)
    t, N = c["t"], 40
    h = t[1] - t[0]
    nodes = np.array(c["nodes"])
    times = np.concatenate([t[nodes] - np.where(np.arange(len(nodes)) % 2 == 0, 0.3 * h, 0.0), [t[-1] + 0.5 * h]])
    y, D, Om = dc.observations(2, 3, len(times))
    prior = ra.ibm_init(h, 3, c["sigma"])
    args = (None, c["ode"], c["W"], c["x0"], 0.0, t[-1], N, gc.ITG[itg][0], prior, y, times, D, Om)
    res = dmod.dalton_grad(*args, wrt=("theta", "ode_init"), **c["params"])
    ref = dmod.dalton(*args, **c["params"])
    rel = float(np.max(np.abs(res.value - ref) / np.maximum(1.0, np.abs(ref))))
    moved = dc.DCase(c)
    moved.update(y=y[:-1], D=D[:-1], Om=Om[:-1])
    dth = np.concatenate([np.eye(3), np.zeros((6, 3))])
    dx = np.concatenate([np.zeros((3, 2, 3)), np.eye(6).reshape(6, 2, 3)])
    _, want = gcs.GCase(case=moved, dtheta=dth, dx0=dx, K=9, B=3, label="uniform").restate()
    got = np.concatenate([res.grad["theta"], res.grad["ode_init"].reshape(3, 6)], axis=1)
    err = float(np.max(np.abs(got - want) / np.max(np.abs(want), axis=1, keepdims=True)))
    print(f"dalton-grad-check dalton_grad {itg}: value {rel:.3e} relative to dalton (bar 1e-9), bit for bit: {bool(np.all(res.value == ref))}; "
          f"gradient {err:.3e} of max|grad| (bar 1e-7)")
    assert rel <= 1e-9 and err <= 1e-7


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


@pytest.mark.parametrize("itg", ["kramer", "rodeo"])
def test_a_traced_right_hand_side_agrees_with_the_built_in_one(itg):
    """One traced Python function (the gradient kind, hiprtc: JIT_DALTON_GRAD), two builds."""
    g = gcs.grad_case(dc.make(gc.fhn(3, itg, "distinct", B=3)), "small")
    value, dvalue = g.device_jvp(dmod.dalton_grid_jvp)
    tv, td = g.device_jvp(dmod.dalton_grid_jvp, ode=_fitz)
    rel = float(np.max(np.abs(tv - value) / np.maximum(1.0, np.abs(value))))
    err = float(np.max(np.abs(td - dvalue) / np.max(np.abs(dvalue), axis=1, keepdims=True)))
    print(f"dalton-grad-check traced {itg}: value {rel:.3e} relative, dvalue {err:.3e} of max|grad| (bars 1e-9)")
    assert rel <= 1e-9 and err <= 1e-9
    assert np.all(td[:, gcs.zero_directions(g)] == 0.0)


def test_an_empty_observation_set_gives_zero():
    c = dc.make(gc.fhn(3, "kramer", "distinct", B=3), ())
    g = gcs.grad_case(c, "small")
    value, dvalue = g.device_jvp(dmod.dalton_grid_jvp)
    assert value.shape == (3,) and dvalue.shape == (3, 5) and np.all(value == 0.0) and np.all(dvalue == 0.0)


def test_every_refused_instance_raises_and_leaves_the_handle_usable():
    """What profiles/dalton_grad_code_objects.txt leaves out -- FitzHugh-Nagumo from n_bstate 4, Lorenz63 from 4 -- and the other
    refusals, in Python and in the library; a served call afterwards still works."""
    lib, dev = _lib.load(), ra.default_device()
    for base in (gc.fhn(4, "kramer", "distinct"), gc.fhn(5, "rodeo", "levels"), gc.lorenz(4, "rodeo", "distinct")):
        g = gcs.grad_case(dc.make(base), "theta")
        with pytest.raises(NotImplementedError, match="not built"):
            g.device_jvp(dmod.dalton_grid_jvp)
        with pytest.raises(NotImplementedError, match="not built"):
            dmod.dalton_grid_grad(*_grad_args(g["case"]), **g["case"]["params"])
    with pytest.raises(NotImplementedError, match="not built"):                  # n_bobs = 2
        gcs.grad_case(dc.make(gc.fhn(3, "kramer", "distinct", B=3), n_bobs=2), "theta").device_jvp(dmod.dalton_grid_jvp)
    for rhs, d, p in ((_lib.RHS_FITZHUGH_NAGUMO, 2, 4), (_lib.RHS_LORENZ63, 3, 4), (_lib.RHS_HIGHER_ORDER, 1, 3)):
        cfg = _lib.SolveCfg(n_traj=4, n_steps=10, n_block=d, n_bstate=p, n_bmeas=1, rhs_id=rhs, interrogate=_lib.INTERROGATE_KRAMER,
                            kalman_type=_lib.KALMAN_STANDARD, n_theta=3, flags=_lib.FLAG_BATCH_MINOR, t_min=0.0, t_max=1.0, seed=0,
                            traj_offset=0)
        import ctypes as C
        rc = lib.rk_dalton_grid_jvp(dev.h, C.byref(cfg), None, None, None, None, None, 1, 1, None, 1, None, 0, None, 0, None, None)
        assert rc == _lib.RK_ERR_UNSUPPORTED and "not built" in lib.rk_last_error().decode()
    g = CASES[0]
    _, dvalue = g.device_jvp(dmod.dalton_grid_jvp)
    np.testing.assert_array_equal(dvalue, _device(g)[1])
