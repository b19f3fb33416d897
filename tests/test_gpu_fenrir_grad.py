"""
``fenrir_grid_jvp`` / ``fenrir_grid_grad`` / ``fenrir_grad`` (``rodeo_amd.inference.fenrir``) on the device against the NumPy
restatement of the tangent recursion, tests/fenrir_grad_oracle.py, and the value against ``fenrir_grid`` on the same inputs.

Cases: tests/fenrir_grad_cases.py (the 19 cases of the DALTON gradients re-read as Fenrir cases -- node 0 observed, node N
unobserved, N = 1, 2, 3, n_bstate 2 and 3, three blocks, a batched sigma, (B, K) = (1, 1), (3, 5), (11, 3), (33, 1) -- then 65
items, a second forward wave with one live item, and two cases at 100 x the prior scale, where Sigma. reaches the value).
tests/test_oracle_fenrir_grad.py checks every one of them on the CPU: the restatement against finite differences, no y forecast
variance within ten times of the 1e-8 rule, and the restated gradient's own move under R (1 + 1e-15) below a tenth of the bar.

Bars: ``dvalue`` within 1e-7 max |grad| of the restatement, per trajectory (tests/test_gpu_dalton_grad.py's bar, a hundred times
the loosest CPU bar); ``value`` within 1e-9 max(1, |value|) of ``fenrir_grid``.  Every comparison prints its largest difference
("fenrir-grad-check ..." lines).
"""
import ctypes as C
import functools
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.fenrir  # noqa: F401
from rodeo_amd import _lib
import grid_cases as gc
import dalton_grid_cases as dc
import fenrir_grid_cases as fc
import fenrir_grad_cases as fgc
import fenrir_grad_oracle as fgr

pytestmark = pytest.mark.gpu
fmod = sys.modules["rodeo_amd.inference.fenrir"]
CASES = fgc.cases()
IDS = [g["label"] for g in CASES]


@functools.lru_cache(maxsize=None)
def _restated(g):
    """The restatement, computed once per case and left unchanged."""
    value, dvalue = g.restate()
    value.setflags(write=False)
    dvalue.setflags(write=False)
    return value, dvalue


@functools.lru_cache(maxsize=None)
def _device(g):
    return g.device_jvp(fmod.fenrir_grid_jvp)


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
    print(f"fenrir-grad-check dvalue {g['label']}: {err:.3e} of max|grad| per trajectory (bar 1e-7); max|grad| {scale.min():.3e} .. {scale.max():.3e}")
    assert np.all(np.isfinite(got)) and err <= 1e-7, (g["label"], got, ref)


@pytest.mark.parametrize("g", CASES, ids=IDS)
def test_value_equals_fenrir_grid(g):
    value, _ = _device(g)
    ref = np.asarray(g["case"].device_call(fmod.fenrir_grid))
    value = np.asarray(value)
    assert value.shape == ref.shape
    rel = float(np.max(np.abs(value - ref) / np.maximum(1.0, np.abs(ref))))
    print(f"fenrir-grad-check value {g['label']}: {rel:.3e} relative to fenrir_grid (bar 1e-9); bit for bit: {bool(np.all(value == ref))}")
    assert rel <= 1e-9, (g["label"], value, ref)


@pytest.mark.parametrize("g", [g for g in CASES if fgc.zero_directions(g)], ids=lambda g: g["label"])
def test_a_zero_direction_gives_exactly_zero(g):
    _, dvalue = _device(g)
    for k in fgc.zero_directions(g):
        assert np.all(dvalue[..., k] == 0.0), dvalue[..., k]


@pytest.mark.parametrize("g", [CASES[0], CASES[4], CASES[5], CASES[13]], ids=lambda g: g["label"])
def test_two_calls_give_identical_bytes(g):
    v1, d1 = _device(g)
    v2, d2 = g.device_jvp(fmod.fenrir_grid_jvp)
    assert np.asarray(v1).tobytes() == np.asarray(v2).tobytes() and d1.tobytes() == d2.tobytes()


@pytest.mark.parametrize("g", [CASES[4], CASES[5], CASES[19]], ids=lambda g: g["label"])
def test_three_chunks_give_the_bytes_of_one(g, monkeypatch):
    """K = 5 in chunks of 2, 2 and 1 directions (a budget of two directions' tangent records), and Lorenz63's K = 3 in chunks of
    one, against the one-chunk call: two blocks and three, a per-trajectory direction, 65 items."""
    assert g["K"] == 5 or g["K"] == 3
    c = g["case"]
    B = 1 if g["B"] is None else g["B"]
    N, d, p = len(c["t"]) - 1, c["W"].shape[-3], c["p"]
    per_dir = (N + 1) * d * (p + p * p) * B * 8
    launches = []
    dev = ra.default_device()

    class Counting:
        """The device's library with the direction count of every rk_fenrir_grid_jvp call written down."""

        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if name != "rk_fenrir_grid_jvp":
                return fn

            def counted(*a):
                launches.append(a[11])
                return fn(*a)
            return counted
    v1, d1 = _device(g)
    monkeypatch.setattr(fmod, "_GRAD_WORKSPACE_BYTES", 2 * per_dir if g["K"] == 5 else per_dir)
    monkeypatch.setattr(dev, "lib", Counting(dev.lib))
    v3, d3 = g.device_jvp(fmod.fenrir_grid_jvp)
    assert launches == ([2, 2, 1] if g["K"] == 5 else [1, 1, 1])
    assert np.asarray(v1).tobytes() == np.asarray(v3).tobytes() and d1.tobytes() == d3.tobytes()


def _grad_args(c):
    return (None,) + c.device_args() + (c["y"], c["t"][list(c["nodes"])], c["D"], c["Om"])


@pytest.mark.parametrize("B", [None, 3])
def test_grad_is_jvp_with_unit_directions_bit_for_bit(B):
    c = dc.make(gc.fhn(3, "kramer", "distinct", B=B))
    res = fmod.fenrir_grid_grad(*_grad_args(c), wrt=("theta", "ode_init"), **c["params"])
    lead = () if B is None else (B,)
    assert isinstance(res, fmod.FenrirGrad) and res.grad["theta"].shape == lead + (3,) and res.grad["ode_init"].shape == lead + (2, 3)
    dth = np.concatenate([np.eye(3), np.zeros((6, 3))])
    dx = np.concatenate([np.zeros((3, 2, 3)), np.eye(6).reshape(6, 2, 3)])
    value, dvalue = fmod.fenrir_grid_jvp(*_grad_args(c), dict(theta=dth, ode_init=dx), **c["params"])
    np.testing.assert_array_equal(np.asarray(res.value), np.asarray(value))
    np.testing.assert_array_equal(res.grad["theta"], dvalue[..., :3])
    np.testing.assert_array_equal(res.grad["ode_init"], dvalue[..., 3:].reshape(lead + (2, 3)))
    only = fmod.fenrir_grid_grad(*_grad_args(c), **c["params"])                   # wrt = ("theta",), the default
    assert set(only.grad) == {"theta"}
    np.testing.assert_array_equal(only.grad["theta"], res.grad["theta"])         # (a lane's arithmetic does not depend on K)


def test_grad_with_init_jac_is_the_total_derivative():
    c = dc.make(gc.fhn(3, "kramer", "distinct"))
    J = fgr.fhn_init_jac(np.array([-1.0, 1.0]), gc.THETA, 3)
    res = fmod.fenrir_grid_grad(*_grad_args(c), wrt=("theta",), init_jac=dict(theta=J), **c["params"])
    g = fgc.FGCase(case=c, dtheta=np.eye(3), dx0=np.moveaxis(J, -1, 0), K=3, B=None, label="init_jac")
    _, ref = g.restate()
    err = float(np.max(np.abs(res.grad["theta"] - ref[0])) / np.max(np.abs(ref)))
    print(f"fenrir-grad-check init_jac: {err:.3e} of max|grad| (bar 1e-7); total derivative {res.grad['theta']}")
    assert err <= 1e-7


@pytest.mark.parametrize("itg", ["kramer", "rodeo"])
def test_fenrir_grad_on_the_uniform_grid(itg):
    """``fenrir_grad`` against ``fenrir``'s value (fenrir_grid_cases.VALUE_BAR) and the restatement's gradient on the uniform grid;
    observation times between nodes, mapped by ``fenrir``'s rule (the next node; with rodeo the last one lies past t_max)."""
    base = gc.fhn(3, itg, "uniform", B=3)
    c = dc.make(base)
    t, N = c["t"], 40
    h = t[1] - t[0]
    nodes = np.array(c["nodes"])
    times = t[nodes] - np.where(np.arange(len(nodes)) % 2 == 0, 0.3 * h, 0.0)
    if itg == "rodeo":
        times[-1] = t[-1] + 0.5 * h                                              # past t_max: node N, as fenrir takes it
    prior = ra.ibm_init(h, 3, c["sigma"])
    args = (None, c["ode"], c["W"], c["x0"], 0.0, t[-1], N, gc.ITG[itg][0], prior, c["y"], times, c["D"], c["Om"])
    res = fmod.fenrir_grad(*args, wrt=("theta", "ode_init"), **c["params"])
    ref = fmod.fenrir(*args, **c["params"])
    rel = float(np.max(np.abs(res.value - ref) / np.maximum(1.0, np.abs(ref))))
    dth = np.concatenate([np.eye(3), np.zeros((6, 3))])
    dx = np.concatenate([np.zeros((3, 2, 3)), np.eye(6).reshape(6, 2, 3)])
    _, want = fgc.FGCase(case=c, dtheta=dth, dx0=dx, K=9, B=3, label="uniform").restate()
    got = np.concatenate([res.grad["theta"], res.grad["ode_init"].reshape(3, 6)], axis=1)
    err = float(np.max(np.abs(got - want) / np.max(np.abs(want), axis=1, keepdims=True)))
    print(f"fenrir-grad-check fenrir_grad {itg}: value {rel:.3e} relative to fenrir (bar {fc.VALUE_BAR:.0e}), bit for bit: "
          f"{bool(np.all(res.value == ref))}; gradient {err:.3e} of max|grad| (bar 1e-7)")
    assert rel <= fc.VALUE_BAR and err <= 1e-7


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


@pytest.mark.parametrize("itg", ["kramer", "rodeo"])
def test_a_traced_right_hand_side_agrees_with_the_built_in_one(itg):
    """One traced Python function (the gradient kind, hiprtc: JIT_FENRIR_GRAD), two builds of the forward kernel."""
    g = fgc.fenrir_case(dc.make(gc.fhn(3, itg, "distinct", B=3)), "small")
    value, dvalue = g.device_jvp(fmod.fenrir_grid_jvp)
    tv, td = g.device_jvp(fmod.fenrir_grid_jvp, ode=_fitz)
    rel = float(np.max(np.abs(tv - value) / np.maximum(1.0, np.abs(value))))
    err = float(np.max(np.abs(td - dvalue) / np.max(np.abs(dvalue), axis=1, keepdims=True)))
    print(f"fenrir-grad-check traced {itg}: value {rel:.3e} relative, dvalue {err:.3e} of max|grad| (bars 1e-9)")
    assert rel <= 1e-9 and err <= 1e-9
    assert np.all(td[:, fgc.zero_directions(g)] == 0.0)


def test_every_refused_instance_raises_and_leaves_the_handle_usable():
    """The instances that are not built and the other refusals, in Python and in the library with a live handle; a served call
    afterwards still works."""
    lib, dev = _lib.load(), ra.default_device()
    for base in (gc.fhn(4, "kramer", "distinct"), gc.fhn(5, "rodeo", "levels"), gc.lorenz(4, "rodeo", "distinct")):
        g = fgc.fenrir_case(dc.make(base), "theta")
        with pytest.raises(NotImplementedError, match="not built"):
            g.device_jvp(fmod.fenrir_grid_jvp)
        with pytest.raises(NotImplementedError, match="not built"):
            fmod.fenrir_grid_grad(*_grad_args(g["case"]), **g["case"]["params"])
    with pytest.raises(NotImplementedError, match="not built"):                  # n_bobs = 2
        fgc.fenrir_case(dc.make(gc.fhn(3, "kramer", "distinct", B=3), n_bobs=2), "theta").device_jvp(fmod.fenrir_grid_jvp)
    for rhs, d, p in ((_lib.RHS_FITZHUGH_NAGUMO, 2, 4), (_lib.RHS_LORENZ63, 3, 4), (_lib.RHS_HIGHER_ORDER, 1, 3)):
        cfg = _lib.SolveCfg(n_traj=4, n_steps=10, n_block=d, n_bstate=p, n_bmeas=1, rhs_id=rhs, interrogate=_lib.INTERROGATE_KRAMER,
                            kalman_type=_lib.KALMAN_STANDARD, n_theta=3, flags=_lib.FLAG_BATCH_MINOR, t_min=0.0, t_max=1.0, seed=0,
                            traj_offset=0)
        rc = lib.rk_fenrir_grid_jvp(dev.h, C.byref(cfg), None, None, None, None, None, None, 1, 1, None, 1, None, 0, None, 0, None, None,
                                    None)
        assert rc == _lib.RK_ERR_UNSUPPORTED and "not built" in lib.rk_last_error().decode()
    g = CASES[0]
    _, dvalue = g.device_jvp(fmod.fenrir_grid_jvp)
    np.testing.assert_array_equal(dvalue, _device(g)[1])


def _kernels(call):
    """Names of the kernels that `call` launched last (the handle's per-launch profile)."""
    dev = ra.default_device()
    dev.profile_enable(True)
    try:
        call()
        return [name for name, _ in dev.profile_last()]
    finally:
        dev.profile_enable(False)


def test_the_profile_names_the_new_kernels_and_the_block_sums():
    """More than one block (every built-in right-hand side): the two new kernels, then magi_sum_kernel for value and for dvalue."""
    for g in (CASES[0], CASES[5]):
        names = _kernels(lambda: g.device_jvp(fmod.fenrir_grid_jvp))
        assert names == ["fenrir_grid_jvp_fwd_kernel", "fenrir_grid_jvp_bwd_kernel", "magi_sum_kernel", "magi_sum_kernel"], names


def _logistic(X, t, theta):
    return np.array([[theta[0] * X[0, 0] * (1.0 - X[0, 0] / theta[1])]])


def test_one_block_writes_value_and_dvalue_without_a_block_sum():
    """A traced one-block right-hand side: the backward lanes write value / dvalue themselves.  The value against ``fenrir_grid`` at
    1e-9; the derivative against Richardson central differences of the device's ``fenrir_grid`` (steps 1e-3 and 5e-4) at 1e-6 of
    max |grad|: the quotient's rounding is about 2e-16 |value| / 5e-4 and its truncation is of fourth order in the step."""
    p, B = 3, 3
    W, init = ra.utils.first_order_pad(_logistic, 1, p)
    theta = np.array([1.5, 2.0]) * (1 + 0.05 * np.arange(B)[:, None])
    x0 = np.stack([init(np.array([0.3]), 0.0, theta=th) for th in theta])
    t = np.concatenate([np.linspace(0.0, 0.5, 11), np.linspace(0.6, 2.0, 15)])
    nodes = [0, 4, 12, 25]
    rng = np.random.default_rng(5)
    y = 0.5 + 0.1 * rng.standard_normal((4, 1, 1))
    D = np.zeros((4, 1, 1, p))
    D[..., 0] = 1.0
    Om = np.full((4, 1, 1, 1), 0.05 ** 2)
    prior_at = lambda h: ra.ibm_init(h, p, np.array([0.5]))                                    # noqa: E731
    args = lambda x0: (None, _logistic, W, x0, t, ra.interrogate.interrogate_kramer, prior_at, y, t[nodes], D, Om)   # noqa: E731
    names = _kernels(lambda: fmod.fenrir_grid_grad(*args(x0), wrt=("theta", "ode_init"), theta=theta))
    assert names == ["fenrir_grid_jvp_fwd_kernel<user>", "fenrir_grid_jvp_bwd_kernel"], names
    res = fmod.fenrir_grid_grad(*args(x0), wrt=("theta", "ode_init"), theta=theta)
    ref = fmod.fenrir_grid(*args(x0), theta=theta)
    assert np.max(np.abs(res.value - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-9
    got = np.concatenate([res.grad["theta"], res.grad["ode_init"].reshape(B, p)], axis=1)
    est = np.zeros_like(got)
    for j in range(2 + p):
        dth, dx = np.zeros(2), np.zeros((1, p))
        if j < 2:
            dth[j] = 1.0
        else:
            dx[0, j - 2] = 1.0
        f = lambda e: fmod.fenrir_grid(*args(x0 + e * dx), theta=theta + e * dth)                # noqa: E731
        h = 1e-3
        d1, d2 = (f(h) - f(-h)) / (2 * h), (f(h / 2) - f(-h / 2)) / h
        est[:, j] = (4 * d2 - d1) / 3
    err = float(np.max(np.abs(got - est) / np.max(np.abs(est), axis=1, keepdims=True)))
    print(f"fenrir-grad-check one block: {err:.3e} of max|grad| against differences of fenrir_grid (bar 1e-6); gradient {got[0]}")
    assert np.all(np.isfinite(got)) and err <= 1e-6
