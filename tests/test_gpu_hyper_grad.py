"""
The ``"log_sigma"`` / ``"log_obs_var"`` directions of ``dalton_grid_jvp`` / ``fenrir_grid_jvp`` and the four gradient calls on top of them
 on the device, against the NumPy restatement tests/hyper_grad_oracle.py.

Cases: tests/hyper_grad_cases.py (20 DALTON and 22 Fenrir cases: the problems of the (21) / (23) tests with the unit theta directions,
the unit directions of the two log-scales, a mixed and a zero direction; 1, 33 and 65 items; a per-trajectory hyper direction).
tests/test_oracle_hyper_grad.py checks every one of them on the CPU: the restatement against Richardson differences, no forecast
variance within ten times of the 1e-8 rule, and the restated derivative's own move under R (1 + 1e-15) below a tenth of the bar.

Bars: ``dvalue`` within 1e-7 max |dvalue| of the restatement, per trajectory (the project's device bar); everything that must not
change -- the value, the non-hyper columns of a mixed call, the hyper entry without hyper directions, chunked against unchunked,
two calls -- bit for bit.  Every comparison prints its largest difference ("hyper-grad-check ..." lines).
"""
import ctypes as C
import functools
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401
import rodeo_amd.inference.fenrir  # noqa: F401
from rodeo_amd import _lib
from rodeo_amd.inference import laplace as lap
from rodeo_amd.interrogate import interrogate_kramer
import grid_cases as gc
import dalton_grid_cases as dc
import hyper_grad_cases as hc
import laplace_grad_oracle as lgo
from test_laplace_grad_host import FHN_SHAPE, FHN_START_OFFSET
from test_oracle_hyper_grad import scaling_cases, scaling_identity

pytestmark = pytest.mark.gpu
dmod = sys.modules["rodeo_amd.inference.dalton"]
fmod = sys.modules["rodeo_amd.inference.fenrir"]
JVP = {"dalton": dmod.dalton_grid_jvp, "fenrir": fmod.fenrir_grid_jvp}
VALUE = {"dalton": dmod.dalton_grid, "fenrir": fmod.fenrir_grid}
GRID_GRAD = {"dalton": dmod.dalton_grid_grad, "fenrir": fmod.fenrir_grid_grad}
GRAD = {"dalton": dmod.dalton_grad, "fenrir": fmod.fenrir_grad}
CASES = hc.cases()
IDS = [g["label"] for g in CASES]
BAR = 1e-7


def _pick(*labels):
    """The first case of each family whose label holds every word of an entry of ``labels``."""
    out = []
    for family in ("dalton", "fenrir"):
        for words in labels:
            out.append(next(g for g in CASES if g["family"] == family and all(w in g["label"] for w in words)))
    return out


@functools.lru_cache(maxsize=None)
def _restated(g):
    """The restatement, computed once per case and left unchanged."""
    value, dvalue = g.restate()
    value.setflags(write=False)
    dvalue.setflags(write=False)
    return value, dvalue


@functools.lru_cache(maxsize=None)
def _device(g):
    return g.device_jvp(JVP[g["family"]])


def _error(got, ref):
    ref = np.atleast_2d(ref)
    return float(np.max(np.abs(np.reshape(got, ref.shape) - ref) / np.max(np.abs(ref), axis=1, keepdims=True)))


@pytest.mark.parametrize("g", CASES, ids=IDS)
def test_dvalue_equals_the_restatement(g):
    value, dvalue = _device(g)
    _, ref = _restated(g)
    assert np.shape(value) == (() if g["B"] is None else (g["B"],)) and dvalue.shape == ((g["K"],) if g["B"] is None else (g["B"], g["K"]))
    err = _error(dvalue, ref)
    hyper = hc.hyper_columns(g)
    err_h = float(np.max(np.abs(np.reshape(dvalue, ref.shape) - ref)[:, hyper] / np.max(np.abs(ref), axis=1, keepdims=True)))
    print(f"hyper-grad-check dvalue {g['label']}: {err:.3e} of max|dvalue| per trajectory (bar 1e-7), the hyper columns {err_h:.3e}; "
          f"max|dvalue| {np.max(np.abs(ref), axis=1).min():.3e} .. {np.max(np.abs(ref)):.3e}")
    assert np.all(np.isfinite(dvalue)) and err <= BAR, (g["label"], dvalue, ref)
    for k in hc.zero_directions(g):
        assert np.all(dvalue[..., k] == 0.0), dvalue[..., k]


@pytest.mark.parametrize("g", CASES, ids=IDS)
def test_value_is_the_value_call_s_bit_for_bit(g):
    value, _ = _device(g)
    ref = np.asarray(g["case"].device_call(VALUE[g["family"]]))
    assert np.asarray(value).shape == ref.shape
    np.testing.assert_array_equal(np.asarray(value), ref)


MIXED = _pick(("fhn kramer p=3 distinct N=40 t_max=4.0 B=None", "obs@1,7"), ("per_traj",), ("lorenz kramer p=3",), ("sigma batched",),
              ("N=3 ",))


@pytest.mark.parametrize("g", MIXED, ids=lambda g: g["label"])
def test_the_other_columns_of_a_mixed_call_are_the_plain_call_s_bit_for_bit(g):
    """The directions without a log-scale entry, in the call with the two names and in the same call without them (the parent's
    kernels): a lane's arithmetic on those columns is the same in both kernels."""
    _, dvalue = _device(g)
    plain = [k for k in range(g["K"]) if k not in hc.hyper_columns(g)]
    value, ref = g.device_jvp(JVP[g["family"]], names=("theta", "ode_init"))
    np.testing.assert_array_equal(dvalue[..., plain], ref[..., plain])
    np.testing.assert_array_equal(np.asarray(value), np.asarray(_device(g)[0]))


class _Redirect:
    """The device's library with every plain ``rk_*_grid_jvp`` call sent to the hyper entry with both hyper pointers null."""

    def __init__(self, lib, seen):
        self._lib, self._seen = lib, seen

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ("rk_dalton_grid_jvp", "rk_fenrir_grid_jvp"):
            return fn
        tail = 2 if name == "rk_dalton_grid_jvp" else 3                          # (value, dvalue) / (workspace, value, dvalue)
        hyper = getattr(self._lib, name + "_hyper")

        def redirected(*a):
            self._seen.append(name + "_hyper")
            return hyper(*a[:-tail], None, 0, None, 0, *a[-tail:])
        redirected.__name__ = name
        return redirected


@pytest.mark.parametrize("g", MIXED, ids=lambda g: g["label"])
def test_the_hyper_entry_with_both_pointers_null_gives_the_plain_entry_s_bits(g, monkeypatch):
    v1, d1 = g.device_jvp(JVP[g["family"]], names=("theta", "ode_init"))
    dev, seen = ra.default_device(), []
    monkeypatch.setattr(dev, "lib", _Redirect(dev.lib, seen))
    v2, d2 = g.device_jvp(JVP[g["family"]], names=("theta", "ode_init"))
    assert seen and set(seen) == {f"rk_{g['family']}_grid_jvp_hyper"}
    assert np.asarray(v1).tobytes() == np.asarray(v2).tobytes() and d1.tobytes() == d2.tobytes()


@pytest.mark.parametrize("g", MIXED[:2] + MIXED[5:7], ids=lambda g: g["label"])
def test_two_calls_give_identical_bytes(g):
    v1, d1 = _device(g)
    v2, d2 = g.device_jvp(JVP[g["family"]])
    assert np.asarray(v1).tobytes() == np.asarray(v2).tobytes() and d1.tobytes() == d2.tobytes()


def _grad_args(c):
    return (None,) + c.device_args() + (c["y"], c["t"][list(c["nodes"])], c["D"], c["Om"])


@pytest.mark.parametrize("family", ["dalton", "fenrir"])
@pytest.mark.parametrize("B", [None, 3])
def test_grad_is_jvp_with_unit_directions_bit_for_bit(family, B):
    c = dc.make(gc.fhn(3, "kramer", "distinct", B=B))
    wrt = ("theta", "log_sigma", "ode_init", "log_obs_var")
    res = GRID_GRAD[family](*_grad_args(c), wrt=wrt, **c["params"])
    lead = () if B is None else (B,)
    assert [res.grad[n].shape for n in wrt] == [lead + (3,), lead + (2,), lead + (2, 3), lead + (2,)]
    K = 13
    unit = np.eye(K)
    tangents = dict(theta=unit[:, :3], log_sigma=unit[:, 3:5], ode_init=unit[:, 5:11].reshape(K, 2, 3), log_obs_var=unit[:, 11:])
    value, dvalue = JVP[family](*_grad_args(c), tangents, **c["params"])
    np.testing.assert_array_equal(np.asarray(res.value), np.asarray(value))
    for name, k0, k1 in (("theta", 0, 3), ("log_sigma", 3, 5), ("ode_init", 5, 11), ("log_obs_var", 11, 13)):
        np.testing.assert_array_equal(res.grad[name].reshape(lead + (-1,)), dvalue[..., k0:k1])
    only = GRID_GRAD[family](*_grad_args(c), wrt="log_sigma", **c["params"])     # (a lane's arithmetic does not depend on K)
    np.testing.assert_array_equal(only.grad["log_sigma"], res.grad["log_sigma"])


@pytest.mark.parametrize("g", scaling_cases(), ids=lambda g: g["label"])
def test_scaling_identity_from_three_device_calls(g):
    """The derivative along (log_sigma = 1/2, log_obs_var = 1) is 2 (value(2 R, 2 Omega) - value(R, Omega)) + n ln 2 - n / 2: one
    jvp call (with the unit theta directions, for the yardstick) and two value calls."""
    c = g["case"]
    d, n_theta = c["W"].shape[-3], g.theta.shape[-1]
    tangents = dict(theta=np.concatenate([np.eye(n_theta), np.zeros((1, n_theta))]),
                    log_sigma=np.concatenate([np.zeros((n_theta, d)), np.full((1, d), 0.5)]),
                    log_obs_var=np.concatenate([np.zeros((n_theta, d)), np.ones((1, d))]))
    _, dvalue = JVP[g["family"]](*_grad_args(c), tangents, **c["params"])
    dvalue = np.atleast_2d(dvalue)

    def value_at(r, Om):
        ode, W, x0, t, itg, prior_at = c.device_args()
        scaled = lambda h: (lambda Q, R: (Q, r * R))(*prior_at(h))               # noqa: E731
        return VALUE[g["family"]](None, ode, W, x0, t, itg, scaled, c["y"], c["t"][list(c["nodes"])], c["D"], Om, **c["params"])
    want, n = scaling_identity(g, value_at)
    scale = np.max(np.abs(dvalue), axis=1)
    err = float(np.max(np.abs(dvalue[:, -1] - want) / scale))
    print(f"hyper-grad-check scaling identity {g['label']}: n = {n}; device {dvalue[:, -1]}, identity {want}; {err:.3e} of max|dvalue| "
          f"{scale.max():.3e} (bar 1e-7)")
    assert err <= BAR


@pytest.mark.parametrize("family", ["dalton", "fenrir"])
@pytest.mark.parametrize("itg", ["kramer", "rodeo"])
def test_grad_on_the_uniform_grid(family, itg):
    """``dalton_grad`` / ``fenrir_grad`` with wrt = (theta, log_sigma, log_obs_var) against the restatement on the uniform grid, and
    the value against the same call without the two names, bit for bit."""
    c = dc.make(gc.fhn(3, itg, "uniform", B=3))
    t, N = c["t"], 40
    h = t[1] - t[0]
    nodes = np.array(c["nodes"])
    times = t[nodes] - np.where(np.arange(len(nodes)) % 2 == 0, 0.3 * h, 0.0)    # between nodes: mapped to the next node
    prior = ra.ibm_init(h, 3, c["sigma"])
    args = (None, c["ode"], c["W"], c["x0"], 0.0, t[-1], N, gc.ITG[itg][0], prior, c["y"], times, c["D"], c["Om"])
    res = GRAD[family](*args, wrt=("theta", "log_sigma", "log_obs_var"), **c["params"])
    plain = GRAD[family](*args, wrt=("theta",), **c["params"])
    np.testing.assert_array_equal(res.value, plain.value)
    np.testing.assert_array_equal(res.grad["theta"], plain.grad["theta"])
    unit = np.eye(7)
    g = hc.HCase(case=c, family=family, dtheta=unit[:, :3], dx0=None, dls=unit[:, 3:5], dlo=unit[:, 5:], K=7, B=3, kind="uniform",
                 label="uniform")
    _, want = g.restate()
    got = np.concatenate([res.grad["theta"], res.grad["log_sigma"], res.grad["log_obs_var"]], axis=1)
    err = _error(got, want)
    print(f"hyper-grad-check {family}_grad {itg}: {err:.3e} of max|grad| (bar 1e-7); log_sigma {res.grad['log_sigma'][0]}, "
          f"log_obs_var {res.grad['log_obs_var'][0]}")
    assert err <= BAR


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


@pytest.mark.parametrize("family", ["dalton", "fenrir"])
@pytest.mark.parametrize("itg", ["kramer", "rodeo"])
def test_a_traced_right_hand_side_agrees_with_the_built_in_one(family, itg):
    """One traced Python function (the gradient kind, hiprtc: JIT_DALTON_GRAD_HYPER / JIT_FENRIR_GRAD_HYPER)."""
    g = hc.hyper_case(dc.make(gc.fhn(3, itg, "distinct", B=3)), family, "standard")
    value, dvalue = g.device_jvp(JVP[family])
    tv, td = g.device_jvp(JVP[family], ode=_fitz)
    rel = float(np.max(np.abs(tv - value) / np.maximum(1.0, np.abs(value))))
    err = _error(td, dvalue)
    print(f"hyper-grad-check traced {family} {itg}: value {rel:.3e} relative, dvalue {err:.3e} of max|dvalue| (bars 1e-9)")
    assert rel <= 1e-9 and err <= 1e-9
    assert np.all(td[:, hc.zero_directions(g)] == 0.0)


@pytest.mark.parametrize("g", [next(g for g in hc.fenrir_cases() if word in g["label"]) for word in ("per_traj", "small", "lorenz kramer p=3")],
                         ids=lambda g: g["label"])
def test_fenrir_s_chunks_give_the_bytes_of_one(g, monkeypatch):
    """A budget of two directions' tangent records: K = 9 in chunks of 2, 2, 2, 2, 1 (11: one more), K = 5 in 2, 2, 1, against the
    one-chunk call -- a per-trajectory hyper direction, 65 items, three blocks.  The two new arrays are sliced with the others."""
    c = g["case"]
    B = 1 if g["B"] is None else g["B"]
    N, d, p = len(c["t"]) - 1, c["W"].shape[-3], c["p"]
    per_dir = (N + 1) * d * (p + p * p) * B * 8
    launches = []
    dev = ra.default_device()

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if name != "rk_fenrir_grid_jvp_hyper":
                return fn

            def counted(*a):
                launches.append(a[11])
                return fn(*a)
            counted.__name__ = name
            return counted
    v1, d1 = _device(g)
    monkeypatch.setattr(fmod, "_GRAD_WORKSPACE_BYTES", 2 * per_dir)
    monkeypatch.setattr(dev, "lib", Counting(dev.lib))
    v3, d3 = g.device_jvp(fmod.fenrir_grid_jvp)
    assert launches == [2] * (g["K"] // 2) + [1] * (g["K"] % 2)
    assert np.asarray(v1).tobytes() == np.asarray(v3).tobytes() and d1.tobytes() == d3.tobytes()


def test_every_hyper_instance_ships_and_what_the_plain_entries_refuse_is_refused():
    """profiles/hyper_grad_code_objects.txt leaves no hyper instance out, so there is no refusal of its own to test; what the plain
    entries refuse is refused in Python and in the library with a live handle, and a served call works afterwards."""
    lib, dev = _lib.load(), ra.default_device()
    for family in ("dalton", "fenrir"):
        for base in (gc.fhn(4, "kramer", "distinct"), gc.lorenz(4, "rodeo", "distinct")):
            c = dc.make(base)
            with pytest.raises(NotImplementedError, match="not built"):
                GRID_GRAD[family](*_grad_args(c), wrt=("log_sigma",), **c["params"])
        for rhs, d, p in ((_lib.RHS_FITZHUGH_NAGUMO, 2, 4), (_lib.RHS_LORENZ63, 3, 4), (_lib.RHS_HIGHER_ORDER, 1, 3)):
            cfg = _lib.SolveCfg(n_traj=4, n_steps=10, n_block=d, n_bstate=p, n_bmeas=1, rhs_id=rhs, interrogate=_lib.INTERROGATE_KRAMER,
                                kalman_type=_lib.KALMAN_STANDARD, n_theta=3, flags=_lib.FLAG_BATCH_MINOR, t_min=0.0, t_max=1.0, seed=0,
                                traj_offset=0)
            if family == "dalton":
                rc = lib.rk_dalton_grid_jvp_hyper(dev.h, C.byref(cfg), None, None, None, None, None, 1, 1, None, 1, None, 0, None, 0,
                                                  None, 0, None, 0, None, None)
            else:
                rc = lib.rk_fenrir_grid_jvp_hyper(dev.h, C.byref(cfg), None, None, None, None, None, None, 1, 1, None, 1, None, 0, None, 0,
                                                  None, 0, None, 0, None, None, None)
            assert rc == _lib.RK_ERR_UNSUPPORTED and "not built" in lib.rk_last_error().decode()
        g = next(g for g in CASES if g["family"] == family)
        _, dvalue = g.device_jvp(JVP[family])
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


def test_the_profile_names_the_hyper_kernels_only_with_a_reserved_name():
    gd, gf = _pick(("fhn kramer p=3 distinct N=40 t_max=4.0 B=None", "obs@1,7"))
    assert _kernels(lambda: gd.device_jvp(JVP["dalton"])) == ["dalton_grid_jvp_hyper_kernel"]
    assert _kernels(lambda: gd.device_jvp(JVP["dalton"], names=("theta", "ode_init"))) == ["dalton_grid_jvp_kernel"]
    assert _kernels(lambda: gf.device_jvp(JVP["fenrir"])) == ["fenrir_grid_jvp_fwd_hyper_kernel", "fenrir_grid_jvp_bwd_hyper_kernel",
                                                              "magi_sum_kernel", "magi_sum_kernel"]
    assert _kernels(lambda: gf.device_jvp(JVP["fenrir"], names=("theta",))) == ["fenrir_grid_jvp_fwd_kernel", "fenrir_grid_jvp_bwd_kernel",
                                                                               "magi_sum_kernel", "magi_sum_kernel"]


# ---- laplace_grad over (log theta, x(0), log sigma, log noise variance) ---------------------------------------------------------
def _hyper_value_and_grad(case, chain="exact"):
    """tests/laplace_grad_oracle.py's FitzHugh-Nagumo log-posterior with two more coordinates: u = (log theta, x(0), s, w) with
    sigma = e^s sigma_0 (both blocks) and obs_var = e^w obs_var_0, N(0, 10^2) priors on all seven.  ``fenrir_grad`` has one obs_var a
    call, so the rows of u are grouped by w (a stencil has three values of it).  ``chain="no_log_sigma"`` leaves the log sigma
    factor out of ``pull_back``."""
    import fenrir_grad_oracle as fgr
    init, p, sigma0 = case["init"], case["p"], np.array([0.1, 0.1])
    dt = case["t_max"] / case["N"]

    def value_and_grad(u):
        B = len(u)
        th, v0, s, w = np.exp(u[:, :3]), u[:, 3:5], u[:, 5], u[:, 6]
        X0 = np.stack([init(v0[b], 0.0, theta=th[b]) for b in range(B)])
        J = np.stack([fgr.fhn_init_jac(v0[b], th[b], p) for b in range(B)])
        Q = ra.ibm_init(dt, p, sigma0)[0]
        R = np.stack([ra.ibm_init(dt, p, sigma0 * np.exp(s[b]))[1] for b in range(B)])
        value = np.zeros(B)
        grad = dict(theta=np.zeros((B, 3)), ode_init=np.zeros((B, 2, p)), log_sigma=np.zeros((B, 2)), log_obs_var=np.zeros((B, 2)))
        for wv in np.unique(w):
            rows = np.flatnonzero(w == wv)
            res = fmod.fenrir_grad(None, ra.ode.fitzhugh_nagumo, case["W"], X0[rows], 0.0, case["t_max"], case["N"], interrogate_kramer,
                                   (Q, R[rows]), case["y"], case["obs_times"], case["ow"], np.exp(wv) * case["ov"],
                                   wrt=("theta", "ode_init", "log_sigma", "log_obs_var"), init_jac=dict(theta=J[rows]), theta=th[rows])
            value[rows] = res.value
            for name in grad:
                grad[name][rows] = res.grad[name]
        d_theta = np.zeros((B, 3, 7))
        d_theta[:, np.arange(3), np.arange(3)] = th
        d_x0 = np.zeros((B, 2, p, 7))
        V, (a, b_, c) = v0[:, 0], th.T
        d_x0[:, 0, 0, 3], d_x0[:, 0, 1, 3], d_x0[:, 1, 1, 3] = 1.0, c * (1 - V * V), -1.0 / c
        d_x0[:, 1, 0, 4], d_x0[:, 0, 1, 4], d_x0[:, 1, 1, 4] = 1.0, c, -b_ / c
        d_s, d_w = np.zeros((B, 2, 7)), np.zeros((B, 2, 7))
        d_s[:, :, 5], d_w[:, :, 6] = 1.0, 1.0
        jac = dict(theta=d_theta, ode_init=d_x0, log_sigma=d_s, log_obs_var=d_w)
        if chain == "no_log_sigma":
            del jac["log_sigma"]
        g = lap.pull_back(grad, jac) - u / 100.0
        return value + np.sum(-0.5 * (u / 10.0) ** 2 - np.log(10.0) - 0.5 * np.log(2 * np.pi), axis=1), g
    return value_and_grad


def test_laplace_grad_with_the_two_hyper_coordinates_passes_its_gradient_check_with_the_right_chain_rule():
    """One iteration on tests/laplace_grad_oracle.py's N = 30 case, k = 7.  With kramer and sigma = 0.1 this likelihood hardly feels
    sigma: at the start its derivative in log s is -2.3e-5 next to -16.6 in R(0) (the gradient printed below), and ``check_grad``'s
    bar for it is 10 x 1e-7 x max |g| = 1.7e-5 plus the quotient's own error.  Leaving the log sigma factor out is therefore
    caught, by a factor of 1.4; the derivative in log w, -3.8, leaves no such question."""
    case = lgo.fhn_case(**FHN_SHAPE)
    start = np.concatenate([np.log(case["theta"]), case["x0"], [0.0, 0.0]]) + FHN_START_OFFSET
    vg = _hyper_value_and_grad(case)
    _, g0 = vg(start[None])
    print(f"hyper-grad-check laplace_grad: gradient at the start {g0[0]}")
    res = lap.laplace_grad(vg, start, max_iter=1, check_grad=True)                # raises if the quotients disagree
    assert res.n_iter == 1 and res.n_bad == 0
    wrong = _hyper_value_and_grad(case, chain="no_log_sigma")
    with pytest.raises(ValueError, match=r"laplace_grad: the gradient of value_and_grad disagrees .* coordinate 5"):
        lap.laplace_grad(wrong, start, max_iter=1)
    assert lap.laplace_grad(wrong, start, max_iter=1, check_grad=False).n_iter == 1
