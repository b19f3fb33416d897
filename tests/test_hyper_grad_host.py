"""
The ``"log_sigma"`` / ``"log_obs_var"`` directions of the six gradient calls on the host (no GPU): the two
names reach the device (``default_device`` patched to fail), every refusal that comes before any device work, the staging layout
and batched flags, which entry a call launches (on a recording stand-in for the plan), Fenrir's chunks slicing the new arrays
with the others, the library's refusals on the configuration alone, both hiprtc kinds built without a device, the tracer's emitted
text, and ``laplace.pull_back`` on a dict that holds the two names.
"""
import ctypes as C
import hashlib
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401
import rodeo_amd.inference.fenrir  # noqa: F401
from rodeo_amd import _lib
from rodeo_amd.inference import laplace
from rodeo_amd.interrogate import interrogate_kramer
from rodeo_amd.trace import from_python, grad_from_python, trace_grad_source, trace_source

dmod = sys.modules["rodeo_amd.inference.dalton"]             # (rodeo_amd.inference.dalton, the attribute, is the function)
fmod = sys.modules["rodeo_amd.inference.fenrir"]
JVP = {"dalton_grid_jvp": dmod.dalton_grid_jvp, "fenrir_grid_jvp": fmod.fenrir_grid_jvp}
GRID_GRAD = {"dalton_grid_grad": dmod.dalton_grid_grad, "fenrir_grid_grad": fmod.fenrir_grid_grad}
GRAD = {"dalton_grad": dmod.dalton_grad, "fenrir_grad": fmod.fenrir_grad}
HYPER = ("log_sigma", "log_obs_var")


def _fhn(p=3, times=(0.1, 0.3), B=None, ode=ra.ode.fitzhugh_nagumo, **over):
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    theta = np.array([0.2, 0.2, 3.0]) if B is None else np.array([0.2, 0.2, 3.0]) * (1 + 0.01 * np.arange(B)[:, None])
    sigma = np.array([0.5, 0.3])
    n = len(times)
    D = np.zeros((n, 2, 1, p))
    D[..., 0, 0] = 1.0
    a = dict(key=None, ode_fun=ode, ode_weight=W, ode_init=init(np.array([-1.0, 1.0]), 0.0, theta=theta),
             t_grid=np.array([0.0, 0.1, 0.15, 0.3, 0.4]), interrogate=interrogate_kramer, prior_at=lambda h: ra.ibm_init(h, p, sigma),
             obs_data=np.zeros((n, 2, 1)), obs_times=np.array(times, dtype=float), obs_weight=D,
             obs_var=np.tile(0.01 * np.eye(1), (n, 2, 1, 1)), tangents=dict(log_sigma=np.eye(2)), theta=theta)
    a.update(over)
    return a


def _grad(**over):
    a = _fhn(**over)
    a.pop("tangents")
    return a


def _uniform(**over):
    a = _grad()
    a.pop("t_grid")
    prior_at = a.pop("prior_at")
    return dict(dict(a, t_min=0.0, t_max=0.4, n_steps=4, prior_pars=prior_at(0.1)), **over)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device fails the test: the refusals below come first."""
    def fail(*a, **k):
        raise AssertionError("default_device was reached")
    monkeypatch.setattr(ra.device, "default_device", fail)
    monkeypatch.setattr(ra.solve, "default_device", fail)


# ---- the two names are served ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("who", sorted(JVP))
def test_the_two_names_reach_the_device_in_tangents(no_device, who):
    for tangents in (dict(log_sigma=np.eye(2)), dict(log_obs_var=np.ones((3, 2))),
                     dict(theta=np.ones((2, 3)), ode_init=np.ones((2, 2, 3)), log_sigma=np.ones((2, 2)), log_obs_var=np.ones((2, 2)))):
        with pytest.raises(AssertionError, match="default_device was reached"):
            JVP[who](**_fhn(tangents=tangents))
    with pytest.raises(AssertionError, match="default_device was reached"):          # a direction of every trajectory's own
        JVP[who](**_fhn(B=4, tangents=dict(log_sigma=np.ones((4, 3, 2)), log_obs_var=np.ones((3, 2)))))
    with pytest.raises(AssertionError, match="default_device was reached"):
        JVP[who](**_fhn(p=2, tangents=dict(log_obs_var=np.ones((1, 2)))))


@pytest.mark.parametrize("who", sorted(GRID_GRAD))
def test_the_two_names_reach_the_device_in_wrt(no_device, who):
    for wrt in ("log_sigma", ("log_obs_var",), ("theta", "log_sigma", "log_obs_var"), ("log_sigma", "ode_init", "theta")):
        with pytest.raises(AssertionError, match="default_device was reached"):
            GRID_GRAD[who](**_grad(), wrt=wrt)
    with pytest.raises(AssertionError, match="default_device was reached"):
        GRAD[who.replace("_grid", "")](**_uniform(wrt=("theta", "log_sigma", "log_obs_var")))


def test_docstrings_name_the_two_directions():
    for fn in list(JVP.values()) + list(GRID_GRAD.values()) + list(GRAD.values()):
        assert "log_sigma" in fn.__doc__ and "log_obs_var" in fn.__doc__, fn.__name__
    assert "e^{2c}" in dmod.dalton_grid_jvp.__doc__                              # what a prior_at that is no scale family gets


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("who", sorted(JVP))
@pytest.mark.parametrize("tangents,word", [
    (dict(log_sigma=np.ones((1, 3))), "shape"), (dict(log_sigma=np.ones(2)), "shape"), (dict(log_obs_var=np.ones((1, 2, 3))), "shape"),
    (dict(log_obs_var=np.ones((1, 1))), "shape"), (dict(log_sigma=np.ones((2, 1, 2))), "shape"),    # a batch axis on an unbatched call
    (dict(log_sigma=np.array([[1.0, np.nan]])), "non-finite"), (dict(log_obs_var=np.array([[np.inf, 0.0]])), "non-finite"),
    (dict(log_sigma=np.ones((2, 2)), log_obs_var=np.ones((3, 2))), "count K"), (dict(theta=np.ones((2, 3)), log_sigma=np.ones((3, 2))), "count K"),
    (dict(ode_init=np.ones((2, 2, 3)), log_obs_var=np.ones((1, 2))), "count K"), (dict(log_sigma=np.zeros((0, 2))), "K = 0"),
    (dict(log_sigma="abc"), "no array")])
def test_bad_hyper_directions_are_refused(no_device, who, tangents, word):
    with pytest.raises(ValueError, match=who + ": .*" + word):
        JVP[who](**_fhn(tangents=tangents))


@pytest.mark.parametrize("who", sorted(JVP))
def test_a_batch_axis_must_be_the_batch_s(no_device, who):
    with pytest.raises(ValueError, match="shape"):
        JVP[who](**_fhn(B=4, tangents=dict(log_sigma=np.ones((3, 1, 2)))))


@pytest.mark.parametrize("who", sorted(GRID_GRAD))
@pytest.mark.parametrize("name", HYPER)
def test_init_jac_on_a_reserved_name_is_a_value_error(no_device, who, name):
    with pytest.raises(ValueError, match=who + ": init_jac"):
        GRID_GRAD[who](**_grad(), wrt=("theta", name), init_jac={name: np.zeros((2, 3, 2))})
    with pytest.raises(ValueError, match="init_jac"):
        GRAD[who.replace("_grid", "")](**_uniform(wrt=(name,), init_jac={name: np.zeros((2, 3, 2))}))
    with pytest.raises(ValueError, match="twice"):
        GRID_GRAD[who](**_grad(), wrt=(name, name))


def _two_param(X, t, theta, log_sigma):
    return np.array([[theta[0] * X[1, 0] + log_sigma[0]], [-theta[1] * X[0, 0] * log_sigma[1] + log_sigma[2]]])


@pytest.mark.parametrize("who", sorted(JVP))
def test_a_parameter_of_that_name_wins(no_device, who, monkeypatch):
    """``log_sigma`` in ``**params`` is an ODE parameter, as it is today: its direction has the parameter's size (3), not d (2)."""
    staged = {}
    real = dmod._stage_directions

    def record(who_, ode, tangents, *rest):
        staged.update(tangents)
        return real(who_, ode, tangents, *rest)
    monkeypatch.setattr(dmod, "_stage_directions", record)
    a = _fhn(ode=_two_param, theta=np.array([1.0, 2.0]), log_sigma=np.array([0.1, 0.2, 0.3]))
    with pytest.raises(AssertionError, match="default_device was reached"):
        JVP[who](**dict(a, tangents=dict(log_sigma=np.ones((1, 3)), log_obs_var=np.ones((1, 2)))))
    assert set(staged) == {"log_sigma"}                                          # staged with the parameters; log_obs_var is the reserved one
    with pytest.raises(ValueError, match="shape"):                               # (K, d) is not that parameter's shape
        JVP[who](**dict(a, tangents=dict(log_sigma=np.ones((1, 2)))))
    assert dmod._split_hyper(dict(log_sigma=1, log_obs_var=2, theta=3), dict(log_sigma=0)) == (dict(log_sigma=1, theta=3), dict(log_obs_var=2))


@pytest.mark.parametrize("name", dmod._GRAD_NOT_WRT)
def test_every_old_name_is_still_not_built(no_device, name):
    assert name not in HYPER
    for who, fn in JVP.items():
        with pytest.raises(NotImplementedError, match=who + ": not built: a derivative with respect to"):
            fn(**_fhn(tangents={name: np.ones((1, 2))}))
        with pytest.raises(NotImplementedError, match="not built"):                 # next to a served name as well
            fn(**_fhn(tangents={"log_sigma": np.ones((1, 2)), name: np.ones((1, 2))}))
    for who, fn in GRID_GRAD.items():
        with pytest.raises(NotImplementedError, match=who + ": not built"):
            fn(**_grad(), wrt=("log_obs_var", name))
    for who, fn in GRAD.items():
        with pytest.raises(NotImplementedError, match=who + ": not built"):
            fn(**_uniform(wrt=(name,)))


def test_what_the_plain_calls_refuse_is_refused_with_the_two_names(no_device):
    for who, fn in JVP.items():
        with pytest.raises(NotImplementedError, match=who + ": not built"):
            fn(**_fhn(p=4))
        with pytest.raises(NotImplementedError, match=who + ": not built"):
            fn(**_fhn(kalman_type="square-root"))
        with pytest.raises(ValueError, match="no parameter"):
            fn(**_fhn(tangents=dict(log_sigma=np.ones((1, 2)), log_noise=np.ones((1, 2)))))
        with pytest.raises(ValueError, match="0.2 is no node"):
            fn(**_fhn(times=(0.1, 0.2)))


def test_an_empty_observation_set_returns_zeros_without_a_launch(no_device):
    for fn in JVP.values():
        value, dvalue = fn(**_fhn(times=(), tangents=dict(log_sigma=np.ones((4, 2)), log_obs_var=np.ones((4, 2)))))
        assert value == 0.0 and dvalue.shape == (4,) and np.all(dvalue == 0.0)
    for fn in GRID_GRAD.values():
        res = fn(**_grad(times=(), B=5), wrt=("theta", "log_sigma", "log_obs_var"))
        assert res.grad["theta"].shape == (5, 3) and res.grad["log_sigma"].shape == (5, 2) and res.grad["log_obs_var"].shape == (5, 2)


# ---- staging --------------------------------------------------------------------------------------------------------------------
def test_hyper_directions_are_staged_batch_minor():
    B, d = 4, 2
    rng = np.random.default_rng(0)
    ls, lo = rng.standard_normal((5, d)), rng.standard_normal((B, 5, d))
    K, dls, dls_b, dlo, dlo_b = dmod._stage_hyper("t", dict(log_sigma=ls, log_obs_var=lo), B, True, d, 5)
    assert (K, dls_b, dlo_b) == (5, 0, 1) and dls.shape == (5, d) and dlo.shape == (5, d, B) and dlo.flags.c_contiguous
    np.testing.assert_array_equal(dls, ls)
    for b in range(B):
        np.testing.assert_array_equal(dlo[..., b], lo[b])
    K, dls, dls_b, dlo, dlo_b = dmod._stage_hyper("t", dict(log_obs_var=ls), B, True, d, None)       # a missing key: no array at all
    assert K == 5 and dls is None and dls_b == 0 and dlo.shape == (5, d) and dlo_b == 0
    ode = ra.ode.fitzhugh_nagumo
    out = dmod._stage_all("t", ode, dict(theta=np.ones((5, 3)), log_sigma=ls), {"theta": 0}, B, True, d, 3)
    assert out[0] == 5 and out[1].shape == (5, 3) and out[3] is None and out[5][0].shape == (5, d) and out[5][2] is None
    out = dmod._stage_all("t", ode, dict(theta=np.ones((5, 3))), {"theta": 0}, B, True, d, 3)
    assert out[:5] == dmod._stage_directions("t", ode, dict(theta=np.ones((5, 3))), B, True, d, 3)[:1] + out[1:5] and out[5] is None
    out = dmod._stage_all("t", ode, dict(log_sigma=ls), {"theta": 0}, B, True, d, 3)                  # the two names alone
    assert out[:5] == (5, None, 0, None, 0)


def test_unit_directions_of_the_two_names():
    a = _grad()
    tangents, layout = dmod._unit_directions("t", a["ode_fun"], a["ode_weight"], a["ode_init"], ("theta", "log_sigma", "log_obs_var"),
                                             None, dict(theta=a["theta"]))
    assert [(n, k, s) for n, k, s in layout] == [("theta", 0, (3,)), ("log_sigma", 3, (2,)), ("log_obs_var", 5, (2,))]
    np.testing.assert_array_equal(tangents["log_sigma"], np.concatenate([np.zeros((3, 2)), np.eye(2), np.zeros((2, 2))]))
    np.testing.assert_array_equal(tangents["log_obs_var"], np.concatenate([np.zeros((5, 2)), np.eye(2)]))
    assert set(tangents) == {"theta", "log_sigma", "log_obs_var"}                # no ode_init direction was made up


class _Arr:
    ptr = None

    def __init__(self, shape):
        self.shape = tuple(shape)

    def to_host(self):
        return np.zeros(self.shape)


class _Plan:
    """What the two ``_jvp`` touch of a SolvePlan, recording it; the library (no device needed for the size query) is the real one."""

    def __init__(self, B, N, d, p):
        self.B, self.log = B, []
        self.cfg = _lib.SolveCfg(n_traj=B, n_steps=N, n_block=d, n_bstate=p, n_bmeas=1, rhs_id=_lib.RHS_FITZHUGH_NAGUMO,
                                 interrogate=_lib.INTERROGATE_KRAMER, kalman_type=_lib.KALMAN_STANDARD, n_theta=3,
                                 flags=_lib.FLAG_BATCH_MINOR, t_min=0.0, t_max=1.0, seed=0, traj_offset=0)
        self.inp = _lib.SolveIn() if hasattr(_lib, "SolveIn") else None
        self.dev = self
        self.h = None
        self.lib = self
        self.real = _lib.load()

    def __getattr__(self, name):                                     # a library entry: recorded, not called
        if name.startswith("rk_dalton_grid_jvp"):
            def entry(*args):
                self.log.append(("call", name, len(args)) + tuple(args[10:len(args) - 2]))
                return _lib.RK_OK
            return entry
        return getattr(self.real, name)

    def empty(self, shape):
        return _Arr(shape)

    def staged(self, slot, *arrays):
        self.log.append(("staged", slot) + tuple(np.shape(a) for a in arrays))
        return tuple(_Arr(np.shape(a)) for a in arrays)

    def set_seed(self, key):
        pass

    def launch(self, fn, key, mode, *extra):
        self.log.append(("launch", fn.__name__, len(extra)) + tuple(extra[7:len(extra) - 3]))

    def sync(self):
        pass


def _recorded(monkeypatch, mod, B, budget=None, **over):
    a = _fhn(B=B, **over)
    plan = _Plan(1 if B is None else B, 4, 2, 3)
    monkeypatch.setattr(mod, "_grid_plan", lambda *args: (plan, _lib.GridIn(), (None,) * 4 + (len(args[-2]), args[-1])))
    if budget is not None:
        monkeypatch.setattr(fmod, "_GRAD_WORKSPACE_BYTES", budget)
    (dmod.dalton_grid_jvp if mod is dmod else fmod.fenrir_grid_jvp)(**a)
    return plan.log


@pytest.mark.parametrize("mod,word", [(dmod, "call"), (fmod, "launch")])
def test_the_hyper_entry_is_called_only_with_a_reserved_name(no_device, monkeypatch, mod, word):
    """(K, dtheta, its flag, dinit, its flag[, dlog_sigma, its flag, dlog_obs_var, its flag]) as the entries receive them."""
    family = "dalton" if mod is dmod else "fenrir"
    log = _recorded(monkeypatch, mod, 4, tangents=dict(theta=np.ones((5, 3)), ode_init=np.ones((4, 5, 2, 3))))
    assert [e[1:] for e in log if e[0] == word] == [(f"rk_{family}_grid_jvp", 17 if mod is dmod else 15, 5, None, 0, None, 1)]
    assert not any("hyper" in str(e[1]) for e in log)
    log = _recorded(monkeypatch, mod, 4, tangents=dict(theta=np.ones((5, 3)), log_sigma=np.ones((4, 5, 2)), log_obs_var=np.ones((5, 2))))
    assert [e[1:] for e in log if e[0] == word] == [(f"rk_{family}_grid_jvp_hyper", 21 if mod is dmod else 19, 5, None, 0, None, 0,
                                                    None, 1, None, 0)]
    slot = "dalton_grad_hyper" if mod is dmod else ("fenrir_grad_hyper", 0)
    assert ("staged", slot, (5, 2, 4), (5, 2)) in log
    log = _recorded(monkeypatch, mod, None, tangents=dict(log_obs_var=np.ones((2, 2))))              # a missing name: no array
    assert ("staged", slot, (1,), (2, 2)) in log


@pytest.mark.parametrize("budget,counts", [(2 * 960, [2, 2, 1]), (100, [1] * 5), (5 * 960, [5])])
def test_fenrir_s_chunks_slice_the_hyper_directions_with_the_others(no_device, monkeypatch, budget, counts):
    """B = 1, N = 4, d = 2, p = 3: 960 bytes of tangent records per direction; K = 5."""
    log = _recorded(monkeypatch, fmod, None, budget=budget,
                    tangents=dict(theta=np.ones((5, 3)), log_sigma=np.ones((5, 2)), log_obs_var=np.ones((5, 2))))
    assert [e[3] for e in log if e[0] == "launch"] == counts
    assert [e for e in log if e[0] == "staged" and e[1][0] == "fenrir_grad_hyper"] == \
        [("staged", ("fenrir_grad_hyper", ci), (k, 2), (k, 2)) for ci, k in enumerate(counts)]
    assert [e[2] for e in log if e[0] == "staged" and e[1][0] == "fenrir_grad"] == [(k, 3) for k in counts]


# ---- the library, on the configuration alone -------------------------------------------------------------------------------
def _cfg(rhs=_lib.RHS_FITZHUGH_NAGUMO, d=2, p=3, m=1, itg=_lib.INTERROGATE_KRAMER, kalman=_lib.KALMAN_STANDARD, flags=_lib.FLAG_BATCH_MINOR):
    return _lib.SolveCfg(n_traj=16, n_steps=50, n_block=d, n_bstate=p, n_bmeas=m, rhs_id=rhs, interrogate=itg, kalman_type=kalman,
                         n_theta=3, flags=flags, t_min=0.0, t_max=1.0, seed=0, traj_offset=0)


def _hyper(family, cfg, n_bobs=1, n_dir=1):
    """The hyper entry with no handle and no pointers: only the configuration, n_bobs and n_dir can be looked at."""
    lib = _lib.load()
    if family == "dalton":
        rc = lib.rk_dalton_grid_jvp_hyper(None, C.byref(cfg), None, None, None, None, None, 1, n_bobs, None, n_dir, None, 0, None, 0,
                                          None, 0, None, 0, None, None)
    else:
        rc = lib.rk_fenrir_grid_jvp_hyper(None, C.byref(cfg), None, None, None, None, None, None, 1, n_bobs, None, n_dir, None, 0, None, 0,
                                          None, 0, None, 0, None, None, None)
    return rc, lib.rk_last_error().decode()


@pytest.mark.parametrize("family", ["dalton", "fenrir"])
@pytest.mark.parametrize("cfg,n_bobs", [
    (_cfg(kalman=_lib.KALMAN_SQRT), 1), (_cfg(itg=_lib.INTERROGATE_CHKREBTII), 1), (_cfg(m=2), 1), (_cfg(), 2), (_cfg(), 3),
    (_cfg(p=4), 1), (_cfg(p=6), 1), (_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=4), 1), (_cfg(rhs=_lib.RHS_HIGHER_ORDER, d=1), 1)])
def test_library_says_not_built(family, cfg, n_bobs):
    rc, msg = _hyper(family, cfg, n_bobs)
    assert rc == _lib.RK_ERR_UNSUPPORTED and family + "_grid_jvp" in msg and "not built" in msg, (rc, msg)


@pytest.mark.parametrize("family", ["dalton", "fenrir"])
def test_library_calls_bad_sizes_invalid_and_passes_every_instance_that_ships_on(family):
    for cfg, n_dir, word in ((_cfg(), 0, "n_dir"), (_cfg(flags=0), 1, "RK_FLAG_BATCH_MINOR"), (_cfg(p=0), 1, "non-positive")):
        rc, msg = _hyper(family, cfg, 1, n_dir)
        assert rc == _lib.RK_ERR_INVALID and word in msg, (rc, msg)
    for rhs, d in ((_lib.RHS_FITZHUGH_NAGUMO, 2), (_lib.RHS_LORENZ63, 3)):       # all twelve: none is left out
        for p in (2, 3):
            for itg in (_lib.INTERROGATE_RODEO, _lib.INTERROGATE_SCHOBER, _lib.INTERROGATE_KRAMER):
                rc, msg = _hyper(family, _cfg(rhs=rhs, d=d, p=p, itg=itg), 1, 5)
                assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)


# ---- the tracer and hiprtc ------------------------------------------------------------------------------------------------------
def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


def _forced(X, t, theta):
    return np.array([np.sin(theta[0] * t) * X[1, 0] - np.exp(-X[0, 0]) / theta[1], np.tanh(X[0, 0] * X[1, 0]) + X[1, 1] ** 2])


def test_a_traced_function_is_served_with_the_two_names(no_device):
    for fn in JVP.values():
        with pytest.raises(AssertionError, match="default_device was reached"):
            fn(**_fhn(ode=_fitz))
        with pytest.raises(AssertionError, match="default_device was reached"):
            fn(**_fhn(ode=from_python(_fitz, 2, 3, theta=3), tangents=dict(theta=np.eye(3), log_obs_var=np.ones((3, 2)))))
    g = grad_from_python(_fitz, 2, 3, theta=3)
    for family in ("dalton", "fenrir"):
        rc, msg = _hyper(family, _cfg(rhs=g.rhs_id))
        assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
        for cfg, word in ((_cfg(rhs=g.rhs_id, p=4), "not built"), (_cfg(rhs=g.rhs_id, d=3), "n_block")):
            rc, msg = _hyper(family, cfg)
            assert rc == _lib.RK_ERR_UNSUPPORTED and word in msg, (rc, msg)


def test_both_hyper_kinds_build_with_hiprtc_without_a_device():
    lib = _lib.load()
    g = grad_from_python(_forced, 2, 3, theta=2)
    for check in (lib.rk_dalton_grad_hyper_compile_check, lib.rk_fenrir_grad_hyper_compile_check):
        for p, itg in ((3, _lib.INTERROGATE_RODEO), (3, _lib.INTERROGATE_KRAMER), (2, _lib.INTERROGATE_SCHOBER)):
            assert check(g.rhs_id, p, itg) == _lib.RK_OK, lib.rk_last_error().decode()
        assert check(_lib.RHS_USER_BASE + 100000, 3, _lib.INTERROGATE_KRAMER) == _lib.RK_ERR_INVALID
        plain = from_python(_forced, 2, 3, theta=2)                              # the solver's kind has no rhs_generic: a clean failure
        assert check(plain.rhs_id, 3, _lib.INTERROGATE_KRAMER) == _lib.RK_ERR_INVALID
        assert "hiprtc could not compile" in lib.rk_last_error().decode()
    assert lib.rk_fenrir_grad_hyper_compile_check(_lib.RHS_LORENZ63, 3, _lib.INTERROGATE_RODEO) == _lib.RK_OK   # the header is RTC-safe


def test_the_tracer_emits_what_it_did():
    """The hashes tests/test_dalton_grad_host.py holds for the solver's emitter, and the gradient kind's text against it."""
    src, ndep, n_bmeas = trace_source(_fitz, 2, 3, (("theta", 3),), "Traced_fixed")
    assert (ndep, n_bmeas) == (1, 1)
    assert hashlib.sha1(src.encode()).hexdigest() == "3387d242e9cb5bbeedd83706c85679a9df15b264"
    gsrc, ndep = trace_grad_source(_fitz, 2, 3, (("theta", 3),), "G")
    assert ndep == 1 and "log_sigma" not in gsrc and "template <class T, class TH, int P>" in gsrc
    body = [ln for ln in trace_source(_fitz, 2, 3, (("theta", 3),), "G")[0].splitlines() if ln.strip().startswith("out[")]
    assert body and all(ln in gsrc for ln in body)


# ---- laplace.pull_back --------------------------------------------------------------------------------------------------------
def test_pull_back_treats_the_two_names_like_any_other():
    rng = np.random.default_rng(1)
    B, n = 3, 7
    grad = dict(theta=rng.standard_normal((B, 3)), log_sigma=rng.standard_normal((B, 2)), log_obs_var=rng.standard_normal((B, 2)))
    jac = dict(theta=rng.standard_normal((B, 3, n)), log_sigma=rng.standard_normal((B, 2, n)), log_obs_var=rng.standard_normal((B, 2, n)))
    out = laplace.pull_back(grad, jac)
    want = sum(np.einsum("bi,bij->bj", grad[k], jac[k]) for k in grad)
    assert out.shape == (B, n)
    np.testing.assert_allclose(out, want, rtol=1e-13, atol=1e-13)
