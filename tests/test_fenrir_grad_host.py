"""
``fenrir_grid_jvp`` / ``fenrir_grid_grad`` / ``fenrir_grad`` on the host (no GPU): the signatures, every refusal that comes before any
device work (``default_device`` patched to fail), the empty observation set, the staging shapes, the chunking of the directions
under a patched ``_GRAD_WORKSPACE_BYTES`` (on a recording stand-in for the plan), the library's refusals on the configuration
alone, the hiprtc build of the forward kernel without a device, and ``dalton``'s own gradient messages, which stay what they were.
"""
import ctypes as C
import functools
import inspect
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401
import rodeo_amd.inference.fenrir  # noqa: F401
from rodeo_amd import _lib
from rodeo_amd.interrogate import interrogate_chkrebtii, interrogate_kramer
from rodeo_amd.ode import from_source
from rodeo_amd.trace import from_python, grad_from_python

dmod = sys.modules["rodeo_amd.inference.dalton"]             # (rodeo_amd.inference.dalton, the attribute, is the function)
fmod = sys.modules["rodeo_amd.inference.fenrir"]


def _fhn(p=3, n_bobs=1, times=(0.1, 0.3), B=None, ode=ra.ode.fitzhugh_nagumo, **over):
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    theta = np.array([0.2, 0.2, 3.0]) if B is None else np.array([0.2, 0.2, 3.0]) * (1 + 0.01 * np.arange(B)[:, None])
    sigma = np.array([0.5, 0.3])
    n = len(times)
    D = np.zeros((n, 2, n_bobs, p))
    D[..., 0, 0] = 1.0
    a = dict(key=None, ode_fun=ode, ode_weight=W, ode_init=init(np.array([-1.0, 1.0]), 0.0, theta=theta),
             t_grid=np.array([0.0, 0.1, 0.15, 0.3, 0.4]), interrogate=interrogate_kramer, prior_at=lambda h: ra.ibm_init(h, p, sigma),
             obs_data=np.zeros((n, 2, n_bobs)), obs_times=np.array(times, dtype=float), obs_weight=D,
             obs_var=np.tile(0.01 * np.eye(n_bobs), (n, 2, 1, 1)), tangents=dict(theta=np.eye(3)), theta=theta)
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


# ---- the interface ------------------------------------------------------------------------------------------------------------
def test_names_signatures_and_docstrings():
    for name in ("fenrir_grid_jvp", "fenrir_grid_grad", "fenrir_grad", "FenrirGrad"):
        assert hasattr(fmod, name) and not hasattr(ra.inference, name)                      # not re-exported
    assert fmod.FenrirGrad._fields == dmod.DaltonGrad._fields == ("value", "grad")
    for ours, theirs in ((fmod.fenrir_grid_jvp, dmod.dalton_grid_jvp), (fmod.fenrir_grid_grad, dmod.dalton_grid_grad),
                         (fmod.fenrir_grad, dmod.dalton_grad)):
        assert str(inspect.signature(ours)) == str(inspect.signature(theirs))
    assert list(inspect.signature(fmod.fenrir_grid_jvp).parameters)[:11] == list(inspect.signature(fmod.fenrir_grid).parameters)[:11]
    assert list(inspect.signature(fmod.fenrir_grad).parameters)[:13] == list(inspect.signature(fmod.fenrir).parameters)[:13]
    assert "1e-8" in fmod.fenrir_grid_jvp.__doc__ and "contributes nothing" in fmod.fenrir_grid_jvp.__doc__
    assert "NOT bit for bit" in fmod.fenrir_grad.__doc__ and "cross-route bar" in fmod.fenrir_grad.__doc__
    assert fmod._GRAD_WORKSPACE_BYTES == 2 ** 32


def test_a_served_call_reaches_the_device(no_device):
    """(the fixture works: what is not refused does ask for a device)"""
    with pytest.raises(AssertionError, match="default_device was reached"):
        fmod.fenrir_grid_jvp(**_fhn())
    with pytest.raises(AssertionError, match="default_device was reached"):
        fmod.fenrir_grid_grad(**_grad(), wrt=("theta", "ode_init"))
    with pytest.raises(AssertionError, match="default_device was reached"):
        fmod.fenrir_grid_jvp(**_fhn(p=2, tangents=dict(ode_init=np.ones((1, 2, 2)))))
    with pytest.raises(AssertionError, match="default_device was reached"):
        fmod.fenrir_grad(**_uniform())


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", [
    dict(kalman_type="square-root"), dict(interrogate=functools.partial(interrogate_chkrebtii, kalman_type="standard")),
    dict(n_bobs=2), dict(n_bobs=3), dict(ode_weight=np.zeros((2, 2, 3))), dict(p=4), dict(p=5), dict(p=6),
    dict(ode=ra.ode.higher_order), dict(tangents=dict(sigma=np.ones((1, 2)))), dict(tangents=dict(ode_weight=np.ones((1, 2)))),
    dict(tangents=dict(obs_data=np.ones((1, 2)))), dict(tangents=dict(prior_pars=np.ones((1, 2)))),
    dict(tangents=dict(prior_at=np.ones((1, 2)))), dict(tangents=dict(t_grid=np.ones((1, 2)))),
    dict(tangents=dict(obs_times=np.ones((1, 2)))), dict(tangents=dict(obs_var=np.ones((1, 2))))],
    ids=["square-root", "chkrebtii", "n_bobs=2", "n_bobs=3", "n_bmeas=2", "p=4", "p=5", "p=6", "higher_order", "d/dsigma",
         "d/dode_weight", "d/ddata", "d/dprior_pars", "d/dprior_at", "d/dt_grid", "d/dobs_times", "d/dobs_var"])
def test_what_is_not_built_is_refused_before_any_device_work(no_device, over):
    with pytest.raises(NotImplementedError, match="fenrir_grid_jvp: not built"):
        fmod.fenrir_grid_jvp(**_fhn(**over))
    if "tangents" not in over:
        with pytest.raises(NotImplementedError, match="fenrir_grid_grad: not built"):
            fmod.fenrir_grid_grad(**_grad(**over))
        if set(over) <= {"kalman_type", "interrogate"}:
            with pytest.raises(NotImplementedError, match="fenrir_grad: not built"):
                fmod.fenrir_grad(**_uniform(**over))
    else:
        with pytest.raises(NotImplementedError, match="fenrir_grid_grad: not built"):
            fmod.fenrir_grid_grad(**_grad(), wrt=tuple(over["tangents"]))
        with pytest.raises(NotImplementedError, match="fenrir_grad: not built"):
            fmod.fenrir_grad(**_uniform(), wrt=tuple(over["tangents"]))


def test_a_source_right_hand_side_of_the_solver_s_kind_is_refused(no_device):
    src = ("struct HostSrc { static constexpr int D = 2, NTHETA = 3, NDEP = 1; template <class T, int P> __device__ static void "
           "rhs(const T (&X)[D][P], double t, const double (&th)[NTHETA], T (&out)[D]) { out[0] = X[1][0]; out[1] = X[0][0]; } };")
    ode = from_source("HostSrc", src, 2, (("theta", 3),))
    with pytest.raises(NotImplementedError, match="not built"):
        fmod.fenrir_grid_jvp(**_fhn(ode=ode))


def test_lorenz_at_four_is_refused(no_device):
    W, init = ra.utils.first_order_pad(ra.ode.lorenz63, 3, 4)
    theta = np.array([28.0, 10.0, 8.0 / 3.0])
    D = np.zeros((1, 3, 1, 4))
    D[..., 0] = 1.0
    with pytest.raises(NotImplementedError, match="not built"):
        fmod.fenrir_grid_jvp(None, ra.ode.lorenz63, W, init(np.array([-12.0, -5.0, 38.0]), 0.0, theta=theta), [0.0, 0.1, 0.2],
                             interrogate_kramer, lambda h: ra.ibm_init(h, 4, np.ones(3)), np.zeros((1, 3, 1)), [0.1], D,
                             np.ones((1, 3, 1, 1)), dict(theta=np.eye(3)), theta=theta)


def test_the_size_message_names_fenrir_grid_and_dalton_s_stays(no_device):
    with pytest.raises(NotImplementedError) as e:
        fmod.fenrir_grid_jvp(**_fhn(p=4))
    assert str(e.value) == "fenrir_grid_jvp: not built: n_bstate = 4 (2 .. 3: beyond, the kernel needs more scratch than fenrir_grid's)"
    with pytest.raises(NotImplementedError) as e:
        dmod.dalton_grid_jvp(**_fhn(p=4))
    assert str(e.value) == "dalton_grid_jvp: not built: n_bstate = 4 (2 .. 3: beyond, the kernel needs more scratch than dalton_grid's)"
    with pytest.raises(NotImplementedError) as e:
        dmod.dalton_grid_grad(**_grad(kalman_type="square-root"))
    assert str(e.value) == "dalton_grid_grad: not built: kalman_type 'square-root' (the standard form only)"
    with pytest.raises(NotImplementedError) as e:
        dmod.dalton_grid_jvp(**_fhn(tangents=dict(sigma=np.ones((1, 2)))))
    assert str(e.value) == "dalton_grid_jvp: not built: a derivative with respect to 'sigma' (the ODE parameters and 'ode_init' only)"
    with pytest.raises(ValueError) as e:
        dmod.dalton_grid_jvp(**_fhn(tangents={}))
    assert str(e.value) == "dalton_grid_jvp: no direction given (K = 0)"


@pytest.mark.parametrize("tangents,word", [
    (dict(phi=np.ones((1, 3))), "no parameter"), ({}, "K = 0"), (dict(theta=np.zeros((0, 3))), "K = 0"),
    (dict(theta=np.ones((1, 4))), "shape"), (dict(theta=np.ones(3)), "shape"), (dict(ode_init=np.ones((1, 2, 4))), "shape"),
    (dict(ode_init=np.ones((2, 3))), "shape"), (dict(theta=np.ones((2, 1, 3))), "shape"),      # a batch axis on an unbatched call
    (dict(theta=np.array([[1.0, np.nan, 0.0]])), "non-finite"), (dict(ode_init=np.full((1, 2, 3), np.inf)), "non-finite"),
    (dict(theta=np.ones((2, 3)), ode_init=np.ones((3, 2, 3))), "count K"), (dict(theta="abc"), "no array"), ([1.0], "dict")])
def test_bad_directions_are_refused(no_device, tangents, word):
    with pytest.raises(ValueError, match="fenrir_grid_jvp: .*" + word):
        fmod.fenrir_grid_jvp(**_fhn(tangents=tangents))


def test_bad_wrt_and_init_jac_are_refused(no_device):
    with pytest.raises(ValueError, match="no parameter"):
        fmod.fenrir_grid_grad(**_grad(), wrt=("phi",))
    with pytest.raises(ValueError, match="K = 0"):
        fmod.fenrir_grid_grad(**_grad(), wrt=())
    with pytest.raises(ValueError, match="twice"):
        fmod.fenrir_grid_grad(**_grad(), wrt=("theta", "theta"))
    with pytest.raises(ValueError, match="fenrir_grid_grad: init_jac"):
        fmod.fenrir_grid_grad(**_grad(), wrt=("ode_init",), init_jac=dict(theta=np.zeros((2, 3, 3))))
    with pytest.raises(ValueError, match="shape"):
        fmod.fenrir_grid_grad(**_grad(), wrt=("theta",), init_jac=dict(theta=np.zeros((2, 3, 2))))
    with pytest.raises(ValueError, match="shape"):                               # a batched Jacobian on an unbatched call
        fmod.fenrir_grid_grad(**_grad(), wrt=("theta",), init_jac=dict(theta=np.zeros((4, 2, 3, 3))))


def test_what_fenrir_grid_refuses_is_refused_in_its_order(no_device):
    for times, word in (((0.1, 0.2), "0.2 is no node"), ((0.3, 0.1), "strictly increasing"), ((0.1, np.nan), "non-finite")):
        with pytest.raises(ValueError, match=word):
            fmod.fenrir_grid_jvp(**_fhn(times=times))
    with pytest.raises(ValueError, match="strictly increasing"):
        fmod.fenrir_grid_jvp(**_fhn(t_grid=[0.0, 0.5, 0.5]))
    with pytest.raises(ValueError, match="callable"):
        fmod.fenrir_grid_jvp(**_fhn(prior_at=1.0))
    with pytest.raises(ValueError, match="obs_weight"):
        fmod.fenrir_grid_jvp(**_fhn(obs_weight=np.zeros((2, 2, 1, 4))))
    # a doubly wrong call gets the refusal fenrir_grid gives it: the observation shapes, then the nodes, then the grid
    for over in (dict(obs_data=np.zeros((3, 2, 1)), times=(0.1, 0.2)), dict(times=(0.1, 0.2), t_grid=[0.0, 0.5, 0.5]),
                 dict(times=(0.1, 0.2), prior_at=1.0)):
        a = _fhn(**over)
        with pytest.raises(ValueError) as ours:
            fmod.fenrir_grid_jvp(**a)
        a.pop("tangents")
        with pytest.raises(ValueError) as theirs:
            fmod.fenrir_grid(**a)
        assert str(ours.value).replace("fenrir_grid_jvp", "fenrir_grid") == str(theirs.value)


def test_fenrir_grad_refuses_like_the_grid_calls(no_device):
    with pytest.raises(NotImplementedError, match="not built"):
        fmod.fenrir_grad(**_uniform(kalman_type="square-root"))
    with pytest.raises(ValueError, match="no parameter"):
        fmod.fenrir_grad(**_uniform(wrt=("phi",)))
    with pytest.raises(ValueError, match="ascending"):                           # fenrir's own message
        fmod.fenrir_grad(**_uniform(obs_times=np.array([0.3, 0.1])))
    with pytest.raises(ValueError, match="strictly increasing"):                 # two times on one node
        fmod.fenrir_grad(**_uniform(obs_times=np.array([0.25, 0.3])))
    with pytest.raises(ValueError, match="strictly increasing"):                 # t_max and a time past it: both are node N
        fmod.fenrir_grad(**_uniform(obs_times=np.array([0.4, 0.45])))
    with pytest.raises(AssertionError, match="default_device was reached"):      # a last time past t_max alone is node N: served
        fmod.fenrir_grad(**_uniform(obs_times=np.array([0.1, 0.45])))


def test_an_empty_observation_set_returns_zeros_without_a_launch_or_a_plan(no_device, monkeypatch):
    def fail(*a, **k):
        raise AssertionError("a plan was asked for")
    monkeypatch.setattr(fmod, "_grid_plan", fail)
    value, dvalue = fmod.fenrir_grid_jvp(**_fhn(times=(), tangents=dict(theta=np.ones((4, 3)))))
    assert value == 0.0 and isinstance(value, float) and dvalue.shape == (4,) and np.all(dvalue == 0.0)
    value, dvalue = fmod.fenrir_grid_jvp(**_fhn(times=(), B=5, tangents=dict(ode_init=np.ones((5, 2, 2, 3)))))
    assert value.shape == (5,) and dvalue.shape == (5, 2) and np.all(value == 0.0) and np.all(dvalue == 0.0)
    res = fmod.fenrir_grid_grad(**_grad(times=(), B=5), wrt=("theta", "ode_init"))
    assert isinstance(res, fmod.FenrirGrad)
    assert np.all(res.value == 0.0) and res.grad["theta"].shape == (5, 3) and res.grad["ode_init"].shape == (5, 2, 3)
    with pytest.raises(ValueError, match="K = 0"):                                # the refusals still come first
        fmod.fenrir_grid_jvp(**_fhn(times=(), tangents={}))


# ---- staging and chunks: a recording stand-in for the plan -------------------------------------------------------------------
class _Arr:
    ptr = None

    def __init__(self, shape):
        self.shape = tuple(shape)

    def to_host(self):
        return np.zeros(self.shape)


class _Plan:
    """What ``_jvp`` touches of a SolvePlan, recording it; the library (no device needed for the size query) is the real one."""

    def __init__(self, B, N, d, p):
        self.B, self.log = B, []
        self.cfg = _lib.SolveCfg(n_traj=B, n_steps=N, n_block=d, n_bstate=p, n_bmeas=1, rhs_id=_lib.RHS_FITZHUGH_NAGUMO,
                                 interrogate=_lib.INTERROGATE_KRAMER, kalman_type=_lib.KALMAN_STANDARD, n_theta=3,
                                 flags=_lib.FLAG_BATCH_MINOR, t_min=0.0, t_max=1.0, seed=0, traj_offset=0)
        self.dev = self
        self.lib = _lib.load()

    def empty(self, shape):
        self.log.append(("empty", tuple(shape)))
        return _Arr(shape)

    def staged(self, slot, *arrays):
        self.log.append(("staged", slot) + tuple(np.shape(a) for a in arrays))
        return tuple(_Arr(np.shape(a)) for a in arrays)

    def launch(self, fn, key, mode, *extra):
        self.log.append(("launch", fn.__name__, mode, extra[4], extra[5], extra[7], extra[9], extra[11]))   # n_obs, n_bobs, K, flags

    def sync(self):
        self.log.append(("sync",))


def _recorded(monkeypatch, B, budget=None, **over):
    a = _fhn(B=B, **over)
    plan = _Plan(1 if B is None else B, 4, 2, 3)
    monkeypatch.setattr(fmod, "_grid_plan", lambda *args: (plan, _lib.GridIn(), (None,) * 4 + (len(args[-2]), args[-1])))
    if budget is not None:
        monkeypatch.setattr(fmod, "_GRAD_WORKSPACE_BYTES", budget)
    value, dvalue = fmod.fenrir_grid_jvp(**a)
    return plan.log, value, dvalue


def test_workspace_bytes_are_the_tangent_records():
    lib = _lib.load()
    need = C.c_size_t(0)
    cfg = _Plan(1024, 4000, 2, 3).cfg
    assert lib.rk_fenrir_grid_jvp_workspace_bytes(C.byref(cfg), 5, C.byref(need)) == _lib.RK_OK
    assert need.value == 4001 * 2 * (3 + 9) * 1024 * 5 * 8                       # 3.9 GB on the headline shape at K = 5
    assert lib.rk_fenrir_grid_jvp_workspace_bytes(C.byref(cfg), 0, C.byref(need)) == _lib.RK_ERR_INVALID


def test_staging_shapes_and_one_launch_by_default(no_device, monkeypatch):
    rng = np.random.default_rng(0)
    log, value, dvalue = _recorded(monkeypatch, 4, tangents=dict(theta=rng.standard_normal((4, 5, 3)), ode_init=rng.standard_normal((5, 2, 3))))
    per_dir = 5 * 2 * 12 * 4                                                      # doubles
    assert ("empty", (5 * per_dir,)) in log
    assert [e for e in log if e[0] == "staged"] == [("staged", ("fenrir_grad", 0), (5, 3, 4), (5, 2, 3))]
    launches = [e for e in log if e[0] == "launch"]
    assert launches == [("launch", "rk_fenrir_grid_jvp", _lib.MODE_FILTER, 2, 1, 5, 1, 0)]
    assert log[-1] == ("sync",) and value.shape == (4,) and dvalue.shape == (4, 5)
    log, value, dvalue = _recorded(monkeypatch, None, tangents=dict(ode_init=np.ones((2, 2, 3))))     # no theta direction: no array
    assert [e for e in log if e[0] == "staged"] == [("staged", ("fenrir_grad", 0), (1,), (2, 2, 3))]
    assert isinstance(value, float) and dvalue.shape == (2,)


@pytest.mark.parametrize("budget,counts", [(2 * 960, [2, 2, 1]), (3 * 960 - 1, [2, 2, 1]), (100, [1] * 5), (5 * 960, [5]), (4 * 960, [4, 1])])
def test_the_directions_run_in_chunks_that_fit_the_budget(no_device, monkeypatch, budget, counts):
    """B = 1, N = 4, d = 2, p = 3: 960 bytes of tangent records per direction; K = 5."""
    log, _, dvalue = _recorded(monkeypatch, None, budget=budget, tangents=dict(theta=np.ones((5, 3)), ode_init=np.ones((5, 2, 3))))
    assert [e[5] for e in log if e[0] == "launch"] == counts
    assert [e[2:] for e in log if e[0] == "staged"] == [((k, 3), (k, 2, 3)) for k in counts]
    assert ("empty", (counts[0] * 120,)) in log and dvalue.shape == (5,)         # one workspace, the first chunk's size


# ---- the library, on the configuration alone -------------------------------------------------------------------------------
def _cfg(rhs=_lib.RHS_FITZHUGH_NAGUMO, d=2, p=3, m=1, itg=_lib.INTERROGATE_KRAMER, kalman=_lib.KALMAN_STANDARD, flags=_lib.FLAG_BATCH_MINOR):
    return _lib.SolveCfg(n_traj=16, n_steps=50, n_block=d, n_bstate=p, n_bmeas=m, rhs_id=rhs, interrogate=itg, kalman_type=kalman,
                         n_theta=3, flags=flags, t_min=0.0, t_max=1.0, seed=0, traj_offset=0)


def _jvp(cfg, n_bobs=1, n_dir=1):
    """rk_fenrir_grid_jvp with no handle and no pointers: only the configuration, n_bobs and n_dir can be looked at."""
    lib = _lib.load()
    rc = lib.rk_fenrir_grid_jvp(None, C.byref(cfg), None, None, None, None, None, None, 1, n_bobs, None, n_dir, None, 0, None, 0, None,
                                None, None)
    return rc, lib.rk_last_error().decode()


@pytest.mark.parametrize("cfg,n_bobs", [
    (_cfg(kalman=_lib.KALMAN_SQRT), 1), (_cfg(itg=_lib.INTERROGATE_CHKREBTII), 1), (_cfg(m=2), 1), (_cfg(), 2), (_cfg(), 3),
    (_cfg(p=1), 1), (_cfg(p=4), 1), (_cfg(p=6), 1), (_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=4), 1), (_cfg(rhs=_lib.RHS_HIGHER_ORDER, d=1), 1)])
def test_library_says_not_built(cfg, n_bobs):
    rc, msg = _jvp(cfg, n_bobs)
    assert rc == _lib.RK_ERR_UNSUPPORTED and "fenrir_grid_jvp" in msg and "not built" in msg, (rc, msg)


def test_library_calls_bad_sizes_invalid_and_passes_a_served_configuration_on():
    for cfg, n_dir, word in ((_cfg(), 0, "n_dir"), (_cfg(flags=0), 1, "RK_FLAG_BATCH_MINOR"), (_cfg(p=0), 1, "non-positive")):
        rc, msg = _jvp(cfg, 1, n_dir)
        assert rc == _lib.RK_ERR_INVALID and word in msg and "fenrir_grid_jvp" in msg, (rc, msg)
    for cfg in (_cfg(), _cfg(p=2), _cfg(itg=_lib.INTERROGATE_RODEO), _cfg(itg=_lib.INTERROGATE_SCHOBER), _cfg(rhs=_lib.RHS_LORENZ63, d=3),
                _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=2)):
        rc, msg = _jvp(cfg, 1, 5)
        assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)


# ---- the tracer and hiprtc ------------------------------------------------------------------------------------------------------
def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


def _forced(X, t, theta):
    return np.array([np.sin(theta[0] * t) * X[1, 0] - np.exp(-X[0, 0]) / theta[1], np.tanh(X[0, 0] * X[1, 0]) + X[1, 1] ** 2])


def test_a_traced_function_is_served_through_the_gradient_kind(no_device):
    with pytest.raises(AssertionError, match="default_device was reached"):
        fmod.fenrir_grid_jvp(**_fhn(ode=_fitz))
    with pytest.raises(AssertionError, match="default_device was reached"):
        fmod.fenrir_grid_jvp(**_fhn(ode=from_python(_fitz, 2, 3, theta=3)))
    g = grad_from_python(_fitz, 2, 3, theta=3)                                    # the registration DALTON's gradients use
    rc, msg = _jvp(_cfg(rhs=g.rhs_id))
    assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
    for cfg, word in ((_cfg(rhs=g.rhs_id, p=4), "not built"), (_cfg(rhs=g.rhs_id, d=3), "n_block")):
        rc, msg = _jvp(cfg)
        assert rc == _lib.RK_ERR_UNSUPPORTED and word in msg and "fenrir_grid_jvp" in msg, (rc, msg)


def test_the_forward_kernel_builds_with_hiprtc_without_a_device():
    lib = _lib.load()
    g = grad_from_python(_forced, 2, 3, theta=2)
    for p, itg in ((3, _lib.INTERROGATE_RODEO), (3, _lib.INTERROGATE_KRAMER), (2, _lib.INTERROGATE_SCHOBER)):
        assert lib.rk_fenrir_grad_compile_check(g.rhs_id, p, itg) == _lib.RK_OK, lib.rk_last_error().decode()
    for rid, p, itg in ((_lib.RHS_FITZHUGH_NAGUMO, 3, _lib.INTERROGATE_KRAMER), (_lib.RHS_LORENZ63, 2, _lib.INTERROGATE_RODEO)):
        assert lib.rk_fenrir_grad_compile_check(rid, p, itg) == _lib.RK_OK, lib.rk_last_error().decode()    # the header is RTC-safe
    assert lib.rk_fenrir_grad_compile_check(_lib.RHS_HIGHER_ORDER, 3, _lib.INTERROGATE_KRAMER) == _lib.RK_ERR_INVALID   # no rhs_generic
    assert lib.rk_fenrir_grad_compile_check(_lib.RHS_USER_BASE + 100000, 3, _lib.INTERROGATE_KRAMER) == _lib.RK_ERR_INVALID
    plain = from_python(_forced, 2, 3, theta=2)                                  # the solver's kind has no rhs_generic: a clean failure
    assert lib.rk_fenrir_grad_compile_check(plain.rhs_id, 3, _lib.INTERROGATE_KRAMER) == _lib.RK_ERR_INVALID
    assert "hiprtc could not compile" in lib.rk_last_error().decode()
