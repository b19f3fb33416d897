"""
``daltonng_grid`` / ``solve_mv_nn_grid`` (``rodeo_amd.inference.dalton``) on the host (no GPU): the signatures, every refusal that
comes before any device work (``default_device`` patched to fail), the library's refusals on the configuration alone (no handle,
no pointers), the hiprtc builds of the two new kernel kinds, and that ``daltonng`` / ``solve_mv_nn`` refuse what they refused
before their refusals were split.
"""
import ctypes as C
import functools
import inspect
import re
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401
from rodeo_amd import _lib
from rodeo_amd.interrogate import interrogate_chkrebtii, interrogate_kramer
from rodeo_amd.solve import EVAL_AT_NODE_TOL
from rodeo_amd.trace import gammaln, trace_obs_source

dmod = sys.modules["rodeo_amd.inference.dalton"]             # (rodeo_amd.inference.dalton, the attribute, is the function)
CALLS = [dmod.daltonng_grid, dmod.solve_mv_nn_grid]
ARGS = ["key", "ode_fun", "ode_weight", "ode_init", "t_grid", "interrogate", "prior_at", "obs_data", "obs_times", "obs_loglik_i",
        "kalman_type", "params"]
THETA = np.array([0.2, 0.2, 3.0])


def poisson_loglik(obs_data_i, ode_data_i, ind, **params):
    eta = 0.1 + 0.5 * ode_data_i[:, 0]
    y = obs_data_i.flatten()
    return np.sum(y * eta - np.exp(eta) - gammaln(y + 1.0))


def test_signatures_and_exports():
    for fn in CALLS:
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ARGS
        assert list(sig.parameters)[:7] == list(inspect.signature(ra.solve_mv_grid).parameters)[:7]
        assert list(sig.parameters)[7:10] == list(inspect.signature(dmod.daltonng).parameters)[9:12]
        assert sig.parameters["kalman_type"].default == "standard"
        assert sig.parameters["params"].kind is inspect.Parameter.VAR_KEYWORD
    for name in ("daltonng_grid", "solve_mv_nn_grid"):
        assert not hasattr(ra.inference, name)                            # imported from rodeo_amd.inference.dalton, not re-exported
    doc = dmod.daltonng_grid.__doc__
    assert "grid_with_times" in doc and "NO\n    OBSERVATIONS" in doc and "NaN" in doc
    assert "rodeo_amd.solve_mv_grid" in dmod.solve_mv_nn_grid.__doc__    # the empty observation set


# ---- refusals before any device work --------------------------------------------------------------------------------------
def _fhn(p=3, times=(0.1, 0.3), **over):
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    sigma = np.array([0.5, 0.3])
    a = dict(key=None, ode_fun=ra.ode.fitzhugh_nagumo, ode_weight=W, ode_init=init(np.array([-1.0, 1.0]), 0.0, theta=THETA),
             t_grid=np.array([0.0, 0.1, 0.15, 0.3, 0.4]), interrogate=interrogate_kramer, prior_at=lambda h: ra.ibm_init(h, p, sigma),
             obs_data=np.ones((len(times), 2, 1)), obs_times=np.array(times, dtype=float), obs_loglik_i=poisson_loglik, theta=THETA)
    a.update(over)
    return a


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device fails the test: the refusals below come first."""
    def fail(*a, **k):
        raise AssertionError("default_device was reached")
    monkeypatch.setattr(ra.device, "default_device", fail)
    monkeypatch.setattr(ra.solve, "default_device", fail)


@pytest.mark.parametrize("call", CALLS)
def test_a_served_call_reaches_the_device(no_device, call):
    """(the fixture works: what is not refused does ask for a device)"""
    with pytest.raises(AssertionError, match="default_device was reached"):
        call(**_fhn())
    with pytest.raises(AssertionError, match="default_device was reached"):
        call(**_fhn(times=(), obs_data=np.ones((0, 2, 1))))              # an empty observation set is served
    with pytest.raises(AssertionError, match="default_device was reached"):
        call(**_fhn(times=(0.15 + 0.5 * EVAL_AT_NODE_TOL * 0.05, 0.4)))  # a time within the tolerance is its node
    for p in (2, 6):
        with pytest.raises(AssertionError, match="default_device was reached"):
            call(**_fhn(p=p))


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("times,word", [
    ((0.1, 0.2), "0.2 is no node"), ((0.1, 0.2), "grid_with_times"), ((0.3, 0.1), "strictly increasing"),
    ((0.1, 0.1), "strictly increasing"), ((0.1, 0.1 + 0.5e-11 * 0.05), "same node"), ((0.1, np.nan), "non-finite"),
    ((0.1, np.inf), "non-finite"), ((0.1, 0.41), "inside the grid"), ((-0.01, 0.1), "inside the grid")])
def test_the_node_rule(no_device, call, times, word):
    with pytest.raises(ValueError, match=word) as e:
        call(**_fhn(times=times))
    assert "daltonng_grid" in str(e.value)
    with pytest.raises(ValueError, match="shape"):
        call(**_fhn(obs_times=np.array([0.1])))                          # two observations, one time


@pytest.mark.parametrize("call", CALLS)
def test_the_configurations_daltonng_refuses(no_device, call):
    with pytest.raises(NotImplementedError, match="daltonng_grid.*square-root"):
        call(**_fhn(kalman_type="square-root"))
    with pytest.raises(NotImplementedError):
        call(**_fhn(kalman_type="other"))
    with pytest.raises(NotImplementedError, match="daltonng_grid.*chkrebtii"):
        call(**_fhn(interrogate=functools.partial(interrogate_chkrebtii, kalman_type="standard")))
    with pytest.raises(NotImplementedError, match="daltonng_grid.*n_bmeas"):
        call(**_fhn(ode_weight=np.zeros((2, 2, 3))))
    for p in (1, 7):
        with pytest.raises(NotImplementedError, match="daltonng_grid.*n_bstate"):
            call(**_fhn(ode_weight=np.zeros((2, 1, p))))
    with pytest.raises(NotImplementedError, match="daltonng_grid.*three or more blocks"):
        call(**_fhn(ode_fun=ra.ode.lorenz63, ode_weight=np.zeros((3, 1, 6)), obs_data=np.ones((2, 3, 1))))
    with pytest.raises(NotImplementedError, match="daltonng_grid.*lane-per-trajectory"):
        call(**_fhn(ode_fun=ra.ode.linear_dense(1, 3), ode_weight=np.zeros((1, 1, 3)), obs_data=np.ones((2, 1, 1))))
    with pytest.raises(NotImplementedError, match="daltonng_grid.*blocks"):
        call(**_fhn(ode_fun=ra.ode.higher_order))
    with pytest.raises(ValueError, match="obs_data"):
        call(**_fhn(obs_data=np.ones((2, 3, 1))))
    with pytest.raises(TypeError, match="obs_loglik_i"):
        call(**_fhn(obs_loglik_i=1.0))
    with pytest.raises(ValueError, match="columns"):
        call(**_fhn(obs_data=np.ones((2, 2, 5))))
    with pytest.raises(ValueError, match="scalar"):
        call(**_fhn(obs_loglik_i=lambda y, X, i, **kw: X[:, 0] * y[:, 0]))
    with pytest.raises(ValueError, match="more than 3"):
        call(**_fhn(p=4, obs_loglik_i=lambda y, X, i, **kw: -np.sum(X[0, :] ** 2)))
    with pytest.raises(ValueError, match="does not depend on the state"):
        call(**_fhn(obs_loglik_i=lambda y, X, i, **kw: np.sum(y) * 1.0))


@pytest.mark.parametrize("call", CALLS)
def test_the_grids_and_priors_solve_mv_grid_refuses(no_device, call):
    for bad, word in ((np.zeros((3, 5)), "per-trajectory grids are not built"), ([0.0], "at least two"),
                      ([0.0, np.nan, 1.0], "non-finite"), ([0.0, 0.5, 0.5], "strictly increasing")):
        with pytest.raises(ValueError, match=word):
            call(**_fhn(t_grid=bad))
    with pytest.raises(ValueError, match="callable"):
        call(**_fhn(prior_at=1.0))
    with pytest.raises(ValueError, match="shape"):
        call(**_fhn(prior_at=lambda h: ra.ibm_init(h, 4, np.array([0.5, 0.3]))))
    with pytest.raises(ValueError, match="pair"):
        call(**_fhn(prior_at=lambda h: 1.0))
    with pytest.raises(ValueError, match="non-finite"):
        call(**_fhn(prior_at=lambda h: tuple(a * np.nan for a in ra.ibm_init(h, 3, np.array([0.5, 0.3])))))


def test_prior_at_is_called_once_per_slot_and_the_function_is_traced_once(no_device):
    calls, runs = [], []

    def prior_at(h):
        calls.append(h)
        return ra.ibm_init(h, 3, np.array([0.5, 0.3]))

    def loglik(y, X, i, **kw):
        runs.append(1)
        return poisson_loglik(y, X, i, **kw)
    with pytest.raises(AssertionError, match="default_device was reached"):
        dmod.daltonng_grid(**_fhn(prior_at=prior_at, obs_loglik_i=loglik))
    assert len(calls) == len(ra.grid_slots([0.0, 0.1, 0.15, 0.3, 0.4])[0]) == 3 and len(runs) == 1


def test_the_model_cache_is_daltonng_s(monkeypatch):
    """A log-likelihood traced for daltonng is found again by daltonng_grid: one model, one registration."""
    monkeypatch.setattr(dmod, "_obs_models", {})
    a = _fhn()
    fn = lambda y, X, i, **kw: -0.5 * np.sum((y[:, 0] - X[:, 0]) ** 2)      # noqa: E731
    m1 = dmod._ng_refusals(a["ode_fun"], a["ode_weight"], interrogate_kramer, "standard", a["obs_data"], np.array([0.1, 0.3]), fn, 0.0,
                           0.4, 4, {"theta": THETA})[2]
    obs = dmod._ng_config("daltonng_grid", a["ode_fun"], a["ode_weight"], interrogate_kramer, "standard", a["obs_data"], fn)
    assert dmod._ng_model(a["ode_fun"], a["ode_weight"], obs, fn, {"theta": THETA}) is m1 and len(dmod._obs_models) == 1


# ---- daltonng and solve_mv_nn refuse exactly what they refused before -----------------------------------------------------------
def _old_case(p=3, d=2, n_obs=3):
    W = np.zeros((d, 1, p))
    W[:, :, 1] = 1.0
    return dict(W=W, x0=np.zeros((d, p)), prior=ra.ibm_init(0.05, p, np.full(d, 0.1)), y=np.ones((n_obs, d, 1)),
                times=np.linspace(0.5, 2.0, n_obs))


def _old_call(fn, c, itg=interrogate_kramer, loglik=poisson_loglik, ode=ra.ode.fitzhugh_nagumo, **kw):
    return fn(None, ode, c["W"], c["x0"], 0.0, 2.0, 40, itg, c["prior"], c["y"], c["times"], loglik, **{"theta": THETA, **kw})


@pytest.mark.parametrize("fn", [dmod.daltonng, dmod.solve_mv_nn], ids=["daltonng", "solve_mv_nn"])
def test_daltonng_refuses_what_it_refused_with_the_same_messages(fn, no_device):
    """The exact texts of the refusals before the split (they name daltonng, never daltonng_grid), in their old order: a call
    that breaks two rules raises the one that came first."""
    def message(exc, **kw):
        with pytest.raises(exc) as e:
            _old_call(fn, **kw)
        return str(e.value)
    assert message(NotImplementedError, c=_old_case(), kalman_type="square-root") == \
        "daltonng: the square-root form is not built on the device (kalman_type='standard' only)"
    assert message(NotImplementedError, c=_old_case(), itg=functools.partial(interrogate_chkrebtii, kalman_type="standard")) == \
        "daltonng: interrogate_chkrebtii is not supported (rodeo, schober, kramer)"
    assert message(NotImplementedError, c=dict(_old_case(), W=np.zeros((2, 2, 3)))) == "daltonng on the device: n_bmeas = 1 only"
    assert message(NotImplementedError, c=dict(_old_case(), W=np.zeros((2, 1, 7)))) == "daltonng on the device: n_bstate in 2..6"
    assert message(NotImplementedError, c=_old_case(p=6, d=3), ode=ra.ode.lorenz63) == \
        "daltonng on the device: n_bstate up to 5 with three or more blocks"
    assert message(NotImplementedError, c=_old_case(d=1), ode=ra.ode.linear_dense(1, 3)).startswith(
        "daltonng on the device: the built-in right-hand side")
    assert message(NotImplementedError, c=_old_case(), ode=ra.ode.higher_order) == \
        "daltonng on the device: the right-hand side 'higher_order' has 1 blocks, ode_weight has 2"
    assert message(ValueError, c=dict(_old_case(), y=np.ones((3, 3, 1)))) == "obs_data must have shape (n_obs, 2, n_ycols), got (3, 3, 1)"
    assert message(TypeError, c=_old_case(), loglik=None).startswith("obs_loglik_i must be a Python function")
    assert message(ValueError, c=dict(_old_case(), times=np.array([0.5, 1.0]))) == "obs_times must have shape (3,), got (2,)"
    assert message(ValueError, c=dict(_old_case(), times=np.array([0.5, 1.0, 2.5]))) == "daltonng: an observation time lies beyond t_max"
    assert message(ValueError, c=dict(_old_case(), times=np.array([0.5, 0.5, 2.0]))).startswith(
        "daltonng: the observations' grid indices must be strictly increasing")
    # the order: the times are looked at before the function is traced, the function's type before the times
    assert "beyond t_max" in message(ValueError, c=dict(_old_case(), times=np.array([0.5, 1.0, 2.5])),
                                     loglik=lambda y, X, i, **kw: np.sum(y) * 1.0)
    assert "does not depend on the state" in message(ValueError, c=_old_case(), loglik=lambda y, X, i, **kw: np.sum(y) * 1.0)
    assert message(TypeError, c=dict(_old_case(), times=np.array([0.5, 1.0])), loglik=None).startswith("obs_loglik_i")
    with pytest.raises(AssertionError, match="default_device was reached"):
        _old_call(fn, _old_case())


# ---- the library, on the configuration alone ---------------------------------------------------------------------------
def _register(p=3, d=2, name="HostGridObs"):
    lib = _lib.load()
    name = f"{name}_{d}_{p}"
    src, _ = trace_obs_source(poisson_loglik, d, p, 1, (("theta", 3),), name)
    oid = C.c_int32(0)
    _lib.check(lib.rk_register_obs_source(name.encode(), src.encode(), d, p, 1, 3, 1, C.byref(oid)))
    return oid.value


@functools.lru_cache(maxsize=None)
def _obs_id(p=3, d=2):
    return _register(p, d)


def _cfg(rhs=_lib.RHS_FITZHUGH_NAGUMO, d=2, p=3, m=1, itg=_lib.INTERROGATE_KRAMER, kalman=_lib.KALMAN_STANDARD, n_steps=50,
         flags=_lib.FLAG_BATCH_MINOR, n_theta=3):
    return _lib.SolveCfg(n_traj=16, n_steps=n_steps, n_block=d, n_bstate=p, n_bmeas=m, rhs_id=rhs, interrogate=itg,
                         kalman_type=kalman, n_theta=n_theta, flags=flags, t_min=0.0, t_max=1.0, seed=0, traj_offset=0)


def _loglik(cfg, oid):
    """rk_daltonng_grid_loglik with no handle and no pointers: only the configuration and the registered model can be looked at."""
    lib = _lib.load()
    rc = lib.rk_daltonng_grid_loglik(None, C.byref(cfg), None, oid, None, None, 1, None, None, 0, None)
    return rc, lib.rk_last_error().decode()


def _solve(cfg, oid, mode=_lib.MODE_MV):
    lib = _lib.load()
    rc = lib.rk_daltonng_grid_solve(None, C.byref(cfg), None, None, mode, oid, None, None, 1, None)
    return rc, lib.rk_last_error().decode()


def _both(cfg, oid):
    return [_loglik(cfg, oid), _solve(cfg, oid, _lib.MODE_MV), _solve(cfg, oid, _lib.MODE_FILTER)]


@pytest.mark.parametrize("cfg,word", [
    (_cfg(kalman=7), "kalman_type"),
    (_cfg(kalman=_lib.KALMAN_SQRT), "not built"),
    (_cfg(itg=9), "interrogate"),
    (_cfg(itg=_lib.INTERROGATE_CHKREBTII), "interrogate"),
    (_cfg(m=2), "n_bmeas"),
    (_cfg(p=1), "n_bstate"),
    (_cfg(p=7), "n_bstate"),
    (_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=6), "three or more blocks"),
    (_cfg(flags=_lib.FLAG_BATCH_MINOR | _lib.FLAG_STORE_PRED), "STORE_PRED"),
])
def test_library_refuses_what_is_not_served(cfg, word):
    for rc, msg in _both(cfg, _obs_id()):
        assert rc == _lib.RK_ERR_UNSUPPORTED, (rc, msg)
        assert "daltonng_grid" in msg and word in msg, msg


def test_library_refuses_a_right_hand_side_or_a_model_of_another_configuration():
    for rc, msg in _both(_cfg(rhs=77), _obs_id()):
        assert rc == _lib.RK_ERR_UNSUPPORTED and "daltonng_grid" in msg and "rhs_id" in msg, (rc, msg)
    for rc, msg in _both(_cfg(rhs=_lib.RHS_HIGHER_ORDER), _obs_id()):            # one block against the model's two
        assert rc == _lib.RK_ERR_UNSUPPORTED and "daltonng_grid" in msg and "n_block" in msg, (rc, msg)
    for rc, msg in _both(_cfg(p=4), _obs_id(3)):
        assert rc == _lib.RK_ERR_INVALID and "daltonng_grid" in msg and "registered for" in msg, (rc, msg)
    for rc, msg in _both(_cfg(n_theta=2), _obs_id()):
        assert rc == _lib.RK_ERR_INVALID and "daltonng_grid" in msg and "parameters" in msg, (rc, msg)
    for rc, msg in _both(_cfg(), 10 ** 6):
        assert rc == _lib.RK_ERR_INVALID and "obs_id" in msg, (rc, msg)


@pytest.mark.parametrize("cfg", [_cfg(n_steps=0), _cfg(d=0), _cfg(p=0), _cfg(m=0)])
def test_library_calls_a_non_positive_size_invalid(cfg):
    for rc, msg in _both(cfg, _obs_id()):
        assert rc == _lib.RK_ERR_INVALID and "daltonng_grid" in msg, (rc, msg)


def test_library_calls_another_mode_or_a_missing_flag_invalid():
    for mode in (_lib.MODE_SIM, 7, -1):
        rc, msg = _solve(_cfg(), _obs_id(), mode)
        assert rc == _lib.RK_ERR_INVALID and "daltonng_grid" in msg and "mode" in msg, (rc, msg)
    for rc, msg in _both(_cfg(flags=0), _obs_id()):
        assert rc == _lib.RK_ERR_INVALID and "daltonng_grid" in msg and "RK_FLAG_BATCH_MINOR" in msg, (rc, msg)


@pytest.mark.parametrize("p,itg", [(3, _lib.INTERROGATE_KRAMER), (2, _lib.INTERROGATE_RODEO), (6, _lib.INTERROGATE_SCHOBER)])
def test_library_passes_a_served_configuration_on_to_the_argument_check(p, itg):
    """A served configuration gets as far as the null handle: RK_ERR_INVALID about the arguments, not about the cfg."""
    for rc, msg in _both(_cfg(p=p, itg=itg), _obs_id(p)):
        assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
    for rc, msg in _both(_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=5), _obs_id(5, 3)):
        assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
    lib = _lib.load()
    assert lib.rk_daltonng_grid_loglik(None, None, None, 0, None, None, 1, None, None, 0, None) == _lib.RK_ERR_INVALID
    assert lib.rk_daltonng_grid_solve(None, None, None, None, _lib.MODE_MV, 0, None, None, 1, None) == _lib.RK_ERR_INVALID


def test_the_two_new_kernel_kinds_compile_for_the_device(capfd, monkeypatch):
    """hiprtc builds both forms of daltonng_grid_fwd_kernel around the traced struct (no GPU needed), FitzHugh-Nagumo with the
    Poisson model at n_bstate = 3, kramer; RK_JIT_VERBOSE reports each build's resources; a model that does not compile, and an
    unknown one, fail cleanly."""
    lib = _lib.load()
    monkeypatch.setenv("RK_JIT_VERBOSE", "1")
    oid = _register(name="HostGridObsCompile")
    _lib.check(lib.rk_obs_grid_compile_check(oid, _lib.RHS_FITZHUGH_NAGUMO, _lib.INTERROGATE_KRAMER))
    err = capfd.readouterr().err
    lines = [ln for ln in err.splitlines() if "jit build" in ln and "daltonng_grid_fwd_kernel" in ln]
    assert len(lines) == 2 and all("0 B scratch per lane" in ln for ln in lines), err
    bad = C.c_int32(0)
    _lib.check(lib.rk_register_obs_source(b"NopeGrid", b"struct NopeGrid { int x };", 2, 3, 1, 3, 1, C.byref(bad)))
    assert lib.rk_obs_grid_compile_check(bad.value, _lib.RHS_FITZHUGH_NAGUMO, _lib.INTERROGATE_KRAMER) == _lib.RK_ERR_INVALID
    assert "NopeGrid" in lib.rk_last_error().decode()
    assert lib.rk_obs_grid_compile_check(10 ** 6, _lib.RHS_FITZHUGH_NAGUMO, _lib.INTERROGATE_KRAMER) == _lib.RK_ERR_INVALID
    assert "obs_id" in lib.rk_last_error().decode()


def test_the_staged_pair_instances_keep_to_the_ship_rule(capfd, monkeypatch):
    """n_bstate = 5 stages the pair in LDS, where the kernel's stores and predictions are arranged for the register allocator
    (csrc/daltonng_grid_kernels.hpp: SPLIT and the barrier behind predict_block).  The ship rule -- no more scratch than
    daltonng_fwd_kernel of the same form -- is held here for FitzHugh-Nagumo with Poisson, rodeo, both forms: daltonng_fwd_kernel
    has none there, so neither may the grid kernel (without either arrangement it takes 100 .. 172 B)."""
    lib = _lib.load()
    monkeypatch.setenv("RK_JIT_VERBOSE", "1")
    oid = _register(p=5, name="HostGridObsShip")
    _lib.check(lib.rk_obs_compile_check(oid, _lib.RHS_FITZHUGH_NAGUMO, _lib.INTERROGATE_RODEO))
    _lib.check(lib.rk_obs_grid_compile_check(oid, _lib.RHS_FITZHUGH_NAGUMO, _lib.INTERROGATE_RODEO))
    err = capfd.readouterr().err

    def scratch(kernel):
        found = re.findall(r"jit build \S*%s\S*: .*?, (\d+) B scratch per lane, (\d+) B LDS" % kernel, err)
        assert len(found) == 2, err
        return [int(a) for a, _ in found], [int(b) for _, b in found]
    (uniform, _), (grid, lds) = scratch("19daltonng_fwd_kernel"), scratch("24daltonng_grid_fwd_kernel")
    print(f"scratch per lane, both / store: daltonng_fwd_kernel {uniform}, daltonng_grid_fwd_kernel {grid}; LDS {lds}")
    assert all(g <= u for g, u in zip(grid, uniform)) and all(b > 0 for b in lds)
