"""
``solve_mv_dynamic`` / ``solve_sim_dynamic`` on the host (no GPU): the signature and re-export, the refusals that come before
any device work (``default_device`` patched to fail), and the library's refusals on the configuration alone (no handle, no
pointers), a traced right-hand side among them.
"""
import ctypes as C
import functools
import inspect
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd import _lib
from rodeo_amd.dynamic import DynamicMV, DynamicSim
from rodeo_amd.interrogate import interrogate_kramer, interrogate_rodeo, interrogate_chkrebtii

DYNAMIC_ARGS = ["key", "ode_fun", "ode_weight", "ode_init", "t_min", "t_max", "n_steps", "interrogate", "prior_pars",
                "kalman_type", "scale_min", "params"]
SOLVERS = [ra.dynamic.solve_mv_dynamic, ra.dynamic.solve_sim_dynamic]


def test_signature_and_re_export():
    assert ra.solve_mv_dynamic is ra.dynamic.solve_mv_dynamic and ra.solve_sim_dynamic is ra.dynamic.solve_sim_dynamic
    assert ra.DynamicMV is DynamicMV and ra.DynamicSim is DynamicSim
    for fn in SOLVERS:
        sig = inspect.signature(fn)
        assert list(sig.parameters) == DYNAMIC_ARGS
        assert list(sig.parameters)[:9] == list(inspect.signature(ra.solve_mv).parameters)[:9]
        assert sig.parameters["kalman_type"].default == "standard"
        assert sig.parameters["scale_min"].default == 0.0
        assert sig.parameters["params"].kind is inspect.Parameter.VAR_KEYWORD
        assert "scale_min" in fn.__doc__
    assert "NaN" in ra.solve_mv_dynamic.__doc__ and "ODE" in ra.solve_mv_dynamic.__doc__     # the z = 0 case, the reserved keyword
    assert DynamicMV._fields == ("mean", "var", "scale", "logdens")
    assert DynamicSim._fields == ("x", "scale", "logdens")


def _fhn(p=3, N=40, t_max=4.0, ode=ra.ode.fitzhugh_nagumo):
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    theta = np.array([0.2, 0.2, 3.0])
    x0 = init(np.array([-1.0, 1.0]), 0.0, theta=theta)
    prior = ra.ibm_init(t_max / N, p, np.array([0.5, 0.3]))
    return dict(key=None, ode_fun=ode, ode_weight=W, ode_init=x0, t_min=0.0, t_max=t_max, n_steps=N,
                interrogate=interrogate_kramer, prior_pars=prior, theta=theta)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device fails the test: the refusals below come first."""
    def fail(*a, **k):
        raise AssertionError("default_device was reached")
    monkeypatch.setattr(ra.device, "default_device", fail)
    monkeypatch.setattr(ra.solve, "default_device", fail)


@pytest.mark.parametrize("solver", SOLVERS)
def test_unknown_kalman_type_is_refused(no_device, solver):
    with pytest.raises(NotImplementedError, match="kalman_type"):
        solver(**_fhn(), kalman_type="nope")


@pytest.mark.parametrize("solver", SOLVERS)
def test_the_square_root_form_is_not_built(no_device, solver):
    with pytest.raises(NotImplementedError, match="not built"):
        solver(**_fhn(), kalman_type="square-root")


@pytest.mark.parametrize("solver", SOLVERS)
def test_chkrebtii_is_refused_with_the_reason(no_device, solver):
    a = _fhn()
    a["interrogate"] = functools.partial(interrogate_chkrebtii, kalman_type="standard")
    with pytest.raises(NotImplementedError, match="interrogate_chkrebtii.*predicted variance.*depends on the point"):
        solver(**a)


@pytest.mark.parametrize("solver", SOLVERS)
def test_several_measurements_per_block_are_refused(no_device, solver):
    a = _fhn()
    a["ode_weight"] = np.concatenate([a["ode_weight"]] * 2, axis=1)         # n_bmeas = 2 (the dense / indep_init form)
    with pytest.raises(NotImplementedError, match="n_bmeas"):
        solver(**a)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("p", [1, 6, 7])
def test_n_bstate_outside_two_to_five_is_refused(no_device, solver, p):
    W = np.zeros((2, 1, p)); W[:, 0, min(1, p - 1)] = 1.0
    a = _fhn()
    a.update(ode_weight=W, ode_init=np.zeros((2, p)), prior_pars=(np.tile(np.eye(p), (2, 1, 1)),) * 2)
    with pytest.raises(NotImplementedError, match="n_bstate"):
        solver(**a)


@pytest.mark.parametrize("solver", SOLVERS)
def test_three_blocks_stop_at_four(no_device, solver):
    W = np.zeros((3, 1, 5)); W[:, 0, 1] = 1.0
    args = dict(key=None, ode_fun=ra.ode.lorenz63, ode_weight=W, ode_init=np.zeros((3, 5)), t_min=0.0, t_max=1.0, n_steps=10,
                interrogate=interrogate_rodeo, prior_pars=(np.tile(np.eye(5), (3, 1, 1)),) * 2, theta=np.array([28.0, 10.0, 8 / 3]))
    with pytest.raises(NotImplementedError, match="three or more blocks"):
        solver(**args)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("change", [
    dict(ode_weight=np.zeros((1, 3))),                                      # rank
    dict(ode_init=np.zeros((2, 4))),                                        # ode_init against ode_weight
    dict(prior_pars=(np.zeros((2, 3, 3)), np.zeros((2, 4, 4)))),            # prior against ode_weight
    dict(ode_init=np.zeros((5, 2, 3)), theta=np.ones((4, 3))),              # inconsistent batch sizes
])
def test_the_shape_rule_s_refusals(no_device, solver, change):
    a = _fhn()
    a.update(change)
    with pytest.raises(ValueError):
        solver(**a)


@pytest.mark.parametrize("solver", SOLVERS)
def test_a_right_hand_side_with_another_block_count_is_refused(no_device, solver):
    with pytest.raises(ValueError, match="n_block"):
        solver(**_fhn(ode=ra.ode.lorenz63))                                # three blocks against a d = 2 weight


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("bad", [-1.0, -1e-300, float("nan"), float("inf"), "x"])
def test_a_negative_or_non_finite_scale_min_is_refused(no_device, solver, bad):
    with pytest.raises(ValueError, match="scale_min"):
        solver(**_fhn(), scale_min=bad)


def test_an_arbitrary_interrogate_is_a_type_error(no_device):
    a = _fhn()
    a["interrogate"] = lambda **k: None
    with pytest.raises(TypeError):
        ra.solve_mv_dynamic(**a)


# ---- the library, on the configuration alone ---------------------------------------------------------------------------
def _cfg(rhs=_lib.RHS_FITZHUGH_NAGUMO, d=2, p=3, m=1, itg=_lib.INTERROGATE_KRAMER, kalman=_lib.KALMAN_STANDARD, n_steps=50):
    return _lib.SolveCfg(n_traj=16, n_steps=n_steps, n_block=d, n_bstate=p, n_bmeas=m, rhs_id=rhs, interrogate=itg,
                         kalman_type=kalman, n_theta=3, flags=_lib.FLAG_BATCH_MINOR, t_min=0.0, t_max=1.0, seed=0, traj_offset=0)


def _call(cfg, mode=_lib.MODE_MV, scale_min=0.0):
    """rk_solve_dynamic with no handle and no pointers: only the configuration, the mode and scale_min can be looked at."""
    lib = _lib.load()
    rc = lib.rk_solve_dynamic(None, C.byref(cfg), None, None, mode, scale_min, None, None)
    return rc, lib.rk_last_error().decode()


@pytest.mark.parametrize("cfg,word", [
    (_cfg(kalman=7), "kalman_type"),
    (_cfg(kalman=_lib.KALMAN_SQRT), "not built"),
    (_cfg(itg=_lib.INTERROGATE_CHKREBTII), "chkrebtii"),
    (_cfg(itg=9), "interrogate"),
    (_cfg(m=2), "n_bmeas"),
    (_cfg(p=1), "n_bstate"),
    (_cfg(p=6), "n_bstate"),
    (_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=5), "three or more blocks"),
    (_cfg(rhs=_lib.RHS_LORENZ63, d=2), "n_block"),
    (_cfg(rhs=77), "rhs_id"),
])
def test_library_refuses_what_is_not_served(cfg, word):
    for mode in (_lib.MODE_MV, _lib.MODE_SIM):
        rc, msg = _call(cfg, mode)
        assert rc == _lib.RK_ERR_UNSUPPORTED, (rc, msg)
        assert "dynamic" in msg and word in msg, msg


@pytest.mark.parametrize("cfg", [_cfg(n_steps=0), _cfg(d=0), _cfg(p=0), _cfg(m=0)])
def test_library_calls_a_non_positive_size_invalid(cfg):
    rc, msg = _call(cfg)
    assert rc == _lib.RK_ERR_INVALID and "dynamic" in msg, (rc, msg)


@pytest.mark.parametrize("mode,scale_min,word", [(_lib.MODE_FILTER, 0.0, "mode"), (7, 0.0, "mode"), (_lib.MODE_MV, -1.0, "scale_min"),
                                                 (_lib.MODE_SIM, float("nan"), "scale_min"), (_lib.MODE_MV, float("inf"), "scale_min")])
def test_library_calls_another_mode_or_a_bad_scale_min_invalid(mode, scale_min, word):
    rc, msg = _call(_cfg(), mode, scale_min)
    assert rc == _lib.RK_ERR_INVALID and "dynamic" in msg and word in msg, (rc, msg)


@pytest.mark.parametrize("cfg", [_cfg(), _cfg(p=2), _cfg(p=5), _cfg(itg=_lib.INTERROGATE_RODEO), _cfg(itg=_lib.INTERROGATE_SCHOBER),
                                 _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=3), _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=4),
                                 _cfg(rhs=_lib.RHS_HIGHER_ORDER, d=1, p=4)])
def test_library_passes_a_served_configuration_on_to_the_argument_check(cfg):
    """A served configuration gets as far as the null handle: RK_ERR_INVALID about the arguments, not about the cfg."""
    for mode in (_lib.MODE_MV, _lib.MODE_SIM):
        rc, msg = _call(cfg, mode, 0.5)
        assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
    assert _lib.load().rk_solve_dynamic(None, None, None, None, _lib.MODE_MV, 0.0, None, None) == _lib.RK_ERR_INVALID


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


@pytest.mark.parametrize("p,served", [(2, True), (5, True), (6, False)])
def test_library_serves_a_traced_right_hand_side_over_the_same_range(p, served):
    from rodeo_amd.trace import from_python
    ode = from_python(_fitz, 2, p, theta=3)
    rc, msg = _call(_cfg(rhs=ode.rhs_id, p=p))
    if served:
        assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
    else:
        assert rc == _lib.RK_ERR_UNSUPPORTED and "dynamic" in msg and "n_bstate" in msg, (rc, msg)
    rc, msg = _call(_cfg(rhs=ode.rhs_id, p=min(p, 4), d=3))                # another block count than the registration's
    assert rc == _lib.RK_ERR_UNSUPPORTED and "dynamic" in msg and "n_block" in msg, (rc, msg)
