"""
``fenrir_grid`` / ``fenrir.solve_mv_grid`` on the host (no GPU): the signatures, every refusal that comes before any device work
(``default_device`` patched to fail), ``prior_at`` called once per slot, and the library's refusals on the configuration and
n_bobs alone (no handle, no pointers), a traced right-hand side among them.
"""
import ctypes as C
import functools
import inspect
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.fenrir  # noqa: F401
from rodeo_amd import _lib
from rodeo_amd.interrogate import interrogate_chkrebtii, interrogate_kramer
from rodeo_amd.solve import EVAL_AT_NODE_TOL

fmod = sys.modules["rodeo_amd.inference.fenrir"]             # (rodeo_amd.inference.fenrir, the attribute, is the function)
dmod = sys.modules["rodeo_amd.inference.dalton"]
CALLS = [fmod.fenrir_grid, fmod.solve_mv_grid]
ARGS = ["key", "ode_fun", "ode_weight", "ode_init", "t_grid", "interrogate", "prior_at", "obs_data", "obs_times", "obs_weight",
        "obs_var", "kalman_type", "params"]


def test_signatures_and_exports():
    for fn in CALLS:
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ARGS
        assert list(sig.parameters) == list(inspect.signature(dmod.dalton_grid).parameters)
        assert list(sig.parameters)[:7] == list(inspect.signature(ra.solve_mv_grid).parameters)[:7]
        assert sig.parameters["kalman_type"].default == "standard"
        assert sig.parameters["params"].kind is inspect.Parameter.VAR_KEYWORD
    for name in ("fenrir_grid", "solve_mv_grid"):
        assert not hasattr(ra.inference, name) or getattr(ra.inference, name) is not getattr(fmod, name)   # not re-exported
    assert "grid_with_times" in fmod.fenrir_grid.__doc__ and "node 0" in fmod.fenrir_grid.__doc__
    assert "_obs_nodes" not in vars(fmod)                            # dalton_grid's node rule is used, not copied


# ---- refusals before any device work --------------------------------------------------------------------------------------
def _fhn(p=3, n_bobs=1, times=(0.1, 0.3), **over):
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    theta = np.array([0.2, 0.2, 3.0])
    sigma = np.array([0.5, 0.3])
    n = len(times)
    D = np.zeros((n, 2, n_bobs, p))
    D[..., 0, 0] = 1.0
    a = dict(key=None, ode_fun=ra.ode.fitzhugh_nagumo, ode_weight=W, ode_init=init(np.array([-1.0, 1.0]), 0.0, theta=theta),
             t_grid=np.array([0.0, 0.1, 0.15, 0.3, 0.4]), interrogate=interrogate_kramer, prior_at=lambda h: ra.ibm_init(h, p, sigma),
             obs_data=np.zeros((n, 2, n_bobs)), obs_times=np.array(times, dtype=float), obs_weight=D,
             obs_var=np.tile(0.01 * np.eye(n_bobs), (n, 2, 1, 1)), theta=theta)
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
    with pytest.raises(AssertionError, match="default_device was reached"):     # chkrebtii is served: the forward pass is the grid solver's
        call(**_fhn(key=3, interrogate=functools.partial(interrogate_chkrebtii, kalman_type="standard")))
    with pytest.raises(AssertionError, match="default_device was reached"):     # every instance ships, (6, 3) included
        call(**_fhn(p=6, n_bobs=3))
    with pytest.raises(AssertionError, match="default_device was reached"):     # an empty observation set
        call(**_fhn(times=()))
    with pytest.raises(AssertionError, match="default_device was reached"):     # node 0 and node N
        call(**_fhn(times=(0.0, 0.4)))


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("times,word", [
    ((0.1, 0.2), "0.2 is no node"), ((0.3, 0.1), "strictly increasing"), ((0.1, 0.1), "strictly increasing"),
    ((0.1, 0.1 + 0.5e-11 * 0.05), "same node"), ((0.1, np.nan), "non-finite"), ((0.1, np.inf), "non-finite"),
    ((0.1, 0.41), "inside the grid"), ((-0.01, 0.1), "inside the grid")])
def test_bad_observation_times_are_refused(no_device, call, times, word):
    with pytest.raises(ValueError, match=word):
        call(**_fhn(times=times))


@pytest.mark.parametrize("call", CALLS)
def test_the_message_for_a_time_off_the_nodes_names_the_helper(no_device, call):
    with pytest.raises(ValueError, match="grid_with_times"):
        call(**_fhn(times=(0.1, 0.2)))
    with pytest.raises(ValueError, match="shape"):
        call(**_fhn(obs_times=np.array([0.1])))                          # two observations, one time


@pytest.mark.parametrize("call", CALLS)
def test_a_time_within_the_tolerance_is_its_node(no_device, call):
    with pytest.raises(AssertionError, match="default_device was reached"):
        call(**_fhn(times=(0.15 + 0.5 * EVAL_AT_NODE_TOL * 0.05, 0.4)))


@pytest.mark.parametrize("call", CALLS)
def test_the_configurations_and_shapes_that_are_refused(no_device, call):
    with pytest.raises(NotImplementedError, match="not built"):
        call(**_fhn(kalman_type="square-root"))
    with pytest.raises(NotImplementedError):
        call(**_fhn(kalman_type="other"))
    with pytest.raises(NotImplementedError, match="n_bmeas"):
        call(**_fhn(ode_weight=np.zeros((2, 2, 3))))
    with pytest.raises(NotImplementedError, match="n_bstate"):
        call(**_fhn(p=7))
    with pytest.raises(NotImplementedError, match="n_bobs"):
        call(**_fhn(n_bobs=4))
    with pytest.raises(ValueError, match="obs_weight"):
        call(**_fhn(obs_weight=np.zeros((2, 2, 1, 4))))
    with pytest.raises(ValueError, match="obs_weight"):
        call(**_fhn(obs_weight=np.zeros((2, 2, 3))))
    with pytest.raises(ValueError):
        call(**_fhn(obs_var=np.zeros((2, 2, 2, 2))))
    with pytest.raises(ValueError):
        call(**_fhn(obs_data=np.zeros((2, 2))))


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
    with pytest.raises(ValueError, match="n_block"):
        call(**_fhn(ode_fun=ra.ode.lorenz63))                            # three blocks against a d = 2 weight
    W3, init3 = ra.utils.first_order_pad(ra.ode.lorenz63, 3, 6)
    with pytest.raises(NotImplementedError, match="three or more blocks"):
        call(**_fhn(ode_fun=ra.ode.lorenz63, ode_weight=W3, obs_weight=np.zeros((2, 3, 1, 6)), obs_data=np.zeros((2, 3, 1)),
                    obs_var=np.ones((2, 3, 1, 1))))


@pytest.mark.parametrize("call", CALLS)
def test_prior_at_is_called_once_per_slot(no_device, call):
    calls = []

    def prior_at(h):
        calls.append(h)
        return ra.ibm_init(h, 3, np.array([0.5, 0.3]))
    with pytest.raises(AssertionError, match="default_device was reached"):
        call(**_fhn(prior_at=prior_at))
    assert len(calls) == len(ra.grid_slots([0.0, 0.1, 0.15, 0.3, 0.4])[0]) == 3


# ---- the library, on the configuration alone ---------------------------------------------------------------------------
def _cfg(rhs=_lib.RHS_FITZHUGH_NAGUMO, d=2, p=3, m=1, itg=_lib.INTERROGATE_KRAMER, kalman=_lib.KALMAN_STANDARD, n_steps=50,
         flags=_lib.FLAG_BATCH_MINOR):
    return _lib.SolveCfg(n_traj=16, n_steps=n_steps, n_block=d, n_bstate=p, n_bmeas=m, rhs_id=rhs, interrogate=itg,
                         kalman_type=kalman, n_theta=3, flags=flags, t_min=0.0, t_max=1.0, seed=0, traj_offset=0)


def _both(cfg, n_bobs=1):
    """Both entries with no handle and no pointers: only the configuration and n_bobs can be looked at."""
    lib = _lib.load()
    out = []
    for fn in (lib.rk_fenrir_grid_loglik, lib.rk_fenrir_grid_solve_mv):
        rc = fn(None, C.byref(cfg), None, None, None, None, None, None, 1, n_bobs, None, None)
        out.append((rc, lib.rk_last_error().decode()))
    return out


@pytest.mark.parametrize("cfg,word", [
    (_cfg(kalman=7), "kalman_type"),
    (_cfg(kalman=_lib.KALMAN_SQRT), "not built"),
    (_cfg(itg=9), "interrogate"),
    (_cfg(m=2), "n_bmeas"),
    (_cfg(p=1), "n_bstate"),
    (_cfg(p=7), "n_bstate"),
    (_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=6), "three or more blocks"),
    (_cfg(rhs=_lib.RHS_LORENZ63, d=2), "n_block"),
    (_cfg(rhs=77), "rhs_id"),
    (_cfg(flags=_lib.FLAG_BATCH_MINOR | _lib.FLAG_STORE_PRED), "STORE_PRED"),
])
def test_library_refuses_what_is_not_served(cfg, word):
    for rc, msg in _both(cfg):
        assert rc == _lib.RK_ERR_UNSUPPORTED, (rc, msg)
        assert "fenrir_grid" in msg and word in msg, msg


def test_library_refuses_n_bobs_outside_one_to_three():
    for n_bobs in (0, 4):
        for rc, msg in _both(_cfg(), n_bobs):
            assert rc == _lib.RK_ERR_UNSUPPORTED and "fenrir_grid" in msg and "n_bobs" in msg, (rc, msg)


@pytest.mark.parametrize("cfg", [_cfg(n_steps=0), _cfg(d=0), _cfg(p=0), _cfg(m=0)])
def test_library_calls_a_non_positive_size_invalid(cfg):
    for rc, msg in _both(cfg):
        assert rc == _lib.RK_ERR_INVALID and "fenrir_grid" in msg and "non-positive" in msg, (rc, msg)


def test_library_calls_a_missing_flag_invalid():
    for rc, msg in _both(_cfg(flags=0)):
        assert rc == _lib.RK_ERR_INVALID and "fenrir_grid" in msg and "RK_FLAG_BATCH_MINOR" in msg, (rc, msg)


@pytest.mark.parametrize("cfg", [_cfg(), _cfg(p=2), _cfg(p=6), _cfg(itg=_lib.INTERROGATE_RODEO), _cfg(itg=_lib.INTERROGATE_SCHOBER),
                                 _cfg(itg=_lib.INTERROGATE_CHKREBTII), _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=3),
                                 _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=5), _cfg(rhs=_lib.RHS_HIGHER_ORDER, d=1, p=6)])
def test_library_passes_a_served_configuration_on_to_the_argument_check(cfg):
    """A served configuration gets as far as the null handle: RK_ERR_INVALID about the arguments, not about the cfg."""
    for n_bobs in (1, 2, 3):
        for rc, msg in _both(cfg, n_bobs):
            assert rc == _lib.RK_ERR_INVALID and "fenrir_grid" in msg and "null argument" in msg, (rc, msg)
    lib = _lib.load()
    for fn in (lib.rk_fenrir_grid_loglik, lib.rk_fenrir_grid_solve_mv):
        assert fn(None, None, None, None, None, None, None, None, 1, 1, None, None) == _lib.RK_ERR_INVALID
        assert "fenrir_grid" in lib.rk_last_error().decode()


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


@pytest.mark.parametrize("p,served", [(2, True), (6, True), (7, False)])
def test_library_serves_a_traced_right_hand_side_over_the_same_range(p, served):
    from rodeo_amd.trace import from_python
    ode = from_python(_fitz, 2, p, theta=3)
    for rc, msg in _both(_cfg(rhs=ode.rhs_id, p=p)):
        if served:
            assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
        else:
            assert rc == _lib.RK_ERR_UNSUPPORTED and "fenrir_grid" in msg and "n_bstate" in msg, (rc, msg)
    for rc, msg in _both(_cfg(rhs=ode.rhs_id, p=min(p, 5), d=3)):         # another block count than the registration's
        assert rc == _lib.RK_ERR_UNSUPPORTED and "fenrir_grid" in msg and "n_block" in msg, (rc, msg)
