"""
``dalton_grid`` / ``dalton.solve_mv_grid`` / ``dalton.solve_sim_grid`` on the host (no GPU): the signatures, ``grid_with_times`` on
hand-made grids, every refusal that comes before any device work (``default_device`` patched to fail), and the library's refusals
on the configuration alone (no handle, no pointers), a traced right-hand side among them.
"""
import ctypes as C
import functools
import inspect
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401
from rodeo_amd import _lib
from rodeo_amd.interrogate import interrogate_chkrebtii, interrogate_kramer
from rodeo_amd.solve import EVAL_AT_NODE_TOL

dmod = sys.modules["rodeo_amd.inference.dalton"]             # (rodeo_amd.inference.dalton, the attribute, is the function)
CALLS = [dmod.dalton_grid, dmod.solve_mv_grid, dmod.solve_sim_grid]
ARGS = ["key", "ode_fun", "ode_weight", "ode_init", "t_grid", "interrogate", "prior_at", "obs_data", "obs_times", "obs_weight",
        "obs_var", "kalman_type", "params"]


def test_signatures_and_exports():
    for fn in CALLS:
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ARGS
        assert list(sig.parameters)[:7] == list(inspect.signature(ra.solve_mv_grid).parameters)[:7]
        assert sig.parameters["kalman_type"].default == "standard"
        assert sig.parameters["params"].kind is inspect.Parameter.VAR_KEYWORD
    for name in ("dalton_grid", "solve_mv_grid", "solve_sim_grid"):
        assert not hasattr(ra.inference, name) or getattr(ra.inference, name) is not getattr(dmod, name)   # not re-exported
    assert ra.grid_with_times is ra.grid.grid_with_times
    doc = dmod.dalton_grid.__doc__
    assert "1e-8" in doc and "grid_with_times" in doc and "jumps" in doc          # the threshold property is documented


# ---- grid_with_times ------------------------------------------------------------------------------------------------------
def test_grid_with_times_on_hand_made_grids():
    t = np.array([0.0, 0.1, 0.15, 0.3, 0.4])
    t_new, node = ra.grid_with_times(t, [0.1])                           # on a node: nothing is added
    np.testing.assert_array_equal(t_new, t)
    assert list(node) == [1]
    t_new, node = ra.grid_with_times(t, [0.2, 0.05])                     # between nodes, in the order given
    np.testing.assert_array_equal(t_new, [0.0, 0.05, 0.1, 0.15, 0.2, 0.3, 0.4])
    assert list(node) == [4, 1]
    inside = 0.15 + 0.5 * EVAL_AT_NODE_TOL * 0.05                         # the shorter step next to node 2 is 0.05
    outside = 0.15 + 2.0 * EVAL_AT_NODE_TOL * 0.05
    t_new, node = ra.grid_with_times(t, [inside])
    np.testing.assert_array_equal(t_new, t)
    assert list(node) == [2]
    t_new, node = ra.grid_with_times(t, [outside])
    assert len(t_new) == 6 and list(node) == [3] and t_new[3] == outside
    t_new, node = ra.grid_with_times(t, [0.0, 0.4, 0.35, 0.35])          # the ends are nodes; a repeated time is one node
    np.testing.assert_array_equal(t_new, [0.0, 0.1, 0.15, 0.3, 0.35, 0.4])
    assert list(node) == [0, 5, 4, 4]
    t_new, node = ra.grid_with_times(t, [])
    np.testing.assert_array_equal(t_new, t)
    assert node.shape == (0,)


@pytest.mark.parametrize("times,word", [([0.41], "inside the grid"), ([-1e-9], "inside the grid"), ([np.nan], "non-finite"),
                                        ([0.1, np.inf], "non-finite"), ([[0.1]], "1-D")])
def test_grid_with_times_refuses_bad_times(times, word):
    with pytest.raises(ValueError, match=word):
        ra.grid_with_times([0.0, 0.1, 0.15, 0.3, 0.4], times)


def test_grid_with_times_refuses_a_bad_grid():
    with pytest.raises(ValueError, match="strictly increasing"):
        ra.grid_with_times([0.0, 0.2, 0.1], [0.1])


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
def test_the_configurations_dalton_refuses(no_device, call):
    with pytest.raises(NotImplementedError, match="square-root"):
        call(**_fhn(kalman_type="square-root"))
    with pytest.raises(NotImplementedError):
        call(**_fhn(kalman_type="other"))
    with pytest.raises(NotImplementedError, match="chkrebtii"):
        call(**_fhn(interrogate=functools.partial(interrogate_chkrebtii, kalman_type="standard")))
    with pytest.raises(NotImplementedError, match="n_bmeas"):
        call(**_fhn(ode_weight=np.zeros((2, 2, 3))))
    with pytest.raises(NotImplementedError, match="n_bstate"):
        call(**_fhn(p=7))
    with pytest.raises(NotImplementedError, match="n_bobs"):
        call(**_fhn(n_bobs=4))
    with pytest.raises(ValueError, match="obs_weight"):
        call(**_fhn(obs_weight=np.zeros((2, 2, 1, 4))))
    with pytest.raises(ValueError):
        call(**_fhn(obs_var=np.zeros((2, 2, 2, 2))))


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


def test_prior_at_is_called_once_per_slot(no_device):
    calls = []

    def prior_at(h):
        calls.append(h)
        return ra.ibm_init(h, 3, np.array([0.5, 0.3]))
    with pytest.raises(AssertionError, match="default_device was reached"):
        dmod.dalton_grid(**_fhn(prior_at=prior_at))
    assert len(calls) == len(ra.grid_slots([0.0, 0.1, 0.15, 0.3, 0.4])[0]) == 3


def test_the_instance_left_out_is_refused_in_python(no_device):
    """dalton_grid (the log-likelihood form) of fitzhugh_nagumo at n_bstate 4 with three observations per block: its kernel needs
    more scratch than both siblings' (profiles/dalton_grid_code_objects.txt).  The two solvers serve the shape."""
    with pytest.raises(NotImplementedError, match="left out"):
        dmod.dalton_grid(**_fhn(p=4, n_bobs=3))
    with pytest.raises(AssertionError, match="default_device was reached"):
        dmod.solve_mv_grid(**_fhn(p=4, n_bobs=3))
    with pytest.raises(AssertionError, match="default_device was reached"):
        dmod.dalton_grid(**_fhn(p=4, n_bobs=2))


# ---- the library, on the configuration alone ---------------------------------------------------------------------------
def _cfg(rhs=_lib.RHS_FITZHUGH_NAGUMO, d=2, p=3, m=1, itg=_lib.INTERROGATE_KRAMER, kalman=_lib.KALMAN_STANDARD, n_steps=50,
         flags=_lib.FLAG_BATCH_MINOR):
    return _lib.SolveCfg(n_traj=16, n_steps=n_steps, n_block=d, n_bstate=p, n_bmeas=m, rhs_id=rhs, interrogate=itg,
                         kalman_type=kalman, n_theta=3, flags=flags, t_min=0.0, t_max=1.0, seed=0, traj_offset=0)


def _loglik(cfg, n_bobs=1):
    """rk_dalton_grid_loglik with no handle and no pointers: only the configuration and n_bobs can be looked at."""
    lib = _lib.load()
    rc = lib.rk_dalton_grid_loglik(None, C.byref(cfg), None, None, None, None, None, 1, n_bobs, None, None)
    return rc, lib.rk_last_error().decode()


def _solve(cfg, mode=_lib.MODE_MV, n_bobs=1):
    lib = _lib.load()
    rc = lib.rk_dalton_grid_solve(None, C.byref(cfg), None, None, mode, None, None, None, None, 1, n_bobs, None)
    return rc, lib.rk_last_error().decode()


def _both(cfg, n_bobs=1):
    return [_loglik(cfg, n_bobs), _solve(cfg, _lib.MODE_MV, n_bobs), _solve(cfg, _lib.MODE_SIM, n_bobs)]


@pytest.mark.parametrize("cfg,word", [
    (_cfg(kalman=7), "kalman_type"),
    (_cfg(kalman=_lib.KALMAN_SQRT), "not built"),
    (_cfg(itg=9), "interrogate"),
    (_cfg(itg=_lib.INTERROGATE_CHKREBTII), "interrogate"),
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
        assert "dalton_grid" in msg and word in msg, msg


def test_library_refuses_n_bobs_outside_one_to_three_and_the_instance_left_out():
    for n_bobs in (0, 4):
        for rc, msg in _both(_cfg(), n_bobs):
            assert rc == _lib.RK_ERR_UNSUPPORTED and "dalton_grid" in msg and "n_bobs" in msg, (rc, msg)
    rc, msg = _loglik(_cfg(p=4), 3)
    assert rc == _lib.RK_ERR_UNSUPPORTED and "dalton_grid" in msg and "left out" in msg, (rc, msg)
    rc, msg = _solve(_cfg(p=4), _lib.MODE_MV, 3)                          # the store form of the same shape ships
    assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)


@pytest.mark.parametrize("cfg", [_cfg(n_steps=0), _cfg(d=0), _cfg(p=0), _cfg(m=0)])
def test_library_calls_a_non_positive_size_invalid(cfg):
    for rc, msg in _both(cfg):
        assert rc == _lib.RK_ERR_INVALID and "dalton_grid" in msg, (rc, msg)


def test_library_calls_another_mode_or_a_missing_flag_invalid():
    for mode in (_lib.MODE_FILTER, 7, -1):
        rc, msg = _solve(_cfg(), mode)
        assert rc == _lib.RK_ERR_INVALID and "dalton_grid" in msg and "mode" in msg, (rc, msg)
    for rc, msg in _both(_cfg(flags=0)):
        assert rc == _lib.RK_ERR_INVALID and "dalton_grid" in msg and "RK_FLAG_BATCH_MINOR" in msg, (rc, msg)


@pytest.mark.parametrize("cfg", [_cfg(), _cfg(p=2), _cfg(p=6), _cfg(itg=_lib.INTERROGATE_RODEO), _cfg(itg=_lib.INTERROGATE_SCHOBER),
                                 _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=3), _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=5),
                                 _cfg(rhs=_lib.RHS_HIGHER_ORDER, d=1, p=6)])
def test_library_passes_a_served_configuration_on_to_the_argument_check(cfg):
    """A served configuration gets as far as the null handle: RK_ERR_INVALID about the arguments, not about the cfg."""
    for n_bobs in (1, 3):
        for rc, msg in _both(cfg, n_bobs):
            assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
    lib = _lib.load()
    assert lib.rk_dalton_grid_loglik(None, None, None, None, None, None, None, 1, 1, None, None) == _lib.RK_ERR_INVALID
    assert lib.rk_dalton_grid_solve(None, None, None, None, _lib.MODE_MV, None, None, None, None, 1, 1, None) == _lib.RK_ERR_INVALID


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
            assert rc == _lib.RK_ERR_UNSUPPORTED and "dalton_grid" in msg and "n_bstate" in msg, (rc, msg)
    for rc, msg in _both(_cfg(rhs=ode.rhs_id, p=min(p, 5), d=3)):         # another block count than the registration's
        assert rc == _lib.RK_ERR_UNSUPPORTED and "dalton_grid" in msg and "n_block" in msg, (rc, msg)
