"""
``solve_mv_grid`` / ``solve_sim_grid`` on the host (no GPU): the signatures and re-exports, the slot rule on hand-made grids, the
refusals that come before any device work (``default_device`` patched to fail), and the library's refusals on the configuration
alone (no handle, no pointers), a traced right-hand side among them.
"""
import ctypes as C
import inspect
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd import _lib
from rodeo_amd.interrogate import interrogate_kramer, interrogate_rodeo

GRID_ARGS = ["key", "ode_fun", "ode_weight", "ode_init", "t_grid", "interrogate", "prior_at", "kalman_type", "params"]
SOLVERS = [ra.grid.solve_mv_grid, ra.grid.solve_sim_grid]


def test_signature_and_re_export():
    assert ra.solve_mv_grid is ra.grid.solve_mv_grid and ra.solve_sim_grid is ra.grid.solve_sim_grid
    assert ra.grid_slots is ra.grid.grid_slots
    for fn in SOLVERS:
        sig = inspect.signature(fn)
        assert list(sig.parameters) == GRID_ARGS
        assert list(sig.parameters)[:4] == list(inspect.signature(ra.solve_mv).parameters)[:4]
        assert sig.parameters["kalman_type"].default == "standard"
        assert sig.parameters["params"].kind is inspect.Parameter.VAR_KEYWORD
    doc = ra.solve_mv_grid.__doc__
    assert "N times on the host" in doc and "once per slot" in doc      # what a fully irregular grid costs
    assert ctypes_size_ok()


def ctypes_size_ok():
    return C.sizeof(_lib.GridIn) == 4 * 8 + 3 * 4 + 4                  # four pointers, three int32, tail padding


# ---- the slot rule ------------------------------------------------------------------------------------------------------
def test_grid_slots_on_hand_made_grids():
    h_rep, slot = ra.grid_slots([0.0, 0.1, 0.15, 0.2, 0.3, 0.5])
    assert slot.dtype == np.int32 and list(slot) == [0, 1, 1, 0, 2]
    np.testing.assert_allclose(h_rep, [0.1, 0.05, 0.2], rtol=1e-12)
    assert h_rep[1] == 0.15 - 0.1                                       # the representative is the step that opened the slot
    h_rep, slot = ra.grid_slots(np.array([1.0, 3.0]))
    assert list(h_rep) == [2.0] and list(slot) == [0]
    for t_max, n in ((4.0, 73), (40.0, 801), (1.0, 11)):
        h_rep, slot = ra.grid_slots(np.linspace(0.0, t_max, n))
        assert len(h_rep) == 1 and not slot.any()
    t = np.concatenate([[0.0], np.cumsum(2.0 ** np.random.default_rng(0).uniform(-1, 1, 30))])
    h_rep, slot = ra.grid_slots(t)
    assert list(slot) == list(range(30)) and np.array_equal(h_rep, np.diff(t))


def test_grid_slots_tolerance_is_relative_to_the_longest_step():
    h = 0.25
    near = ra.grid_slots(np.cumsum([0.0, h, h * (1 + 5e-13), 1.0]))[1]       # within 1e-12 of the longest step, 1.0
    far = ra.grid_slots(np.cumsum([0.0, h, h * (1 + 1e-11), 1.0]))[1]
    assert list(near) == [0, 0, 1] and list(far) == [0, 1, 2]


@pytest.mark.parametrize("bad,word", [(np.zeros((2, 5)), "per-trajectory grids are not built"), ([0.0], "at least two"), ([], "at least two"),
                                      ([0.0, np.nan, 1.0], "non-finite"), ([0.0, np.inf], "non-finite"),
                                      ([0.0, 0.5, 0.5, 1.0], "strictly increasing"), ([0.0, 1.0, 0.5], "strictly increasing"),
                                      (1.0, "1-D")])
def test_grid_slots_refuses_a_bad_grid(bad, word):
    with pytest.raises(ValueError, match=word):
        ra.grid_slots(bad)


# ---- refusals before any device work --------------------------------------------------------------------------------------
def _fhn(p=3, ode=ra.ode.fitzhugh_nagumo, sigma=np.array([0.5, 0.3])):
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    theta = np.array([0.2, 0.2, 3.0])
    x0 = init(np.array([-1.0, 1.0]), 0.0, theta=theta)
    return dict(key=None, ode_fun=ode, ode_weight=W, ode_init=x0, t_grid=np.array([0.0, 0.1, 0.15, 0.3, 0.4]),
                interrogate=interrogate_kramer, prior_at=lambda h: ra.ibm_init(h, p, sigma), theta=theta)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device fails the test: the refusals below come first."""
    def fail(*a, **k):
        raise AssertionError("default_device was reached")
    monkeypatch.setattr(ra.device, "default_device", fail)
    monkeypatch.setattr(ra.solve, "default_device", fail)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("bad,word", [(np.zeros((3, 5)), "per-trajectory grids are not built"), ([0.0], "at least two"),
                                      ([0.0, np.nan, 1.0], "non-finite"), ([0.0, 0.5, 0.5], "strictly increasing"),
                                      ([1.0, 0.0], "strictly increasing")])
def test_a_bad_grid_is_refused(no_device, solver, bad, word):
    a = _fhn()
    a["t_grid"] = bad
    with pytest.raises(ValueError, match=word):
        solver(**a)


@pytest.mark.parametrize("solver", SOLVERS)
def test_unknown_kalman_type_is_refused(no_device, solver):
    with pytest.raises(NotImplementedError, match="kalman_type"):
        solver(**_fhn(), kalman_type="nope")


@pytest.mark.parametrize("solver", SOLVERS)
def test_the_square_root_form_is_not_built(no_device, solver):
    with pytest.raises(NotImplementedError, match="not built"):
        solver(**_fhn(), kalman_type="square-root")


@pytest.mark.parametrize("solver", SOLVERS)
def test_several_measurements_per_block_are_refused(no_device, solver):
    a = _fhn()
    a["ode_weight"] = np.concatenate([a["ode_weight"]] * 2, axis=1)         # n_bmeas = 2 (the dense / indep_init form)
    with pytest.raises(NotImplementedError, match="n_bmeas"):
        solver(**a)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("p", [1, 7, 8])
def test_n_bstate_outside_two_to_six_is_refused(no_device, solver, p):
    W = np.zeros((2, 1, p)); W[:, 0, min(1, p - 1)] = 1.0
    a = _fhn()
    a.update(ode_weight=W, ode_init=np.zeros((2, p)), prior_at=lambda h: (np.tile(np.eye(p), (2, 1, 1)),) * 2)
    with pytest.raises(NotImplementedError, match="n_bstate"):
        solver(**a)


@pytest.mark.parametrize("solver", SOLVERS)
def test_three_blocks_stop_at_five(no_device, solver):
    W = np.zeros((3, 1, 6)); W[:, 0, 1] = 1.0
    a = dict(key=None, ode_fun=ra.ode.lorenz63, ode_weight=W, ode_init=np.zeros((3, 6)), t_grid=[0.0, 0.1, 0.3],
             interrogate=interrogate_rodeo, prior_at=lambda h: (np.tile(np.eye(6), (3, 1, 1)),) * 2, theta=np.array([28.0, 10.0, 8 / 3]))
    with pytest.raises(NotImplementedError, match="three or more blocks"):
        solver(**a)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("result,word", [
    ((np.zeros((2, 3, 3)), np.zeros((2, 4, 4))), "shape"),                  # a matrix of the wrong shape
    ((np.zeros((3, 3)), np.zeros((3, 3))), "shape"),                        # rank
    (None, "pair"),                                                         # not a pair
    ((np.eye(3)[None].repeat(2, 0), np.full((2, 3, 3), np.nan)), "non-finite"),
    ((np.full((2, 3, 3), np.inf), np.eye(3)[None].repeat(2, 0)), "non-finite"),
])
def test_a_bad_prior_at_result_is_refused(no_device, solver, result, word):
    a = _fhn()
    a["prior_at"] = lambda h: result
    with pytest.raises(ValueError, match=word):
        solver(**a)


@pytest.mark.parametrize("solver", SOLVERS)
def test_prior_at_is_called_once_per_slot_and_batches_must_agree(no_device, solver):
    calls = []

    def later_batched(h):                                                   # slot 0 unbatched, a later slot with a batch of 4
        calls.append(h)
        Q, R = ra.ibm_init(h, 3, np.array([0.5, 0.3]))
        return (Q, R) if len(calls) == 1 else (Q, np.tile(R, (4, 1, 1, 1)))
    a = _fhn()
    a["prior_at"] = later_batched
    with pytest.raises(ValueError, match="batch"):
        solver(**a)
    assert len(calls) == 3                                                  # steps .1, .05, .15, .1: three slots
    a = _fhn(sigma=np.array([[0.5, 0.3]] * 4))                              # a batched sigma (4) against a batched theta (5)
    a["theta"] = np.tile(a["theta"], (5, 1))
    with pytest.raises(ValueError, match="batch"):
        solver(**a)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("change", [
    dict(ode_weight=np.zeros((1, 3))),                                      # rank
    dict(ode_init=np.zeros((2, 4))),                                        # ode_init against ode_weight
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


# ---- the library, on the configuration alone ---------------------------------------------------------------------------
def _cfg(rhs=_lib.RHS_FITZHUGH_NAGUMO, d=2, p=3, m=1, itg=_lib.INTERROGATE_KRAMER, kalman=_lib.KALMAN_STANDARD, n_steps=50,
         flags=_lib.FLAG_BATCH_MINOR):
    return _lib.SolveCfg(n_traj=16, n_steps=n_steps, n_block=d, n_bstate=p, n_bmeas=m, rhs_id=rhs, interrogate=itg,
                         kalman_type=kalman, n_theta=3, flags=flags, t_min=0.0, t_max=1.0, seed=0, traj_offset=0)


def _call(cfg, mode=_lib.MODE_MV):
    """rk_solve_grid with no handle and no pointers: only the configuration and the mode can be looked at."""
    lib = _lib.load()
    rc = lib.rk_solve_grid(None, C.byref(cfg), None, None, mode, None)
    return rc, lib.rk_last_error().decode()


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
    for mode in (_lib.MODE_MV, _lib.MODE_SIM):
        rc, msg = _call(cfg, mode)
        assert rc == _lib.RK_ERR_UNSUPPORTED, (rc, msg)
        assert "grid" in msg and word in msg, msg


@pytest.mark.parametrize("cfg", [_cfg(n_steps=0), _cfg(d=0), _cfg(p=0), _cfg(m=0)])
def test_library_calls_a_non_positive_size_invalid(cfg):
    rc, msg = _call(cfg)
    assert rc == _lib.RK_ERR_INVALID and "grid" in msg, (rc, msg)


def test_library_calls_another_mode_or_a_missing_flag_invalid():
    for mode in (_lib.MODE_FILTER, 7):
        rc, msg = _call(_cfg(), mode)
        assert rc == _lib.RK_ERR_INVALID and "grid" in msg and "mode" in msg, (rc, msg)
    rc, msg = _call(_cfg(flags=0))
    assert rc == _lib.RK_ERR_INVALID and "grid" in msg and "RK_FLAG_BATCH_MINOR" in msg, (rc, msg)


@pytest.mark.parametrize("cfg", [_cfg(), _cfg(p=2), _cfg(p=6), _cfg(itg=_lib.INTERROGATE_RODEO), _cfg(itg=_lib.INTERROGATE_SCHOBER),
                                 _cfg(itg=_lib.INTERROGATE_CHKREBTII), _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=3),
                                 _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=5), _cfg(rhs=_lib.RHS_HIGHER_ORDER, d=1, p=6)])
def test_library_passes_a_served_configuration_on_to_the_argument_check(cfg):
    """A served configuration gets as far as the null handle: RK_ERR_INVALID about the arguments, not about the cfg."""
    for mode in (_lib.MODE_MV, _lib.MODE_SIM):
        rc, msg = _call(cfg, mode)
        assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
    assert _lib.load().rk_solve_grid(None, None, None, None, _lib.MODE_MV, None) == _lib.RK_ERR_INVALID


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


@pytest.mark.parametrize("p,served", [(2, True), (6, True), (7, False)])
def test_library_serves_a_traced_right_hand_side_over_the_same_range(p, served):
    from rodeo_amd.trace import from_python
    ode = from_python(_fitz, 2, p, theta=3)
    rc, msg = _call(_cfg(rhs=ode.rhs_id, p=p))
    if served:
        assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
    else:
        assert rc == _lib.RK_ERR_UNSUPPORTED and "grid" in msg and "n_bstate" in msg, (rc, msg)
    rc, msg = _call(_cfg(rhs=ode.rhs_id, p=min(p, 5), d=3))                # another block count than the registration's
    assert rc == _lib.RK_ERR_UNSUPPORTED and "grid" in msg and "n_block" in msg, (rc, msg)
