"""
``rodeo_amd.solve_sim_draws_grid`` and ``rodeo_amd.inference.dalton.solve_sim_draws_grid`` on the host (no GPU): the signatures and
the re-export, every refusal that comes before any device work (``default_device`` patched to fail), a traced right-hand side
among them, the rules for ``keep`` and ``n_draws``, and the library's refusals on the configuration alone (no handle, no
pointers) for both entry points, in the project's order: the configuration, then n_draws and n_keep, then the pointers.
"""
import ctypes as C
import functools
import inspect
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401
from rodeo_amd import _lib, grid_draws
from rodeo_amd.interrogate import interrogate_chkrebtii, interrogate_kramer

dmod = sys.modules["rodeo_amd.inference.dalton"]             # (rodeo_amd.inference.dalton, the attribute, is the function)
PLAIN, DALTON = ra.solve_sim_draws_grid, dmod.solve_sim_draws_grid
CALLS = [PLAIN, DALTON]
OBS = ["obs_data", "obs_times", "obs_weight", "obs_var"]
NAME = {PLAIN: "solve_sim_draws_grid", DALTON: "dalton.solve_sim_draws_grid"}


def test_signatures_and_the_re_export():
    assert ra.solve_sim_draws_grid is grid_draws.solve_sim_draws_grid
    assert not hasattr(ra.inference, "solve_sim_draws_grid")                     # DALTON's is imported from its module
    sig, dsig = inspect.signature(PLAIN), inspect.signature(DALTON)
    head = list(inspect.signature(ra.solve_sim_grid).parameters)[:7]
    assert head == ["key", "ode_fun", "ode_weight", "ode_init", "t_grid", "interrogate", "prior_at"]
    assert list(sig.parameters) == head + ["kalman_type", "n_draws", "keep", "params"]
    assert list(dsig.parameters) == head + OBS + ["kalman_type", "n_draws", "keep", "params"]
    assert list(dsig.parameters)[:12] == list(inspect.signature(dmod.solve_sim_grid).parameters)[:12]
    for s in (sig, dsig):
        assert s.parameters["kalman_type"].default == "standard"
        assert s.parameters["n_draws"].default == 1 and s.parameters["keep"].default is None
        assert s.parameters["params"].kind is inspect.Parameter.VAR_KEYWORD
    assert "draw_seed" in PLAIN.__doc__ and "ODE parameter" in PLAIN.__doc__ and "draw_seed" in DALTON.__doc__


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


def _args(call, p=3, times=(0.1, 0.3), **over):
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    theta = np.array([0.2, 0.2, 3.0])
    sigma = np.array([0.5, 0.3])
    a = dict(key=3, ode_fun=ra.ode.fitzhugh_nagumo, ode_weight=W, ode_init=init(np.array([-1.0, 1.0]), 0.0, theta=theta),
             t_grid=np.array([0.0, 0.1, 0.15, 0.3, 0.4]), interrogate=interrogate_kramer, prior_at=lambda h: ra.ibm_init(h, p, sigma),
             theta=theta)
    if call is DALTON:
        n = len(times)
        D = np.zeros((n, 2, 1, p))
        D[..., 0, 0] = 1.0
        a.update(obs_data=np.zeros((n, 2, 1)), obs_times=np.array(times, dtype=float), obs_weight=D,
                 obs_var=np.tile(0.01 * np.eye(1), (n, 2, 1, 1)))
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
    """(the fixture works: what is not refused does ask for a device) -- with a traced right-hand side too"""
    for over in (dict(), dict(n_draws=7, keep=[0, 2, 4]), dict(ode_fun=_fitz)):
        with pytest.raises(AssertionError, match="default_device was reached"):
            call(**_args(call, **over))


# ---- what grid._refusals refuses --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("t_grid,word", [(np.zeros((2, 3)), "1-D"), ([0.0], "two nodes"), ([0.0, np.nan, 1.0], "non-finite"),
                                         ([0.0, 0.2, 0.1, 0.3, 0.4], "strictly increasing")])
def test_a_bad_grid_is_refused(no_device, call, t_grid, word):
    with pytest.raises(ValueError, match=word):
        call(**_args(call, t_grid=t_grid, n_draws=2))


@pytest.mark.parametrize("call", CALLS)
def test_the_configurations_the_grid_solver_refuses(no_device, call):
    with pytest.raises(NotImplementedError):
        call(**_args(call, kalman_type="nope"))
    with pytest.raises(NotImplementedError, match="square-root"):
        call(**_args(call, kalman_type="square-root"))
    with pytest.raises(NotImplementedError, match="n_bmeas"):
        call(**_args(call, ode_weight=np.zeros((2, 2, 3))))
    with pytest.raises(NotImplementedError, match="n_bstate"):
        call(**_args(call, ode_weight=np.zeros((2, 1, 7))))
    with pytest.raises(ValueError, match="prior_at"):
        call(**_args(call, prior_at=3.0))
    with pytest.raises(ValueError, match="prior_at"):
        call(**_args(call, prior_at=lambda h: (np.zeros((2, 4, 4)), np.zeros((2, 4, 4)))))
    with pytest.raises(ValueError, match="non-finite"):
        call(**_args(call, prior_at=lambda h: (np.full((2, 3, 3), np.inf), np.zeros((2, 3, 3)))))
    with pytest.raises(ValueError):
        call(**_args(call, ode_init=np.zeros((2, 4))))
    with pytest.raises(TypeError):
        call(**_args(call, interrogate=lambda **k: None))


def test_three_blocks_stop_at_n_bstate_five(no_device):
    W, init = ra.utils.first_order_pad(ra.ode.lorenz63, 3, 6)
    theta = np.array([28.0, 10.0, 8.0 / 3.0])
    with pytest.raises(NotImplementedError, match="n_bstate up to 5 with three or more blocks.*6"):
        PLAIN(None, ra.ode.lorenz63, W, init(np.array([-12.0, -5.0, 38.0]), 0.0, theta=theta), [0.0, 0.1, 0.3], interrogate_kramer,
              lambda h: ra.ibm_init(h, 6, np.ones(3)), n_draws=3, theta=theta)


@pytest.mark.parametrize("call", CALLS)
def test_a_traced_right_hand_side_with_a_bad_argument_is_refused(no_device, call):
    """The refusals hold for a plain-Python right-hand side as well (it is traced on the host, without a device)."""
    with pytest.raises(ValueError, match="n_draws"):
        call(**_args(call, ode_fun=_fitz, n_draws=0))
    with pytest.raises(ValueError, match="keep"):
        call(**_args(call, ode_fun=_fitz, keep=[0, 5]))
    with pytest.raises(ValueError, match="strictly increasing"):
        call(**_args(call, ode_fun=_fitz, t_grid=[0.0, 0.2, 0.1]))


# ---- what draws._refusals refuses for the draws -----------------------------------------------------------------------------
@pytest.mark.parametrize("call", CALLS)
def test_chkrebtii_is_refused_with_the_reason(no_device, call):
    itg = functools.partial(interrogate_chkrebtii, kalman_type="standard")
    with pytest.raises(NotImplementedError, match="solve_sim_draws_grid: interrogate_chkrebtii.*depends on the key.*cannot share "
                                                  "one filter"):
        call(**_args(call, interrogate=itg, n_draws=4))


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("bad", [0, -3, 2.0, "4", None, True, 65536, np.array([2, 3])])
def test_n_draws_must_be_an_integer_from_one(no_device, call, bad):
    with pytest.raises(ValueError, match=NAME[call].replace(".", r"\.") + ": n_draws") as e:
        call(**_args(call, n_draws=bad))
    assert call is DALTON or not str(e.value).startswith("dalton")


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("bad,word", [
    ([[0, 1]], "1-D"), (3, "1-D"), ([0.0, 1.0], "integer"), ([True, False], "integer"), ([], "1-D|empty|integer"),
    (np.zeros(0, dtype=np.int64), "empty"),
    ([-1, 3], "0 .. n_steps"),                  # below the grid
    ([0, 5], "0 .. n_steps"),                   # N = 4: node 5 does not exist
    ([3, 3], "strictly increasing"), ([4, 2], "strictly increasing")])
def test_keep_must_be_strictly_increasing_node_indices(no_device, call, bad, word):
    with pytest.raises(ValueError, match=f"solve_sim_draws_grid: keep.*({word})"):
        call(**_args(call, keep=bad))


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("keep", [[0], [4], [0, 4], [1], [1, 2, 3], list(range(5)), np.array([0, 4], dtype=np.uint8), None])
def test_a_good_keep_and_n_draws_pass(no_device, call, keep):
    for n_draws in (1, 65535, np.int64(3)):
        with pytest.raises(AssertionError, match="default_device was reached"):
            call(**_args(call, keep=keep, n_draws=n_draws))


# ---- what dalton's _on_grid refuses ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("times,word", [
    ((0.1, 0.2), "0.2 is no node"), ((0.3, 0.1), "strictly increasing"), ((0.1, 0.1 + 0.5e-11 * 0.05), "same node"),
    ((0.1, np.nan), "non-finite"), ((0.1, 0.41), "inside the grid")])
def test_dalton_refuses_bad_observation_times(no_device, times, word):
    with pytest.raises(ValueError, match=word) as e:
        DALTON(**_args(DALTON, times=times, n_draws=2))
    assert "dalton.solve_sim_draws_grid" in str(e.value)


def test_dalton_refuses_bad_observations(no_device):
    with pytest.raises(ValueError, match="grid_with_times"):
        DALTON(**_args(DALTON, times=(0.1, 0.2)))
    with pytest.raises(ValueError, match="shape"):
        DALTON(**_args(DALTON, obs_times=np.array([0.1])))
    with pytest.raises(NotImplementedError, match="n_bobs"):
        DALTON(**_args(DALTON, obs_weight=np.zeros((2, 2, 4, 3)), obs_data=np.zeros((2, 2, 4)),
                       obs_var=np.tile(np.eye(4), (2, 2, 1, 1))))
    with pytest.raises(ValueError, match="obs_weight"):
        DALTON(**_args(DALTON, obs_weight=np.zeros((2, 2, 1, 4))))


# ---- the library, on the configuration alone ---------------------------------------------------------------------------
def _cfg(rhs=_lib.RHS_FITZHUGH_NAGUMO, d=2, p=3, m=1, itg=_lib.INTERROGATE_KRAMER, kalman=_lib.KALMAN_STANDARD, n_steps=50,
         flags=_lib.FLAG_BATCH_MINOR):
    return _lib.SolveCfg(n_traj=16, n_steps=n_steps, n_block=d, n_bstate=p, n_bmeas=m, rhs_id=rhs, interrogate=itg,
                         kalman_type=kalman, n_theta=3, flags=flags, t_min=0.0, t_max=1.0, seed=0, traj_offset=0)


def _plain(cfg, n_draws=4, n_keep=0, keep=None, n_bobs=None):
    """rk_solve_sim_draws_grid with no handle and no pointers: only the configuration, n_draws and n_keep can be looked at."""
    lib = _lib.load()
    rc = lib.rk_solve_sim_draws_grid(None, C.byref(cfg), None, None, None, n_draws, keep, n_keep, None)
    return rc, lib.rk_last_error().decode()


def _dalton(cfg, n_draws=4, n_keep=0, keep=None, n_bobs=1):
    lib = _lib.load()
    rc = lib.rk_dalton_grid_sim_draws(None, C.byref(cfg), None, None, None, None, None, None, 3, n_bobs, None, n_draws, keep, n_keep,
                                      None)
    return rc, lib.rk_last_error().decode()


ENTRIES = [_plain, _dalton]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("cfg,word", [
    (_cfg(itg=_lib.INTERROGATE_CHKREBTII), "chkrebtii"),
    (_cfg(itg=_lib.INTERROGATE_CHKREBTII), "cannot share one filter"),
    (_cfg(kalman=_lib.KALMAN_SQRT), "not built"),
    (_cfg(kalman=7), "kalman_type"),
    (_cfg(itg=9), "interrogate"),
    (_cfg(m=2), "n_bmeas"),
    (_cfg(p=1), "n_bstate"),
    (_cfg(p=7), "n_bstate"),
    (_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=6), "three or more blocks"),
    (_cfg(flags=_lib.FLAG_BATCH_MINOR | _lib.FLAG_STORE_PRED), "RK_FLAG_STORE_PRED"),
    (_cfg(rhs=_lib.RHS_LORENZ63, d=2), "n_block"),
    (_cfg(rhs=77), "rhs_id"),
])
def test_library_refuses_what_is_not_served(entry, cfg, word):
    rc, msg = entry(cfg)
    assert rc == _lib.RK_ERR_UNSUPPORTED, (rc, msg)
    assert "grid_draws" in msg and word in msg, msg


@pytest.mark.parametrize("n_bobs", [0, 4, -1])
def test_library_refuses_n_bobs_outside_one_to_three(n_bobs):
    rc, msg = _dalton(_cfg(), n_bobs=n_bobs)
    assert rc == _lib.RK_ERR_UNSUPPORTED and "grid_draws" in msg and "n_bobs" in msg, (rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("cfg", [_cfg(n_steps=0), _cfg(d=0), _cfg(p=0), _cfg(m=0)])
def test_library_calls_a_non_positive_size_invalid(entry, cfg):
    rc, msg = entry(cfg)
    assert rc == _lib.RK_ERR_INVALID and "grid_draws" in msg, (rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_library_needs_the_batch_minor_records(entry):
    for flags in (0, _lib.FLAG_STORE_PRED):
        rc, msg = entry(_cfg(flags=flags))
        assert rc == _lib.RK_ERR_INVALID and "grid_draws" in msg and "RK_FLAG_BATCH_MINOR" in msg, (rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n_draws", [0, -1, 65536])
def test_library_calls_a_bad_n_draws_invalid(entry, n_draws):
    rc, msg = entry(_cfg(), n_draws=n_draws)
    assert rc == _lib.RK_ERR_INVALID and "grid_draws" in msg and "n_draws" in msg, (rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n_keep", [0, -2, 52])
def test_library_calls_a_bad_n_keep_invalid(entry, n_keep):
    """With a `keep` array n_keep must lie in 1 .. n_steps + 1 (the pointer itself is not read on the host)."""
    rc, msg = entry(_cfg(n_steps=50), n_keep=n_keep, keep=C.c_void_p(8))
    assert rc == _lib.RK_ERR_INVALID and "grid_draws" in msg and "n_keep" in msg, (rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_configuration_is_looked_at_before_the_counts(entry):
    rc, msg = entry(_cfg(p=7), n_draws=0)
    assert rc == _lib.RK_ERR_UNSUPPORTED and "n_bstate" in msg, (rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("cfg", [_cfg(), _cfg(p=2), _cfg(p=6), _cfg(itg=_lib.INTERROGATE_RODEO), _cfg(itg=_lib.INTERROGATE_SCHOBER),
                                 _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=3), _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=5),
                                 _cfg(rhs=_lib.RHS_HIGHER_ORDER, d=1, p=4)])
def test_library_passes_a_served_configuration_on_to_the_argument_check(entry, cfg):
    """A served configuration gets as far as the null handle: RK_ERR_INVALID about the arguments, not about the cfg."""
    for n_keep, keep in ((0, None), (51, C.c_void_p(8)), (1, C.c_void_p(8))):
        rc, msg = entry(cfg, n_keep=n_keep, keep=keep)
        assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
    for n_bobs in (1, 2, 3):
        rc, msg = entry(cfg, n_bobs=n_bobs)
        assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)


def test_a_null_cfg_is_invalid():
    lib = _lib.load()
    assert lib.rk_solve_sim_draws_grid(None, None, None, None, None, 1, None, 0, None) == _lib.RK_ERR_INVALID
    assert lib.rk_dalton_grid_sim_draws(None, None, None, None, None, None, None, None, 0, 1, None, 1, None, 0, None) == _lib.RK_ERR_INVALID


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("p,served", [(2, True), (6, True), (7, False)])
def test_library_serves_a_traced_right_hand_side_over_the_same_range(entry, p, served):
    from rodeo_amd.trace import from_python
    ode = from_python(_fitz, 2, min(p, 6), theta=3)
    rc, msg = entry(_cfg(rhs=ode.rhs_id, p=p))
    if served:
        assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
    else:
        assert rc == _lib.RK_ERR_UNSUPPORTED and "grid_draws" in msg and "n_bstate" in msg, (rc, msg)
    rc, msg = entry(_cfg(rhs=ode.rhs_id, p=min(p, 4), d=3))                # another block count than the registration's
    assert rc == _lib.RK_ERR_UNSUPPORTED and "grid_draws" in msg and "n_block" in msg, (rc, msg)
