"""
DALTON's public interface on the host (no GPU): the reference's signatures, the refusals that come before any device work,
and the layout that rk_dalton_layout reports for each configuration (src/rodeo/inference/dalton.py:39-545).
"""
import ctypes as C
import functools
import inspect
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd import _lib
import rodeo_amd.inference.dalton  # noqa: F401  (the module; the package attribute `dalton` is the function)
import sys
dalton_mod = sys.modules["rodeo_amd.inference.dalton"]
from rodeo_amd.interrogate import interrogate_kramer, interrogate_rodeo, interrogate_schober, interrogate_chkrebtii

REF_ARGS = ["key", "ode_fun", "ode_weight", "ode_init", "t_min", "t_max", "n_steps", "interrogate", "prior_pars",
            "obs_data", "obs_times", "obs_weight", "obs_var", "kalman_type", "params"]


def test_api_has_the_reference_signature():
    assert ra.inference.dalton is dalton_mod.dalton
    for fn in (dalton_mod.dalton, dalton_mod.solve_mv, dalton_mod.solve_sim):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == REF_ARGS, fn.__name__
        assert sig.parameters["kalman_type"].default == "standard"
        assert sig.parameters["params"].kind is inspect.Parameter.VAR_KEYWORD
    assert not hasattr(ra.inference, "daltonng")


def _fhn(p=3, n_obs=5, n_bobs=1, N=40, t_max=4.0):
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    theta = np.array([0.2, 0.2, 3.0])
    x0 = init(np.array([-1.0, 1.0]), 0.0, theta=theta)
    prior = ra.ibm_init(t_max / N, p, np.array([0.1, 0.1]))
    obs_times = np.linspace(0.5, t_max, n_obs)
    D = np.zeros((n_obs, 2, n_bobs, p))
    for j in range(n_bobs):
        D[:, :, j, j] = 1.0
    obs = dict(obs_data=np.zeros((n_obs, 2, n_bobs)), obs_times=obs_times, obs_weight=D,
               obs_var=np.tile(0.1 * np.eye(n_bobs), (n_obs, 2, 1, 1)))
    return dict(key=None, ode_fun=ra.ode.fitzhugh_nagumo, ode_weight=W, ode_init=x0, t_min=0.0, t_max=t_max, n_steps=N,
                interrogate=interrogate_kramer, prior_pars=prior, theta=theta, **obs)


FUNS = [dalton_mod.dalton, dalton_mod.solve_mv, dalton_mod.solve_sim]


@pytest.mark.parametrize("fn", FUNS)
def test_unknown_kalman_type_is_refused(fn):
    with pytest.raises(NotImplementedError):
        fn(**_fhn(), kalman_type="nope")


@pytest.mark.parametrize("fn", FUNS)
def test_square_root_is_refused_as_not_built(fn):
    with pytest.raises(NotImplementedError, match="not built"):
        fn(**_fhn(), kalman_type="square-root")


@pytest.mark.parametrize("fn", FUNS)
def test_chkrebtii_is_refused(fn):
    a = _fhn()
    a["interrogate"] = functools.partial(interrogate_chkrebtii, kalman_type="standard")
    with pytest.raises(NotImplementedError, match="chkrebtii"):
        fn(**a)


@pytest.mark.parametrize("fn", FUNS)
def test_several_measurements_per_block_are_refused(fn):
    a = _fhn()
    a["ode_weight"] = np.concatenate([a["ode_weight"]] * 2, axis=1)         # n_bmeas = 2 (the dense / indep_init form)
    with pytest.raises(NotImplementedError, match="n_bmeas"):
        fn(**a)


@pytest.mark.parametrize("fn", FUNS)
@pytest.mark.parametrize("p", [7, 8])
def test_n_bstate_outside_the_lane_kernels_is_refused(fn, p):
    with pytest.raises(NotImplementedError, match="n_bstate"):
        fn(**_fhn(p=p))


@pytest.mark.parametrize("fn", FUNS)
def test_four_observations_per_block_are_refused(fn):
    a = _fhn(p=4)
    D = np.zeros((5, 2, 4, 4))
    a.update(obs_data=np.zeros((5, 2, 4)), obs_weight=D, obs_var=np.tile(np.eye(4), (5, 2, 1, 1)))
    with pytest.raises(NotImplementedError, match="n_bobs"):
        fn(**a)


@pytest.mark.parametrize("fn", FUNS)
@pytest.mark.parametrize("times", [[1.0, 1.0, 2.0], [2.0, 1.0, 3.0], [0.95, 1.0, 3.0]])
def test_grid_indices_must_increase_strictly(fn, times):
    a = _fhn(n_obs=3)                                              # grid step 0.1: 0.95 and 1.0 share index 10
    a["obs_times"] = np.array(times)
    with pytest.raises(ValueError, match="strictly increasing"):
        fn(**a)


def test_observations_past_t_max_need_not_be_distinct():
    """Grid indices above n_steps never match (in the reference either): only those on the grid must increase strictly."""
    a = _fhn(n_obs=4)
    a["obs_times"] = np.array([1.0, 2.0, 4.5, 5.0])                # t_max = 4: the last two both map to index n_steps + 1
    *_, ind = dalton_mod._refusals(a["ode_weight"], a["interrogate"], "standard", a["obs_data"], a["obs_weight"],
                                   a["obs_var"], a["t_min"], a["t_max"], a["n_steps"], a["obs_times"])
    assert list(ind) == [10, 20, 41, 41]


def _cfg(rhs=_lib.RHS_FITZHUGH_NAGUMO, d=2, p=3, m=1, itg=_lib.INTERROGATE_KRAMER, kalman=_lib.KALMAN_STANDARD, flags=0):
    return _lib.SolveCfg(n_traj=16, n_steps=50, n_block=d, n_bstate=p, n_bmeas=m, rhs_id=rhs, interrogate=itg,
                         kalman_type=kalman, n_theta=3, flags=flags, t_min=0.0, t_max=1.0, seed=0, traj_offset=0)


def _layout(cfg, n_bobs=1, mode=_lib.MODE_MV):
    lay = C.c_int32(-1)
    rc = _lib.load().rk_dalton_layout(C.byref(cfg), mode, n_bobs, C.byref(lay))
    return rc, lay.value


@pytest.mark.parametrize("mode", [_lib.MODE_FILTER, _lib.MODE_MV, _lib.MODE_SIM])
@pytest.mark.parametrize("itg", [_lib.INTERROGATE_KRAMER, _lib.INTERROGATE_RODEO, _lib.INTERROGATE_SCHOBER])
@pytest.mark.parametrize("p,n_bobs", [(3, 2), (3, 3), (2, 1), (4, 1), (5, 2), (6, 3)])
def test_layout_is_batch_minor_on_the_lane_route(mode, itg, p, n_bobs):
    assert _layout(_cfg(p=p, itg=itg), n_bobs, mode) == (_lib.RK_OK, _lib.LAYOUT_BATCH_MINOR)


@pytest.mark.parametrize("mode", [_lib.MODE_FILTER, _lib.MODE_MV, _lib.MODE_SIM])
@pytest.mark.parametrize("itg", [_lib.INTERROGATE_KRAMER, _lib.INTERROGATE_RODEO, _lib.INTERROGATE_SCHOBER])
@pytest.mark.parametrize("flags", [0, _lib.FLAG_BATCH_MINOR])
def test_layout_is_tile3_on_the_tile_route(mode, itg, flags):
    """FitzHugh-Nagumo at p = 3 with one observation per block: the MFMA-tile records, whatever the caller's flags."""
    assert _layout(_cfg(p=3, itg=itg, flags=flags), 1, mode) == (_lib.RK_OK, _lib.LAYOUT_TILE3)


def test_rk_dalton_lanes_forces_the_lane_route(monkeypatch):
    monkeypatch.setenv("RK_DALTON_LANES", "1")
    assert _layout(_cfg(p=3), 1) == (_lib.RK_OK, _lib.LAYOUT_BATCH_MINOR)
    monkeypatch.setenv("RK_DALTON_LANES", "0")
    assert _layout(_cfg(p=3), 1) == (_lib.RK_OK, _lib.LAYOUT_TILE3)


def test_layout_other_built_in_right_hand_sides():
    assert _layout(_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=3)) == (_lib.RK_OK, _lib.LAYOUT_TILE3)
    assert _layout(_cfg(rhs=_lib.RHS_HIGHER_ORDER, d=1, p=3)) == (_lib.RK_OK, _lib.LAYOUT_TILE3)
    assert _layout(_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=3), 2) == (_lib.RK_OK, _lib.LAYOUT_BATCH_MINOR)
    assert _layout(_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=5)) == (_lib.RK_OK, _lib.LAYOUT_BATCH_MINOR)
    assert _layout(_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=6))[0] == _lib.RK_ERR_UNSUPPORTED


@pytest.mark.parametrize("cfg,n_bobs", [
    (_cfg(kalman=_lib.KALMAN_SQRT), 1),
    (_cfg(itg=_lib.INTERROGATE_CHKREBTII), 1),
    (_cfg(p=7), 1),
    (_cfg(m=2), 1),
    (_cfg(), 4),
    (_cfg(rhs=_lib.RHS_LORENZ63, d=2), 1),
])
def test_layout_refuses_what_is_not_served(cfg, n_bobs):
    rc, _ = _layout(cfg, n_bobs)
    assert rc == _lib.RK_ERR_UNSUPPORTED
    assert b"dalton" in _lib.load().rk_last_error()
