"""
``solve_evidence_grid`` / ``solve_mv_dynamic_grid`` / ``solve_sim_dynamic_grid`` on the host (no GPU): the signatures and
re-exports, the refusals that come before any device work (``default_device`` patched to fail), a traced right-hand side among
them, and the library's refusals on the configuration alone (no handle, no pointers).
"""
import ctypes as C
import functools
import inspect
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd import _lib
from rodeo_amd.interrogate import interrogate_chkrebtii, interrogate_kramer, interrogate_rodeo
from test_grid_host import _cfg, _fhn, _fitz, no_device                      # noqa: F401  (the fixture)

GRID_ARGS = ["key", "ode_fun", "ode_weight", "ode_init", "t_grid", "interrogate", "prior_at", "kalman_type"]
EVIDENCE, DYNAMIC = ra.grid_calib.solve_evidence_grid, [ra.grid_calib.solve_mv_dynamic_grid, ra.grid_calib.solve_sim_dynamic_grid]
SOLVERS = [EVIDENCE] + DYNAMIC


def test_signatures_and_re_exports():
    assert ra.solve_evidence_grid is EVIDENCE
    assert ra.solve_mv_dynamic_grid is DYNAMIC[0] and ra.solve_sim_dynamic_grid is DYNAMIC[1]
    assert list(inspect.signature(EVIDENCE).parameters) == GRID_ARGS + ["params"]
    assert list(inspect.signature(EVIDENCE).parameters)[:-1] == list(inspect.signature(ra.solve_mv_grid).parameters)[:-1]
    for fn in DYNAMIC:
        sig = inspect.signature(fn)
        assert list(sig.parameters) == GRID_ARGS + ["scale_min", "params"]
        assert sig.parameters["scale_min"].default == 0.0
    for fn in SOLVERS:
        sig = inspect.signature(fn)
        assert sig.parameters["kalman_type"].default == "standard"
        assert sig.parameters["params"].kind is inspect.Parameter.VAR_KEYWORD
    for fn in DYNAMIC:                                                      # what scale[n, b] means on steps of different length
        doc = " ".join(fn.__doc__.split())
        assert "already carries" in doc and "compared across steps" in doc
    assert "evidence_scale" in EVIDENCE.__doc__ and "evidence_at" in EVIDENCE.__doc__ and "once per slot" in EVIDENCE.__doc__


# ---- refusals before any device work --------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("bad,word", [(np.zeros((3, 5)), "per-trajectory grids are not built"), ([0.0], "at least two"),
                                      ([0.0, np.nan, 1.0], "non-finite"), ([0.0, 0.5, 0.5], "strictly increasing")])
def test_a_bad_grid_is_refused(no_device, solver, bad, word):
    a = _fhn()
    a["t_grid"] = bad
    with pytest.raises(ValueError, match=word):
        solver(**a)


@pytest.mark.parametrize("solver", SOLVERS)
def test_kalman_types_that_are_not_served(no_device, solver):
    with pytest.raises(NotImplementedError, match="kalman_type"):
        solver(**_fhn(), kalman_type="nope")
    with pytest.raises(NotImplementedError, match="not built"):
        solver(**_fhn(), kalman_type="square-root")


@pytest.mark.parametrize("solver", SOLVERS)
def test_interrogate_chkrebtii_is_refused_with_its_reason(no_device, solver):
    a = _fhn()
    word = "scale law" if solver is EVIDENCE else "depends on the point"
    for itg in (interrogate_chkrebtii, functools.partial(interrogate_chkrebtii, kalman_type="standard")):
        a["interrogate"] = itg
        with pytest.raises(NotImplementedError, match=word):
            solver(**a)


@pytest.mark.parametrize("solver", SOLVERS)
def test_several_measurements_per_block_are_refused(no_device, solver):
    a = _fhn()
    a["ode_weight"] = np.concatenate([a["ode_weight"]] * 2, axis=1)
    with pytest.raises(NotImplementedError, match="n_bmeas"):
        solver(**a)


def _sized(d, p, ode):
    W = np.zeros((d, 1, p)); W[:, 0, min(1, p - 1)] = 1.0
    return dict(key=None, ode_fun=ode, ode_weight=W, ode_init=np.zeros((d, p)), t_grid=[0.0, 0.1, 0.3], interrogate=interrogate_rodeo,
                prior_at=lambda h: (np.tile(np.eye(p), (d, 1, 1)),) * 2, theta=np.ones(3))


@pytest.mark.parametrize("solver,d,p,word", [(EVIDENCE, 2, 1, "2..6"), (EVIDENCE, 2, 7, "2..6"), (EVIDENCE, 3, 6, "three or more blocks")] +
                         [(fn, d, p, w) for fn in DYNAMIC for d, p, w in ((2, 1, "2..5"), (2, 6, "2..5"), (3, 5, "three or more blocks"))])
def test_n_bstate_outside_the_range_is_refused(no_device, solver, d, p, word):
    with pytest.raises(NotImplementedError, match=word):
        solver(**_sized(d, p, ra.ode.fitzhugh_nagumo if d == 2 else ra.ode.lorenz63))


@pytest.mark.parametrize("solver", DYNAMIC)
@pytest.mark.parametrize("bad", [-1.0, np.nan, np.inf, "x"])
def test_a_bad_scale_min_is_refused(no_device, solver, bad):
    with pytest.raises(ValueError, match="scale_min"):
        solver(**_fhn(), scale_min=bad)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("result,word", [((np.zeros((2, 3, 3)), np.zeros((2, 4, 4))), "shape"), (None, "pair"),
                                         ((np.eye(3)[None].repeat(2, 0), np.full((2, 3, 3), np.nan)), "non-finite")])
def test_a_bad_prior_at_result_is_refused(no_device, solver, result, word):
    a = _fhn()
    a["prior_at"] = lambda h: result
    with pytest.raises(ValueError, match=word):
        solver(**a)


@pytest.mark.parametrize("solver", SOLVERS)
def test_prior_at_is_called_once_per_slot(no_device, solver):
    calls = []

    def later_batched(h):
        calls.append(h)
        Q, R = ra.ibm_init(h, 3, np.array([0.5, 0.3]))
        return (Q, R) if len(calls) == 1 else (Q, np.tile(R, (4, 1, 1, 1)))
    a = _fhn()
    a["prior_at"] = later_batched
    with pytest.raises(ValueError, match="batch"):
        solver(**a)
    assert len(calls) == 3                                                  # steps .1, .05, .15, .1: three slots


@pytest.mark.parametrize("solver", SOLVERS)
def test_shapes_and_block_counts_are_refused(no_device, solver):
    a = _fhn()
    a["ode_init"] = np.zeros((2, 4))
    with pytest.raises(ValueError):
        solver(**a)
    with pytest.raises(ValueError, match="n_block"):
        solver(**_fhn(ode=ra.ode.lorenz63))


@pytest.mark.parametrize("solver", SOLVERS)
def test_a_traced_right_hand_side_is_refused_the_same_way(no_device, solver):
    """The plain-Python ode_fun is traced on the host; the refusals still come before the device."""
    a = _fhn(ode=_fitz)
    a["t_grid"] = [0.0, 0.2, 0.1]
    with pytest.raises(ValueError, match="strictly increasing"):
        solver(**a)
    a = _fhn(ode=_fitz)
    a["interrogate"] = interrogate_chkrebtii
    with pytest.raises(NotImplementedError, match="chkrebtii"):
        solver(**a)
    a = _fhn(p=7, ode=_fitz)
    with pytest.raises(NotImplementedError, match="n_bstate"):
        solver(**a)


# ---- the library, on the configuration alone ---------------------------------------------------------------------------
def _evidence(cfg, mode=None, scale_min=None):
    lib = _lib.load()
    return lib.rk_solve_evidence_grid(None, C.byref(cfg), None, None, None, None, None), lib.rk_last_error().decode()


def _dynamic(cfg, mode=_lib.MODE_MV, scale_min=0.0):
    lib = _lib.load()
    return lib.rk_solve_dynamic_grid(None, C.byref(cfg), None, None, mode, None, scale_min, None, None), lib.rk_last_error().decode()


ENTRIES = [(_evidence, "evidence_grid"), (_dynamic, "dynamic_grid")]


@pytest.mark.parametrize("call,who", ENTRIES)
@pytest.mark.parametrize("cfg,word", [
    (_cfg(kalman=7), "kalman_type"), (_cfg(kalman=_lib.KALMAN_SQRT), "not built"), (_cfg(itg=9), "interrogate"),
    (_cfg(itg=_lib.INTERROGATE_CHKREBTII), "chkrebtii"), (_cfg(m=2), "n_bmeas"), (_cfg(p=1), "n_bstate"), (_cfg(p=7), "n_bstate"),
    (_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=6), "n_bstate"), (_cfg(rhs=_lib.RHS_LORENZ63, d=2), "n_block"), (_cfg(rhs=77), "rhs_id"),
    (_cfg(flags=_lib.FLAG_BATCH_MINOR | _lib.FLAG_STORE_PRED), "STORE_PRED"),
])
def test_library_refuses_what_is_not_served(call, who, cfg, word):
    rc, msg = call(cfg)
    assert rc == _lib.RK_ERR_UNSUPPORTED, (rc, msg)
    assert msg.startswith(who) and word in msg, msg


def test_library_ranges_differ_between_the_two_entries():
    for cfg, ev_ok, dyn_ok in ((_cfg(p=6), True, False), (_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=5), True, False),
                               (_cfg(p=5), True, True), (_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=4), True, True),
                               (_cfg(rhs=_lib.RHS_HIGHER_ORDER, d=1, p=6), True, False)):
        for (call, who), ok in zip(ENTRIES, (ev_ok, dyn_ok)):
            rc, msg = call(cfg)
            if ok:
                assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (who, rc, msg)
            else:
                assert rc == _lib.RK_ERR_UNSUPPORTED and msg.startswith(who) and "n_bstate" in msg, (who, rc, msg)


@pytest.mark.parametrize("call,who", ENTRIES)
def test_library_calls_a_bad_size_or_a_missing_flag_invalid(call, who):
    for cfg in (_cfg(n_steps=0), _cfg(d=0), _cfg(p=0), _cfg(m=0)):
        rc, msg = call(cfg)
        assert rc == _lib.RK_ERR_INVALID and msg.startswith(who), (rc, msg)
    rc, msg = call(_cfg(flags=0))
    assert rc == _lib.RK_ERR_INVALID and msg.startswith(who) and "RK_FLAG_BATCH_MINOR" in msg, (rc, msg)


def test_library_checks_mode_and_scale_min_of_the_dynamic_entry():
    for mode in (_lib.MODE_FILTER, 7):
        rc, msg = _dynamic(_cfg(), mode)
        assert rc == _lib.RK_ERR_INVALID and msg.startswith("dynamic_grid") and "mode" in msg, (rc, msg)
    for bad in (-1.0, float("nan"), float("inf")):
        rc, msg = _dynamic(_cfg(), scale_min=bad)
        assert rc == _lib.RK_ERR_INVALID and msg.startswith("dynamic_grid") and "scale_min" in msg, (rc, msg)
    lib = _lib.load()
    assert lib.rk_solve_dynamic_grid(None, None, None, None, _lib.MODE_MV, None, 0.0, None, None) == _lib.RK_ERR_INVALID
    assert lib.rk_solve_evidence_grid(None, None, None, None, None, None, None) == _lib.RK_ERR_INVALID


@pytest.mark.parametrize("call,who,pmax", [(_evidence, "evidence_grid", 6), (_dynamic, "dynamic_grid", 5)])
def test_library_serves_a_traced_right_hand_side_over_the_same_range(call, who, pmax):
    from rodeo_amd.trace import from_python
    for p, served in ((2, True), (pmax, True), (pmax + 1, False)):
        ode = from_python(_fitz, 2, p, theta=3)
        rc, msg = call(_cfg(rhs=ode.rhs_id, p=p))
        if served:
            assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
        else:
            assert rc == _lib.RK_ERR_UNSUPPORTED and msg.startswith(who) and "n_bstate" in msg, (rc, msg)
    rc, msg = call(_cfg(rhs=ode.rhs_id, p=4, d=3))                         # another block count than the registration's
    assert rc == _lib.RK_ERR_UNSUPPORTED and msg.startswith(who) and "n_block" in msg, (rc, msg)
