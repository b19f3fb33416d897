"""
Host side of ``rodeo_amd.solve_mv_at`` (the solver's posterior at arbitrary times) and of rk_eval_at: the signature, where the
evaluation times sit on the grid, the consistency check of ``prior_at`` and every refusal -- none of it needs a device.
"""
import ctypes as C
import inspect
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.solve as solve
from rodeo_amd import _lib
from rodeo_amd.interrogate import interrogate_kramer

THETA = np.array([0.2, 0.2, 3.0])
N, T_MAX = 40, 4.0
DT = T_MAX / N


def _case(p=3, sigma=0.1):
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    sig = np.full(2, sigma)
    return dict(W=W, x0=init(np.array([-1.0, 1.0]), 0.0, theta=THETA), prior=ra.ibm_init(DT, p, sig),
                prior_at=lambda h: ra.ibm_init(h, p, sig))


def _call(c, t_eval, ode=ra.ode.fitzhugh_nagumo, **kw):
    kw = {"theta": THETA, **kw}
    return ra.solve_mv_at(None, ode, c["W"], c["x0"], 0.0, T_MAX, N, interrogate_kramer, c["prior"], t_eval, c["prior_at"], **kw)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(solve, "default_device", lambda *a, **k: pytest.fail("a device was asked for"))


def test_signature():
    assert ra.solve_mv_at is solve.solve_mv_at
    sig = inspect.signature(ra.solve_mv_at)
    assert list(sig.parameters) == list(inspect.signature(ra.solve_mv).parameters)[:9] + ["t_eval", "prior_at", "kalman_type",
                                                                                         "params"]
    assert sig.parameters["kalman_type"].default == "standard"
    assert sig.parameters["params"].kind is inspect.Parameter.VAR_KEYWORD


def test_times_on_and_off_the_grid():
    t = np.array([T_MAX, 0.0, 0.25 * DT, 7 * DT + 0.9e-10 * DT, 7 * DT + 1e-3 * DT, 39.5 * DT, 12 * DT - 0.5e-10 * DT])
    node, on, h1, h2 = solve.eval_at_nodes(t, 0.0, T_MAX, N)
    assert node.tolist() == [N, 0, 0, 7, 7, 39, 12] and on.tolist() == [True, True, False, True, False, False, True]
    assert np.all(h1[on] == 0) and np.all(h2[on] == 0)
    np.testing.assert_allclose(h1[~on], [0.25 * DT, 1e-3 * DT, 0.5 * DT], rtol=1e-9)
    np.testing.assert_allclose(h1[~on] + h2[~on], DT, rtol=1e-14)


def test_refused_times(no_device):
    c = _case()
    for bad, what in (([-1e-3, 1.0], "lie in"), ([1.0, T_MAX + 1e-6], "lie in"), ([1.0, np.nan], "non-finite"),
                      ([np.inf], "non-finite"), ([], "non-empty"), ([[1.0, 2.0]], "non-empty")):
        with pytest.raises(ValueError, match=what):
            _call(c, np.array(bad, dtype=float))


def test_refused_configurations(no_device):
    t = np.array([0.33, 1.0])
    with pytest.raises(NotImplementedError, match="not built"):
        _call(_case(), t, kalman_type="square-root")
    with pytest.raises(NotImplementedError):
        _call(_case(), t, kalman_type="other")
    for p in (6, 7):
        with pytest.raises(NotImplementedError, match="n_bstate"):
            _call(_case(p=p), t)
    # the dense / indep_init route keeps trajectory-major records
    A = np.array([[-1.0, 0.2], [0.0, -0.5]])
    Qd, Rd = ra.indep_init(ra.ibm_init(DT, 2, np.array([0.1, 0.1])))
    dense = dict(W=np.zeros((1, 2, 4)), x0=np.zeros((1, 4)), prior=(Qd, Rd),
                 prior_at=lambda h: ra.indep_init(ra.ibm_init(h, 2, np.array([0.1, 0.1]))))
    with pytest.raises(NotImplementedError, match="dense"):
        ra.solve_mv_at(None, ra.ode.linear_dense(2, 2), dense["W"], dense["x0"], 0.0, T_MAX, N, interrogate_kramer,
                       dense["prior"], t, dense["prior_at"], A=A)


def test_refused_prior_at(no_device):
    t = np.array([1.0, 0.33])
    c = _case()
    for bad in (lambda h: ra.ibm_init(h, 4, np.full(2, 0.1)),                       # another n_deriv
                lambda h: ra.ibm_init(h, 3, np.full(3, 0.1)),                       # another n_block
                lambda h: ra.ibm_init(h, 3, np.full((5, 2), 0.1)),                  # a batch the call does not have
                lambda h: ra.ibm_init(h, 3, np.full(2, 0.1))[0]):                   # not a pair
        with pytest.raises(ValueError, match="prior_at"):
            _call(dict(c, prior_at=bad), t)
    # another sigma: a silently wrong posterior otherwise
    with pytest.raises(ValueError, match="inconsistent"):
        _call(dict(c, prior_at=lambda h: ra.ibm_init(h, 3, np.full(2, 0.101))), t)
    with pytest.raises(ValueError, match="inconsistent"):
        _call(dict(c, prior_at=lambda h: ra.ibm_init(2 * h, 3, np.full(2, 0.1))), t)
    # p = 2 is checked before it is padded onto the three-state tiles
    with pytest.raises(ValueError, match="inconsistent"):
        _call(dict(_case(p=2), prior_at=lambda h: ra.ibm_init(h, 2, np.full(2, 0.101))), t)


def test_consistency_check_accepts_ibm_init_to_rounding():
    for p in (2, 3, 4, 5):
        for sig in (np.array([0.1, 3.0]), np.array([[0.1, 3.0], [0.5, 0.02], [1.0, 1.0]])):
            prior = ra.ibm_init(DT, p, sig)
            for frac in (1e-3, 0.25, 0.5, 1 - 1e-3):
                h1 = frac * DT
                res = solve.check_prior_at(ra.ibm_init(h1, p, sig), ra.ibm_init(DT - h1, p, sig), prior, h1, DT - h1)
                assert max(res) <= 2e-15, (p, frac, res)


def test_prior_at_is_not_called_when_every_time_is_a_node(monkeypatch):
    """... and the device is reached only after every check has passed."""
    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached
    monkeypatch.setattr(solve, "default_device", reached)
    c = dict(_case(), prior_at=lambda h: pytest.fail("prior_at was called"))
    with pytest.raises(Reached):
        _call(c, np.array([0.0, T_MAX, 3 * DT, 3 * DT]))
    calls = []
    base = _case()

    def spy(h):
        calls.append(h)
        return base["prior_at"](h)
    with pytest.raises(Reached):
        _call(dict(base, prior_at=spy), np.array([0.33, 1.0, 0.33, 2.71, 0.33]))
    assert len(calls) == 4                                     # h1 and h2 of the two distinct off-grid times


def _cfg(p=3, kalman=_lib.KALMAN_STANDARD):
    return _lib.SolveCfg(n_traj=8, n_steps=N, n_block=2, n_bstate=p, n_bmeas=1, rhs_id=_lib.RHS_FITZHUGH_NAGUMO,
                         interrogate=_lib.INTERROGATE_KRAMER, kalman_type=kalman, n_theta=3, flags=0, t_min=0.0, t_max=T_MAX,
                         seed=0, traj_offset=0)


def test_library_repeats_the_refusals():
    lib = _lib.load()
    q = _lib.EvalAtIn(n_query=1, n_quad=1)
    out = _lib.SolveOut()

    def rc(cfg, layout):
        return lib.rk_eval_at(None, C.byref(cfg), layout, C.byref(out), C.byref(out), C.byref(q), None, None)
    for cfg, layout in ((_cfg(kalman=_lib.KALMAN_SQRT), _lib.LAYOUT_BATCH_MINOR), (_cfg(p=7), _lib.LAYOUT_TILEP),
                        (_cfg(p=6), _lib.LAYOUT_BATCH_MINOR), (_cfg(p=2), _lib.LAYOUT_BATCH_MINOR),
                        (_cfg(p=4), _lib.LAYOUT_TRAJ_MAJOR)):
        assert rc(cfg, layout) == _lib.RK_ERR_UNSUPPORTED
        assert b"eval_at" in lib.rk_last_error()
    # a layout that does not hold records of this n_bstate, and null arrays
    assert rc(_cfg(p=4), _lib.LAYOUT_TILE3) == _lib.RK_ERR_INVALID and b"eval_at" in lib.rk_last_error()
    assert rc(_cfg(p=3), _lib.LAYOUT_TILE3) == _lib.RK_ERR_INVALID and b"eval_at" in lib.rk_last_error()
    assert lib.rk_eval_at(None, None, 0, None, None, None, None, None) == _lib.RK_ERR_INVALID
    assert C.sizeof(_lib.EvalAtIn) == 48
