"""
``solve_evidence`` on the host (no GPU): the signature, the refusals that come before any device work (``default_device``
patched to fail), the library's refusals on the configuration alone (no handle, no pointers), and ``evidence_scale`` /
``evidence_at`` on hand-made numbers.
"""
import ctypes as C
import functools
import inspect
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd import _lib
from rodeo_amd.evidence import Evidence, evidence_at, evidence_scale
from rodeo_amd.interrogate import interrogate_kramer, interrogate_rodeo, interrogate_chkrebtii

SOLVE_MV_ARGS = ["key", "ode_fun", "ode_weight", "ode_init", "t_min", "t_max", "n_steps", "interrogate", "prior_pars",
                 "kalman_type", "params"]


def test_signature_is_solve_mv_s():
    assert ra.solve_evidence is ra.evidence.solve_evidence
    assert ra.evidence_scale is evidence_scale and ra.evidence_at is evidence_at and ra.Evidence is Evidence
    for fn in (ra.solve_evidence, ra.solve_mv):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == SOLVE_MV_ARGS
        assert sig.parameters["kalman_type"].default == "standard"
        assert sig.parameters["params"].kind is inspect.Parameter.VAR_KEYWORD
    assert Evidence._fields == ("logdens", "quad", "logdet", "n_steps")


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


def test_unknown_kalman_type_is_refused(no_device):
    with pytest.raises(NotImplementedError, match="kalman_type"):
        ra.solve_evidence(**_fhn(), kalman_type="nope")


@pytest.mark.parametrize("kalman_type", ["standard", "square-root"])
def test_chkrebtii_is_refused_with_the_reason(no_device, kalman_type):
    a = _fhn()
    a["interrogate"] = functools.partial(interrogate_chkrebtii, kalman_type=kalman_type)
    with pytest.raises(NotImplementedError, match="interrogate_chkrebtii.*predicted variance"):
        ra.solve_evidence(**a, kalman_type=kalman_type)


def test_several_measurements_per_block_are_refused(no_device):
    a = _fhn()
    a["ode_weight"] = np.concatenate([a["ode_weight"]] * 2, axis=1)         # n_bmeas = 2 (the dense / indep_init form)
    with pytest.raises(NotImplementedError, match="n_bmeas"):
        ra.solve_evidence(**a)


@pytest.mark.parametrize("kalman_type,p", [("standard", 1), ("standard", 7), ("standard", 8), ("square-root", 1),
                                           ("square-root", 9)])
def test_n_bstate_outside_the_served_range_is_refused(no_device, kalman_type, p):
    W = np.zeros((2, 1, p)); W[:, 0, min(1, p - 1)] = 1.0
    a = _fhn()
    a.update(ode_weight=W, ode_init=np.zeros((2, p)), prior_pars=(np.tile(np.eye(p), (2, 1, 1)),) * 2)
    with pytest.raises(NotImplementedError, match="n_bstate"):
        ra.solve_evidence(**a, kalman_type=kalman_type)


def test_three_blocks_stop_at_five_in_the_standard_form(no_device):
    W = np.zeros((3, 1, 6)); W[:, 0, 1] = 1.0
    args = dict(key=None, ode_fun=ra.ode.lorenz63, ode_weight=W, ode_init=np.zeros((3, 6)), t_min=0.0, t_max=1.0, n_steps=10,
                interrogate=interrogate_rodeo, prior_pars=(np.tile(np.eye(6), (3, 1, 1)),) * 2, theta=np.array([28.0, 10.0, 8 / 3]))
    with pytest.raises(NotImplementedError, match="three or more blocks"):
        ra.solve_evidence(**args)


@pytest.mark.parametrize("change", [
    dict(ode_weight=np.zeros((1, 3))),                                      # rank
    dict(ode_init=np.zeros((2, 4))),                                        # ode_init against ode_weight
    dict(prior_pars=(np.zeros((2, 3, 3)), np.zeros((2, 4, 4)))),            # prior against ode_weight
    dict(ode_init=np.zeros((5, 2, 3)), theta=np.ones((4, 3))),              # inconsistent batch sizes
])
def test_the_shape_rule_s_refusals(no_device, change):
    a = _fhn()
    a.update(change)
    with pytest.raises(ValueError):
        ra.solve_evidence(**a)


def test_a_right_hand_side_with_another_block_count_is_refused(no_device):
    a = _fhn(ode=ra.ode.lorenz63)                                          # three blocks against a d = 2 weight
    with pytest.raises(ValueError, match="n_block"):
        ra.solve_evidence(**a)


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


@pytest.mark.parametrize("p,kalman,rc_served", [(6, _lib.KALMAN_STANDARD, True), (7, _lib.KALMAN_STANDARD, False),
                                               (7, _lib.KALMAN_SQRT, True), (8, _lib.KALMAN_SQRT, True), (9, _lib.KALMAN_SQRT, False)])
def test_library_serves_a_traced_right_hand_side_over_the_whole_range(p, kalman, rc_served):
    """A Python ode_fun has the built-in ones' range: standard 2..6, square-root 2..8 (no handle: a served configuration gets
    as far as the argument check)."""
    from rodeo_amd.trace import from_python
    ode = from_python(_fitz, 2, p, theta=3)
    rc, msg = _call(_cfg(rhs=ode.rhs_id, p=p, kalman=kalman))
    if rc_served:
        assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
    else:
        assert rc == _lib.RK_ERR_UNSUPPORTED and "n_bstate" in msg, (rc, msg)
    rc, msg = _call(_cfg(rhs=ode.rhs_id, p=p, kalman=kalman, d=3))
    assert rc == _lib.RK_ERR_UNSUPPORTED, (rc, msg)


def test_an_arbitrary_interrogate_is_a_type_error(no_device):
    a = _fhn()
    a["interrogate"] = lambda **k: None
    with pytest.raises(TypeError):
        ra.solve_evidence(**a)


# ---- the library, on the configuration alone ---------------------------------------------------------------------------
def _cfg(rhs=_lib.RHS_FITZHUGH_NAGUMO, d=2, p=3, m=1, itg=_lib.INTERROGATE_KRAMER, kalman=_lib.KALMAN_STANDARD, n_steps=50):
    return _lib.SolveCfg(n_traj=16, n_steps=n_steps, n_block=d, n_bstate=p, n_bmeas=m, rhs_id=rhs, interrogate=itg,
                         kalman_type=kalman, n_theta=3, flags=0, t_min=0.0, t_max=1.0, seed=0, traj_offset=0)


def _call(cfg):
    """rk_solve_evidence with no handle and no pointers: only the configuration can be looked at."""
    lib = _lib.load()
    rc = lib.rk_solve_evidence(None, C.byref(cfg), None, None, None, None)
    return rc, lib.rk_last_error().decode()


@pytest.mark.parametrize("cfg,word", [
    (_cfg(kalman=7), "kalman_type"),
    (_cfg(itg=_lib.INTERROGATE_CHKREBTII), "chkrebtii"),
    (_cfg(itg=_lib.INTERROGATE_CHKREBTII, kalman=_lib.KALMAN_SQRT), "chkrebtii"),
    (_cfg(itg=9), "interrogate"),
    (_cfg(m=2), "n_bmeas"),
    (_cfg(p=1), "n_bstate"),
    (_cfg(p=7), "n_bstate"),
    (_cfg(p=9, kalman=_lib.KALMAN_SQRT), "n_bstate"),
    (_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=6), "n_bstate"),
    (_cfg(rhs=_lib.RHS_LORENZ63, d=2), "n_block"),
    (_cfg(rhs=77), "rhs_id"),
])
def test_library_refuses_what_is_not_served(cfg, word):
    rc, msg = _call(cfg)
    assert rc == _lib.RK_ERR_UNSUPPORTED, (rc, msg)
    assert "evidence" in msg and word in msg, msg


@pytest.mark.parametrize("cfg", [_cfg(n_steps=0), _cfg(d=0), _cfg(p=0), _cfg(m=0)])
def test_library_calls_a_non_positive_size_invalid(cfg):
    rc, msg = _call(cfg)
    assert rc == _lib.RK_ERR_INVALID, (rc, msg)
    assert "evidence" in msg


@pytest.mark.parametrize("cfg", [_cfg(), _cfg(p=2), _cfg(p=6), _cfg(p=8, kalman=_lib.KALMAN_SQRT), _cfg(itg=_lib.INTERROGATE_RODEO),
                                 _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=5), _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=8, kalman=_lib.KALMAN_SQRT),
                                 _cfg(rhs=_lib.RHS_HIGHER_ORDER, d=1, p=4)])
def test_library_passes_a_served_configuration_on_to_the_argument_check(cfg):
    """A served configuration gets as far as the null handle: RK_ERR_INVALID about the arguments, not about the cfg."""
    rc, msg = _call(cfg)
    assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
    assert _lib.load().rk_solve_evidence(None, None, None, None, None, None) == _lib.RK_ERR_INVALID


# ---- the host helpers --------------------------------------------------------------------------------------------------
def test_evidence_scale_and_evidence_at_on_hand_made_numbers():
    N = 10
    quad, logdet = np.array([40.0, 2.5]), np.array([-30.0, -12.0])
    ld = -0.5 * ((40.0 - 30.0) + (2.5 - 12.0)) - 2 * N * np.log(2 * np.pi) / 2
    ev = Evidence(ld, quad, logdet, N)
    c = evidence_scale(ev)
    np.testing.assert_array_equal(c, [4.0, 0.25])
    assert evidence_at(ev, np.ones(2)) == pytest.approx(ld, rel=1e-15)
    assert isinstance(evidence_at(ev, np.ones(2)), float)
    want = -0.5 * ((40.0 / 4.0 - 30.0 + N * np.log(4.0)) + (2.5 / 0.25 - 12.0 + N * np.log(0.25))) - N * np.log(2 * np.pi)
    assert evidence_at(ev, c) == pytest.approx(want, rel=1e-14)
    # the maximum over c is at quad / N
    for other in ([4.4, 0.25], [4.0, 0.2], [3.0, 0.3]):
        assert evidence_at(ev, np.array(other)) < evidence_at(ev, c)
    with pytest.raises(ValueError):
        evidence_at(ev, np.array([1.0, 0.0]))


def test_helpers_keep_a_batch_axis():
    N = 8
    quad = np.array([[8.0, 16.0], [4.0, 2.0], [1.0, 80.0]])
    logdet = np.array([[-3.0, 1.0], [0.5, -7.0], [2.0, 2.0]])
    ld = np.array([-0.5 * ((q[0] + l[0]) + (q[1] + l[1])) - 2 * N * np.log(2 * np.pi) / 2 for q, l in zip(quad, logdet)])
    ev = Evidence(ld, quad, logdet, N)
    c = evidence_scale(ev)
    assert c.shape == (3, 2)
    np.testing.assert_array_equal(c, quad / N)
    np.testing.assert_allclose(evidence_at(ev, np.ones(2)), ld, rtol=1e-15)
    at = evidence_at(ev, c)
    assert at.shape == (3,)
    for i in range(3):
        one = Evidence(ld[i], quad[i], logdet[i], N)
        assert at[i] == evidence_at(one, c[i])
        assert evidence_at(ev, c[i])[i] == at[i]                   # a shared c broadcasts over the batch
