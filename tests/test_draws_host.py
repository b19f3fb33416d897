"""
``solve_sim_draws`` on the host (no GPU): the signature and re-export, the refusals that come before any device work
(``default_device`` patched to fail), the rules for ``keep`` and ``n_draws``, the seed law's wrap at 2**64, and the library's
refusals on the configuration alone (no handle, no pointers), a traced right-hand side among them.
"""
import ctypes as C
import functools
import inspect
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd import _lib, draws
from rodeo_amd.interrogate import interrogate_kramer, interrogate_chkrebtii

DRAWS_ARGS = ["key", "ode_fun", "ode_weight", "ode_init", "t_min", "t_max", "n_steps", "interrogate", "prior_pars",
              "kalman_type", "n_draws", "keep", "params"]


def test_signature_and_re_export():
    assert ra.solve_sim_draws is draws.solve_sim_draws
    sig = inspect.signature(ra.solve_sim_draws)
    assert list(sig.parameters) == DRAWS_ARGS
    assert list(sig.parameters)[:9] == list(inspect.signature(ra.solve_sim).parameters)[:9]
    assert sig.parameters["kalman_type"].default == "standard"
    assert sig.parameters["n_draws"].default == 1 and sig.parameters["keep"].default is None
    assert sig.parameters["params"].kind is inspect.Parameter.VAR_KEYWORD
    doc = ra.solve_sim_draws.__doc__
    assert "n_draws" in doc and "keep" in doc and "ODE parameter" in doc          # the reserved keywords
    assert "2**64" in doc


def _fhn(p=3, N=40, t_max=4.0, ode=ra.ode.fitzhugh_nagumo):
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    theta = np.array([0.2, 0.2, 3.0])
    x0 = init(np.array([-1.0, 1.0]), 0.0, theta=theta)
    prior = ra.ibm_init(t_max / N, p, np.array([0.5, 0.3]))
    return dict(key=3, ode_fun=ode, ode_weight=W, ode_init=x0, t_min=0.0, t_max=t_max, n_steps=N,
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
        ra.solve_sim_draws(**_fhn(), kalman_type="nope")


def test_the_square_root_form_is_not_built(no_device):
    with pytest.raises(NotImplementedError, match="not built"):
        ra.solve_sim_draws(**_fhn(), kalman_type="square-root")


def test_chkrebtii_is_refused_with_the_reason(no_device):
    a = _fhn()
    a["interrogate"] = functools.partial(interrogate_chkrebtii, kalman_type="standard")
    with pytest.raises(NotImplementedError, match="interrogate_chkrebtii.*depends on the key.*cannot share one filter"):
        ra.solve_sim_draws(**a, n_draws=4)


def test_several_measurements_per_block_are_refused(no_device):
    a = _fhn()
    a["ode_weight"] = np.concatenate([a["ode_weight"]] * 2, axis=1)         # n_bmeas = 2 (the dense / indep_init form)
    with pytest.raises(NotImplementedError, match="n_bmeas"):
        ra.solve_sim_draws(**a)


@pytest.mark.parametrize("p", [1, 7, 9])
def test_n_bstate_outside_two_to_six_is_refused(no_device, p):
    W = np.zeros((2, 1, p)); W[:, 0, min(1, p - 1)] = 1.0
    a = _fhn()
    a.update(ode_weight=W, ode_init=np.zeros((2, p)), prior_pars=(np.tile(np.eye(p), (2, 1, 1)),) * 2)
    with pytest.raises(NotImplementedError, match="n_bstate"):
        ra.solve_sim_draws(**a)


@pytest.mark.parametrize("bad", [0, -3, 2.0, "4", None, True, 65536, np.array([2, 3])])
def test_n_draws_must_be_an_integer_from_one(no_device, bad):
    with pytest.raises(ValueError, match="n_draws"):
        ra.solve_sim_draws(**_fhn(), n_draws=bad)


@pytest.mark.parametrize("bad,word", [
    ([[0, 1]], "1-D"),                          # rank
    (3, "1-D"),                                 # a scalar
    ([0.0, 1.0], "integer"),                    # floats
    ([True, False], "integer"),                 # booleans
    ([], "1-D|empty|integer"),                  # empty (a float array by default)
    (np.zeros(0, dtype=np.int64), "empty"),
    ([-1, 3], "0 .. n_steps"),                  # below the grid
    ([0, 41], "0 .. n_steps"),                  # N = 40: node 41 does not exist
    ([3, 3], "strictly increasing"),
    ([5, 2], "strictly increasing"),
])
def test_keep_must_be_strictly_increasing_grid_indices(no_device, bad, word):
    with pytest.raises(ValueError, match=f"keep.*({word})"):
        ra.solve_sim_draws(**_fhn(), keep=bad)


def test_keep_rule_returns_the_indices_as_int32():
    assert draws._keep_rule(None, 40) is None
    for given in ([0], [40], [0, 40], np.arange(41), np.array([1, 7, 9], dtype=np.uint8), (2, 3)):
        k = draws._keep_rule(given, 40)
        assert k.dtype == np.int32 and k.ndim == 1
        np.testing.assert_array_equal(k, np.asarray(given))


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
        ra.solve_sim_draws(**a, n_draws=2, keep=[0, 5])


def test_a_right_hand_side_with_another_block_count_is_refused(no_device):
    with pytest.raises(ValueError, match="n_block"):
        ra.solve_sim_draws(**_fhn(ode=ra.ode.lorenz63))                    # three blocks against a d = 2 weight


def test_an_arbitrary_interrogate_is_a_type_error(no_device):
    a = _fhn()
    a["interrogate"] = lambda **k: None
    with pytest.raises(TypeError):
        ra.solve_sim_draws(**a)


def test_the_seed_wraps_at_two_to_the_sixty_four():
    top = 2 ** 64 - 1
    assert draws.draw_seed(None, 0) == 0 and draws.draw_seed(None, 5) == 5
    assert draws.draw_seed(7, 3) == 10
    assert draws.draw_seed(top, 0) == top and draws.draw_seed(top, 1) == 0 and draws.draw_seed(top - 1, 4) == 2
    assert draws.draw_seed(np.array([1, 2], dtype=np.uint32), 1) == (1 << 32) + 3       # a packed two-word key
    assert draws.draw_seed(np.array([0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32), 2) == 1
    assert C.c_uint64(draws.draw_seed(top, 1)).value == C.c_uint64(top + 1).value         # the device's own 64-bit sum


def test_the_oracle_helper_follows_the_same_law():
    """tests/draws_oracle.py at the wrap: draw 1 under seed 2**64 - 1 is solve_sim's path under seed 0."""
    import draws_oracle
    from oracle import scan, odes, interrogations as oi
    a = _fhn(N=4, t_max=0.1)
    args = (odes.fitzhugh_nagumo, a["ode_weight"], a["ode_init"], 0.0, 0.1, 4, oi.interrogate_kramer, a["prior_pars"])
    x = draws_oracle.solve_sim_draws(2 ** 64 - 1, *args, n_draws=2, keep=[0, 2, 4], theta=a["theta"])
    assert x.shape == (2, 3, 2, 3)
    np.testing.assert_array_equal(x[1], scan.solve_sim(0, *args, theta=a["theta"])[[0, 2, 4]])
    np.testing.assert_array_equal(x[0], scan.solve_sim(2 ** 64 - 1, *args, theta=a["theta"])[[0, 2, 4]])
    np.testing.assert_array_equal(x[:, 0], np.broadcast_to(a["ode_init"], (2, 2, 3)))      # node 0 is ode_init


# ---- the library, on the configuration alone ---------------------------------------------------------------------------
def _cfg(rhs=_lib.RHS_FITZHUGH_NAGUMO, d=2, p=3, m=1, itg=_lib.INTERROGATE_KRAMER, kalman=_lib.KALMAN_STANDARD, n_steps=50,
         flags=_lib.FLAG_BATCH_MINOR):
    return _lib.SolveCfg(n_traj=16, n_steps=n_steps, n_block=d, n_bstate=p, n_bmeas=m, rhs_id=rhs, interrogate=itg,
                         kalman_type=kalman, n_theta=3, flags=flags, t_min=0.0, t_max=1.0, seed=0, traj_offset=0)


def _call(cfg, n_draws=4, n_keep=0, keep=None):
    """rk_solve_sim_draws with no handle and no pointers: only the configuration, n_draws and n_keep can be looked at."""
    lib = _lib.load()
    rc = lib.rk_solve_sim_draws(None, C.byref(cfg), None, None, n_draws, keep, n_keep, None)
    return rc, lib.rk_last_error().decode()


@pytest.mark.parametrize("cfg,word", [
    (_cfg(kalman=7), "kalman_type"),
    (_cfg(kalman=_lib.KALMAN_SQRT), "not built"),
    (_cfg(itg=_lib.INTERROGATE_CHKREBTII), "chkrebtii"),
    (_cfg(itg=_lib.INTERROGATE_CHKREBTII), "cannot share one filter"),
    (_cfg(itg=9), "interrogate"),
    (_cfg(m=2), "n_bmeas"),
    (_cfg(p=1), "n_bstate"),
    (_cfg(p=7), "n_bstate"),
    (_cfg(rhs=_lib.RHS_LORENZ63, d=2), "n_block"),
    (_cfg(rhs=77), "rhs_id"),
])
def test_library_refuses_what_is_not_served(cfg, word):
    rc, msg = _call(cfg)
    assert rc == _lib.RK_ERR_UNSUPPORTED, (rc, msg)
    assert "sim_draws" in msg and word in msg, msg


@pytest.mark.parametrize("cfg", [_cfg(n_steps=0), _cfg(d=0), _cfg(p=0), _cfg(m=0)])
def test_library_calls_a_non_positive_size_invalid(cfg):
    rc, msg = _call(cfg)
    assert rc == _lib.RK_ERR_INVALID and "sim_draws" in msg, (rc, msg)


def test_library_needs_the_batch_minor_records():
    for flags in (0, _lib.FLAG_STORE_PRED):
        rc, msg = _call(_cfg(flags=flags))
        assert rc == _lib.RK_ERR_INVALID and "sim_draws" in msg and "RK_FLAG_BATCH_MINOR" in msg, (rc, msg)


@pytest.mark.parametrize("n_draws", [0, -1, 65536])
def test_library_calls_a_bad_n_draws_invalid(n_draws):
    rc, msg = _call(_cfg(), n_draws=n_draws)
    assert rc == _lib.RK_ERR_INVALID and "sim_draws" in msg and "n_draws" in msg, (rc, msg)


@pytest.mark.parametrize("n_keep", [0, -2, 52])
def test_library_calls_a_bad_n_keep_invalid(n_keep):
    """With a `keep` array n_keep must lie in 1 .. n_steps + 1 (the pointer itself is not read on the host)."""
    rc, msg = _call(_cfg(n_steps=50), n_keep=n_keep, keep=C.c_void_p(8))
    assert rc == _lib.RK_ERR_INVALID and "sim_draws" in msg and "n_keep" in msg, (rc, msg)


@pytest.mark.parametrize("cfg", [_cfg(), _cfg(p=2), _cfg(p=6), _cfg(itg=_lib.INTERROGATE_RODEO), _cfg(itg=_lib.INTERROGATE_SCHOBER),
                                 _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=3), _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=6),
                                 _cfg(rhs=_lib.RHS_HIGHER_ORDER, d=1, p=4)])
def test_library_passes_a_served_configuration_on_to_the_argument_check(cfg):
    """A served configuration gets as far as the null handle: RK_ERR_INVALID about the arguments, not about the cfg."""
    for n_keep, keep in ((0, None), (51, C.c_void_p(8)), (1, C.c_void_p(8))):
        rc, msg = _call(cfg, n_keep=n_keep, keep=keep)
        assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
    assert _lib.load().rk_solve_sim_draws(None, None, None, None, 1, None, 0, None) == _lib.RK_ERR_INVALID


def test_library_reports_its_chunk():
    assert draws.chunk() == _lib.load().rk_sim_draws_chunk() >= 1


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


@pytest.mark.parametrize("p,served", [(2, True), (6, True), (7, False)])
def test_library_serves_a_traced_right_hand_side_over_the_same_range(p, served):
    from rodeo_amd.trace import from_python
    ode = from_python(_fitz, 2, min(p, 6), theta=3)
    rc, msg = _call(_cfg(rhs=ode.rhs_id, p=p))
    if served:
        assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
    else:
        assert rc == _lib.RK_ERR_UNSUPPORTED and "sim_draws" in msg and "n_bstate" in msg, (rc, msg)
    rc, msg = _call(_cfg(rhs=ode.rhs_id, p=min(p, 4), d=3))                # another block count than the registration's
    assert rc == _lib.RK_ERR_UNSUPPORTED and "sim_draws" in msg and "n_block" in msg, (rc, msg)
