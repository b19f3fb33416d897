"""
Pins tests/fenrir_at_oracle.py (the NumPy restatement of ``fenrir_at``) and the host side of ``fenrir_at``; no GPU.

For a LINEAR ODE with the first-order (kramer) interrogation the solver's model is exactly linear Gaussian, so Fenrir's value
is the exact log p(y | z_{1:N} = 0) of one joint Gaussian: the prior's Markov chain over nodes and observation times together
(``oracle.joint_gaussian.gauss_markov_mv``), with z_n at the nodes and y at its own times -- the dense conditioning of
tests/test_oracle_dalton_at.py, whose models, observations and ``_exact_block`` are used here.  DALTON is exact on this model
too, so the two restatements must agree.
"""
import sys
import numpy as np
import pytest
from oracle import fenrir as ofen, interrogations as oi, odes, priors
import dalton_at_oracle as dat
import fenrir_at_oracle as fat
from test_oracle_dalton_at import DT, N, OM, SIGMA, T_MAX, T_MIN, _exact_block, _observations, _problem

# one at t_min; first interval; 1e-3 dt from a node; interior interval; two in one interval; an off-grid time in the interval
# below an observed node (6.6 dt under node 7); last interval; t_max (the second on-node time)
TIMES = np.array([0.0, 0.37 * DT, (3 + 1e-3) * DT, 4.5 * DT, 5.2 * DT, 5.9 * DT, 6.6 * DT, 7.0 * DT, 9.81 * DT, T_MAX])


def test_the_times_cover_the_placements():
    node, on = dat.classify(TIMES, T_MIN, T_MAX, N)
    assert list(node[on]) == [0, 7, N] and list(node[~on]) == [0, 3, 4, 5, 5, 6, 9]
    assert OM >= 1e-2


@pytest.mark.parametrize("p", [3, 4])
@pytest.mark.parametrize("d", [1, 2])
def test_at_oracle_equals_dense_conditioning_for_a_linear_ode(p, d):
    ode, W, x0, model = _problem(p, d)
    sigma = np.full(d, SIGMA)
    prior = priors.ibm_init(DT, p, sigma)
    y, D, Om = _observations(p, d, TIMES)
    seen = []
    val = fat.fenrir_at(ode, W, x0, T_MIN, T_MAX, N, oi.interrogate_kramer, prior, y, TIMES, D, Om,
                        lambda h: priors.ibm_init(h, p, sigma), forecast_vars=seen)
    # every forecast variance is D M D^T + Omega >= Omega = 0.05, so utils.py:60-78's 1e-8 rule never acts
    smallest = min(float(np.min(w)) for w in seen)
    print(f"p = {p}, d = {d}: smallest forecast variance {smallest:.3e}")
    assert len(seen) == len(TIMES) * d and smallest >= OM * (1 - 1e-9), smallest
    ref = sum(_exact_block(p, x0[b], model[b][0], model[b][1], TIMES, y[:, b, 0]) for b in range(d))
    print(f"p = {p}, d = {d}: at-oracle {val!r}, dense {ref!r}, |diff| = {abs(val - ref):.3e}")
    assert abs(val - ref) < 1e-8 * max(1.0, abs(ref)), (val, ref)
    # Fenrir and DALTON are both exact on this model
    dal = dat.dalton_at(ode, W, x0, T_MIN, T_MAX, N, oi.interrogate_kramer, prior, y, TIMES, D, Om,
                        lambda h: priors.ibm_init(h, p, sigma))
    print(f"p = {p}, d = {d}: dalton_at oracle {dal!r}, |diff| = {abs(val - dal):.3e}")
    assert abs(val - dal) < 1e-8 * max(1.0, abs(dal)), (val, dal)
    # and the times matter: the snapped value is another number
    keep = np.unique(np.searchsorted(np.linspace(T_MIN, T_MAX, N + 1), TIMES), return_index=True)[1]
    snapped = ofen.fenrir(None, ode, W, x0, T_MIN, T_MAX, N, oi.interrogate_kramer, prior, y[keep], TIMES[keep], D[keep], Om[keep])
    assert abs(snapped - val) > 1e-3


@pytest.mark.parametrize("itg", ["kramer", "rodeo", "schober"])
def test_with_all_times_on_nodes_the_at_oracle_is_the_fenrir_oracle(itg):
    fn = getattr(oi, "interrogate_" + itg)
    W, init = priors.first_order_pad(odes.fitzhugh_nagumo, 2, 3)
    theta = np.array([0.2, 0.2, 3.0])
    x0 = init(np.array([-1.0, 1.0]), 0.0, theta=theta)
    n, t_max = 20, 2.0
    prior = priors.ibm_init(t_max / n, 3, np.array([0.1, 0.1]))
    nodes = np.array([0, 3, 4, 11, 20])
    times = t_max * nodes / n
    times[2] += 0.5e-10 * t_max / n                             # within the tolerance of node 4: that node
    y, D, Om = _observations(3, 2, times)

    def never(h):
        raise AssertionError("prior_at is not needed when every time is a node")
    a = fat.fenrir_at(odes.fitzhugh_nagumo, W, x0, 0.0, t_max, n, fn, prior, y, times, D, Om, never, theta=theta)
    b = ofen.fenrir(None, odes.fitzhugh_nagumo, W, x0, 0.0, t_max, n, fn, prior, y, np.linspace(0.0, t_max, n + 1)[nodes], D, Om,
                    theta=theta)
    print(f"{itg}: at-oracle {a!r}, fenrir oracle {b!r}, relative difference {abs(a - b) / max(1.0, abs(b)):.3e}")
    assert abs(a - b) <= 1e-8 * max(1.0, abs(b)), (a, b)


# ---- the host side of fenrir_at: everything is refused before a device is asked for ----------------------------------------
def _module():
    import rodeo_amd.inference.fenrir  # noqa: F401
    return sys.modules["rodeo_amd.inference.fenrir"]


def _call(**over):
    import rodeo_amd as ra
    from rodeo_amd.interrogate import interrogate_kramer
    p, n, t_max = over.pop("p", 3), 10, 1.0
    sigma = np.array([0.1, 0.1])
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    theta = np.array([0.2, 0.2, 3.0])
    c = dict(W=W, x0=init(np.array([-1.0, 1.0]), 0.0, theta=theta), prior=ra.ibm_init(t_max / n, p, sigma),
             times=np.array([0.137, 0.5, 0.93]), prior_at=lambda h: ra.ibm_init(h, p, sigma), kalman_type="standard")
    c.update(over)
    y, D, Om = _observations(p, 2, c["times"])
    return _module().fenrir_at(None, ra.ode.fitzhugh_nagumo, c["W"], c["x0"], 0.0, t_max, n, interrogate_kramer, c["prior"], y,
                               c["times"], D, Om, c["prior_at"], kalman_type=c["kalman_type"], theta=theta)


def test_fenrir_at_refusals_are_raised_without_a_device(monkeypatch):
    import rodeo_amd as ra
    import rodeo_amd.solve as solve
    _module()
    assert not hasattr(ra.inference, "fenrir_at")           # imported from rodeo_amd.inference.fenrir, not re-exported
    monkeypatch.setattr(solve, "default_device", lambda *a, **k: pytest.fail("a device was asked for"))
    sigma = np.array([0.1, 0.1])
    with pytest.raises(ValueError, match="fenrir_at: obs_times must be strictly increasing"):
        _call(times=np.array([0.5, 0.137, 0.93]))
    with pytest.raises(ValueError, match="strictly increasing"):
        _call(times=np.array([0.137, 0.137, 0.93]))
    with pytest.raises(ValueError, match="t_max"):
        _call(times=np.array([0.137, 0.5, 1.0 + 1e-6]))
    with pytest.raises(ValueError, match="t_max"):
        _call(times=np.array([-1e-6, 0.5, 0.93]))
    with pytest.raises(ValueError, match="non-finite"):
        _call(times=np.array([0.137, np.nan, 0.93]))
    with pytest.raises(ValueError, match="non-finite"):
        _call(times=np.array([0.137, 0.5, np.inf]))
    with pytest.raises(ValueError, match="fenrir_at: two observation times are the same grid node"):
        _call(times=np.array([0.2, 0.2 + 0.5e-11, 0.93]))
    with pytest.raises(ValueError, match="inconsistent"):
        _call(prior_at=lambda h: ra.ibm_init(h, 3, 1.01 * sigma))
    with pytest.raises(ValueError, match="inconsistent"):    # the chain of an interval with two observations
        _call(times=np.array([0.52, 0.57, 0.93]), prior_at=lambda h: ra.ibm_init(h, 3, 1.01 * sigma))
    with pytest.raises(ValueError, match="shape"):
        _call(prior_at=lambda h: ra.ibm_init(h, 4, sigma))
    with pytest.raises(ValueError, match="shape"):
        _call(prior_at=lambda h: ra.ibm_init(h, 3, np.array([0.1])))
    with pytest.raises(ValueError, match="pair"):
        _call(prior_at=lambda h: 1.0)
    with pytest.raises(NotImplementedError, match="not built"):
        _call(kalman_type="square-root")
    with pytest.raises(NotImplementedError):
        _call(kalman_type="other")
    for p in (7, 8):
        with pytest.raises(NotImplementedError, match="n_bstate"):
            _call(p=p)


def test_the_shared_table_builder_keeps_dalton_at_s_texts():
    from rodeo_amd.inference import _obs as dmod
    with pytest.raises(ValueError, match="dalton_at: obs_times must be strictly increasing"):
        dmod._at_layout(np.array([0.5, 0.2]), 0.0, 1.0, 10, None, None, 2, 3, 1)
    with pytest.raises(ValueError, match="fenrir_at: obs_times must be strictly increasing"):
        dmod._at_layout(np.array([0.5, 0.2]), 0.0, 1.0, 10, None, None, 2, 3, 1, who="fenrir_at")


def test_library_refuses_on_the_configuration_alone_and_names_fenrir_at():
    """rk_fenrir_backward_at refuses on the configuration alone, before it looks at the handle or at any array: no handle and
    no pointer is passed here."""
    import ctypes as C
    from rodeo_amd import _lib
    lib = _lib.load()
    both = _lib.FLAG_STORE_PRED | _lib.FLAG_BATCH_MINOR
    cfg = _lib.SolveCfg(n_traj=1, n_steps=10, n_block=2, n_bstate=3, n_bmeas=1, rhs_id=_lib.RHS_FITZHUGH_NAGUMO,
                        interrogate=_lib.INTERROGATE_KRAMER, kalman_type=_lib.KALMAN_SQRT, n_theta=3, flags=0, t_min=0.0,
                        t_max=1.0, seed=0, traj_offset=0)

    def call(n_bobs=1):
        return lib.rk_fenrir_backward_at(None, C.byref(cfg), None, None, None, None, None, None, 1, n_bobs, None, None)
    assert call() == _lib.RK_ERR_UNSUPPORTED and b"fenrir_at" in lib.rk_last_error() and b"not built" in lib.rk_last_error()
    cfg.kalman_type = 7
    assert call() == _lib.RK_ERR_UNSUPPORTED and b"fenrir_at" in lib.rk_last_error()
    cfg.kalman_type = _lib.KALMAN_STANDARD
    assert call(n_bobs=4) == _lib.RK_ERR_UNSUPPORTED and b"fenrir_at" in lib.rk_last_error()
    for p in (7, 8):
        for flags in (0, both):
            cfg.n_bstate, cfg.flags = p, flags
            assert call() == _lib.RK_ERR_UNSUPPORTED and b"fenrir_at" in lib.rk_last_error() and b"n_bstate" in lib.rk_last_error()
    cfg.n_bstate, cfg.flags = 5, 0                                          # the blocked-tile records are not served
    assert call() == _lib.RK_ERR_UNSUPPORTED and b"fenrir_at" in lib.rk_last_error()
    cfg.n_bstate = 3                                                        # two observations per block need the lanes
    assert call(n_bobs=2) == _lib.RK_ERR_UNSUPPORTED and b"fenrir_at" in lib.rk_last_error()
    cfg.flags = _lib.FLAG_BATCH_MINOR                                       # one of the two flags only
    assert call() == _lib.RK_ERR_INVALID and b"fenrir_at" in lib.rk_last_error()
    for p, flags, n_bobs in ((3, 0, 1), (3, both, 2), (6, both, 3)):        # served, but no handle
        cfg.n_bstate, cfg.flags = p, flags
        assert call(n_bobs) == _lib.RK_ERR_INVALID and b"fenrir_at" in lib.rk_last_error()
        need = C.c_size_t(0)
        assert lib.rk_fenrir_at_workspace_bytes(C.byref(cfg), n_bobs, 5, C.byref(need)) == _lib.RK_OK
        assert need.value == 8 * 5 * 2 * (48 if flags == 0 else 3 * p * p + 2 * p)
    assert lib.rk_fenrir_backward_at(None, None, None, None, None, None, None, None, 1, 1, None, None) == _lib.RK_ERR_INVALID
