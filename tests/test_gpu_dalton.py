"""
DALTON on the device (rodeo_amd.inference.dalton, src/rodeo/inference/dalton.py:39-545) against the NumPy restatement
tests/dalton_oracle.py (the reference's literal joint form), on the lane-per-trajectory kernels (dalton_kernels.hpp).
"""
import ctypes as C
import os
import sys
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd.interrogate import interrogate_kramer, interrogate_rodeo, interrogate_schober
from oracle import odes, priors, interrogations as oi
import dalton_oracle as dal

pytestmark = pytest.mark.gpu

ITG = {"kramer": (interrogate_kramer, oi.interrogate_kramer), "rodeo": (interrogate_rodeo, oi.interrogate_rodeo),
       "schober": (interrogate_schober, oi.interrogate_schober)}
THETA = np.array([0.2, 0.2, 3.0])


def _module():
    import rodeo_amd.inference.dalton  # noqa: F401
    return sys.modules["rodeo_amd.inference.dalton"]


def _obs(N, t_max, d, p, n_bobs, times, seed=0):
    """Observations at `times` (one per grid index, first kept), D picks the first n_bobs state components."""
    ind = np.searchsorted(np.linspace(0.0, t_max, N + 1), times)
    _, keep = np.unique(ind, return_index=True)
    times = np.asarray(times)[np.sort(keep)]
    n = len(times)
    rng = np.random.default_rng(seed)
    D = np.zeros((n, d, n_bobs, p))
    for j in range(n_bobs):
        D[:, :, j, j] = 1.0
    D[:, :, 0, -1] = 0.05                                   # a dense row: the observation reads more than one component
    L = rng.standard_normal((n, d, n_bobs, n_bobs)) * 0.1
    Om = 0.05 * np.eye(n_bobs) + L @ np.swapaxes(L, -1, -2)
    y = rng.standard_normal((n, d, n_bobs)) * 0.5
    return y, times, D, Om


def _fhn(p, N=40, t_max=4.0, B=None, n_bobs=1, times=None, sigma=0.1):
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    thetas = THETA if B is None else THETA * (1 + 0.05 * np.arange(B))[:, None]
    x0 = init(np.array([-1.0, 1.0]), 0.0, theta=THETA)
    prior = priors.ibm_init(t_max / N, p, np.array([sigma, sigma]))
    if times is None:
        times = np.concatenate([[0.0], np.linspace(0.37, t_max - 0.21, 9), [t_max]])   # t = 0, off-grid, t_max
        times = np.sort(times[(times >= 0.0) & (times <= t_max)])
    y, times, D, Om = _obs(N, t_max, 2, p, n_bobs, times)
    return dict(W=W, x0=x0, N=N, t_max=t_max, prior=prior, thetas=thetas, obs=(y, times, D, Om))


def _device(fn, c, itg, ode_fun=ra.ode.fitzhugh_nagumo, key=None):
    y, times, D, Om = c["obs"]
    return fn(key, ode_fun, c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[itg][0], c["prior"], y, times, D, Om,
              theta=c["thetas"])


def _oracle(fn, c, itg, theta, ode=odes.fitzhugh_nagumo, **kw):
    y, times, D, Om = c["obs"]
    return fn(ode, c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[itg][1], c["prior"], y, times, D, Om, theta=theta, **kw)


def _check_ll(val, ref, rtol=1e-7):
    assert abs(val - ref) <= rtol * max(1.0, abs(ref)), (val, ref)


@pytest.mark.parametrize("itg", ["kramer", "rodeo", "schober"])
def test_dalton_fhn_p3_single_and_batched(itg):
    c = _fhn(3, N=80, t_max=2.0)                          # (dt = 0.025: schober's filter stays finite for every theta)
    val = _device(_module().dalton, c, itg)
    assert isinstance(val, float)
    _check_ll(val, _oracle(dal.dalton, c, itg, THETA))
    cb = _fhn(3, B=7, N=80, t_max=2.0)
    vals = _device(_module().dalton, cb, itg)
    assert vals.shape == (7,)
    for b in range(7):
        _check_ll(vals[b], _oracle(dal.dalton, cb, itg, cb["thetas"][b]))


@pytest.mark.parametrize("N", [1, 2, 16, 17, 33])
def test_dalton_horizons(N):
    c = _fhn(3, N=N, t_max=0.1 * N)
    _check_ll(_device(_module().dalton, c, "kramer"), _oracle(dal.dalton, c, "kramer", THETA))


def test_dalton_lorenz_three_blocks():
    N, t_max, p = 60, 1.2, 3
    W, init = ra.utils.first_order_pad(ra.ode.lorenz63, 3, p)
    theta = np.array([28.0, 10.0, 8.0 / 3.0])
    x0 = init(np.array([-12.0, -5.0, 38.0]), 0.0, theta=theta)
    prior = priors.ibm_init(t_max / N, p, np.array([5.0] * 3))
    y, times, D, Om = _obs(N, t_max, 3, p, 1, np.linspace(0.0, t_max, 7))
    y = y + x0[None, :, :1]
    val = _module().dalton(None, ra.ode.lorenz63, W, x0, 0.0, t_max, N, interrogate_kramer, prior, y, times, D, Om, theta=theta)
    ref = dal.dalton(odes.lorenz63, W, x0, 0.0, t_max, N, oi.interrogate_kramer, prior, y, times, D, Om, theta=theta)
    _check_ll(val, ref)


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


@pytest.mark.parametrize("p", [3, 4])
def test_dalton_traced_python_rhs(p):
    c = _fhn(p, **LANE[p])
    c["W"], _ = ra.utils.first_order_pad(_fitz, 2, p)
    _check_ll(_device(_module().dalton, c, "kramer", ode_fun=_fitz), _oracle(dal.dalton, c, "kramer", THETA))


def test_dalton_traced_rhs_keys_stay_apart_in_one_process():
    """One traced right-hand side at every (p, n_bobs) of the list, then the list in reverse: the run-time builds are keyed
    by n_bstate AND n_bobs, so no shape may be served by another shape's kernel; the second pass runs on cache hits."""
    shapes = [(3, 1), (3, 2), (3, 3), (4, 1), (4, 2)]
    cases = {}
    for p, n_bobs in shapes:
        c = _fhn(p, n_bobs=n_bobs, **LANE[p])
        c["W"], _ = ra.utils.first_order_pad(_fitz, 2, p)
        cases[p, n_bobs] = (c, _oracle(dal.dalton, c, "kramer", THETA))
    for shape in shapes + shapes[::-1]:
        c, ref = cases[shape]
        _check_ll(_device(_module().dalton, c, "kramer", ode_fun=_fitz), ref)


@pytest.mark.parametrize("p,n_bobs,lanes", [(3, 1, "0"), (3, 1, "1"), (4, 2, "0")])
def test_dalton_traced_rhs_solve_mv(p, n_bobs, lanes, monkeypatch):
    """test_dalton_solve_mv_parity around a traced right-hand side: the run-time builds of the tile and lane store kernels."""
    monkeypatch.setenv("RK_DALTON_LANES", lanes)
    c = _fhn(p, B=3, n_bobs=n_bobs, **LANE[p])
    c["W"], _ = ra.utils.first_order_pad(_fitz, 2, p)
    m, v = _device(_module().solve_mv, c, "kramer", ode_fun=_fitz)
    assert m.shape == (3, c["N"] + 1, 2, p) and v.shape == (3, c["N"] + 1, 2, p, p)
    for b in range(3):
        mo, vo = _oracle(dal.solve_mv, c, "kramer", c["thetas"][b])
        assert np.max(np.abs(m[b] - mo)) <= 1e-8 * max(1.0, np.max(np.abs(mo)))
        assert np.max(np.abs(v[b] - vo)) <= 1e-8 * max(1.0, np.max(np.abs(vo)))


# (grids and prior scales that keep every forecast variance far above utils.py:60-78's 1e-8 threshold)
LANE = {2: {}, 3: {}, 4: dict(N=20, sigma=10.0), 5: dict(N=20, sigma=10.0), 6: dict(N=10, t_max=2.0, sigma=1000.0)}


@pytest.mark.parametrize("p,n_bobs", [(3, 2), (3, 3), (2, 1), (4, 1), (5, 2), (6, 3)])
def test_dalton_lane_shapes(p, n_bobs):
    c = _fhn(p, n_bobs=n_bobs, **LANE[p])
    _check_ll(_device(_module().dalton, c, "rodeo"), _oracle(dal.dalton, c, "rodeo", THETA))


def test_dalton_linear_model_is_exact_on_the_device():
    from scipy.stats import multivariate_normal
    from test_oracle_fenrir import _exact_loglik
    N, t_max, p = 10, 1.0, 3
    W = np.array([[[0.0, 0.0, 1.0]]]); x0 = np.array([[-1.0, 0.0, 1.0]])
    Q, R = priors.ibm_init(t_max / N, p, np.array([0.5]))
    times = np.array([0.0, 0.2, 0.5, 1.0])
    y = np.random.default_rng(0).standard_normal((4, 1, 1)) * 0.3 - 0.5
    Dv = np.array([1.0, 0.0, 0.0])
    ow, ov = np.tile(Dv[None, None, None, :], (4, 1, 1, 1)), np.full((4, 1, 1, 1), 0.05)
    val = _module().dalton(None, ra.ode.higher_order, W, x0, 0.0, t_max, N, interrogate_kramer, (Q, R), y, times, ow, ov)
    ind = np.searchsorted(np.linspace(0.0, t_max, N + 1), times)
    ref = multivariate_normal.logpdf(y[0, 0, 0], Dv @ x0[0], 0.05) + _exact_loglik(
        W[0, 0], x0[0], Q[0], R[0], N, 0.0, t_max, {"a": np.array([-1.0, 0.0, 0.0]), "f": lambda t: np.sin(2 * t)},
        ind[1:], Dv, 0.05, y[1:, 0, 0])
    _check_ll(val, ref, 1e-8)


@pytest.mark.parametrize("p,n_bobs,lanes", [(3, 1, "0"), (3, 1, "1"), (4, 2, "0")])
def test_dalton_solve_mv_parity(p, n_bobs, lanes, monkeypatch):
    """solve_mv on the tile route (p = 3, one observation per block), on the lanes forced there, and at p = 4."""
    monkeypatch.setenv("RK_DALTON_LANES", lanes)
    c = _fhn(p, B=3, n_bobs=n_bobs, **LANE[p])
    m, v = _device(_module().solve_mv, c, "kramer")
    assert m.shape == (3, c["N"] + 1, 2, p) and v.shape == (3, c["N"] + 1, 2, p, p)
    for b in range(3):
        mo, vo = _oracle(dal.solve_mv, c, "kramer", c["thetas"][b])
        assert np.max(np.abs(m[b] - mo)) <= 1e-8 * max(1.0, np.max(np.abs(mo)))
        assert np.max(np.abs(v[b] - vo)) <= 1e-8 * max(1.0, np.max(np.abs(vo)))


@pytest.mark.parametrize("lanes", ["0", "1"])
def test_dalton_solve_sim_parity(lanes, monkeypatch):
    monkeypatch.setenv("RK_DALTON_LANES", lanes)
    c = _fhn(3, B=3)
    x = _device(_module().solve_sim, c, "kramer", key=5)
    assert x.shape == (3, c["N"] + 1, 2, 3)
    for b in range(3):
        xo = _oracle(dal.solve_sim, c, "kramer", c["thetas"][b], seed=5, traj=b)
        assert np.all(x[b, 0] == c["x0"])
        assert np.max(np.abs(x[b] - xo)) <= 1e-7 * max(1.0, np.max(np.abs(xo)))
    x2 = _device(_module().solve_sim, c, "kramer", key=6)
    assert np.max(np.abs(x2[:, 1:] - x[:, 1:])) > 1e-6


def test_dalton_leaves_the_plan_without_output_buffers():
    from rodeo_amd.solve import _plan_cache
    c = _fhn(3, N=23, t_max=2.3)
    _device(_module().dalton, c, "kramer")
    plans = [pl for pl in _plan_cache.values() if pl.N == 23]
    assert plans and all(pl._bufs == {} and pl.mean_state is None and pl.var_state is None for pl in plans)


def test_basic_then_dalton_solve_mv_makes_an_unread_xt_stale():
    from rodeo_amd.inference.basic import GaussianObsLoglik
    c = _fhn(3)                                           # (tile route: the plan without flags that basic() uses)
    y, times, D, Om = c["obs"]
    _, Xt = ra.inference.basic(None, ra.ode.fitzhugh_nagumo, c["W"], c["x0"], 0.0, c["t_max"], c["N"], interrogate_kramer,
                               c["prior"], np.zeros((len(times), 2)), times, GaussianObsLoglik(0.1), theta=THETA)
    _device(_module().solve_mv, c, "kramer")
    with pytest.raises(RuntimeError, match="earlier call"):
        np.asarray(Xt)


def _both_routes(fn, monkeypatch):
    monkeypatch.setenv("RK_DALTON_LANES", "0")
    tile = fn()
    monkeypatch.setenv("RK_DALTON_LANES", "1")
    lane = fn()
    return np.asarray(tile), np.asarray(lane)


@pytest.mark.parametrize("itg", ["kramer", "rodeo", "schober"])
def test_dalton_tile_and_lane_routes_agree(itg, monkeypatch):
    """The MFMA-tile route and the lane route on the same configurations (RK_DALTON_LANES=1), to 1e-9 relative."""
    from rodeo_amd import _lib
    c = _fhn(3, B=7, N=80, t_max=2.0)
    cfg_lay = []

    def run():
        v = _device(_module().dalton, c, itg)
        plan = [pl for pl in __import__("rodeo_amd.solve", fromlist=["_plan_cache"])._plan_cache.values() if pl.N == 80][-1]
        lay = C.c_int32(0)
        _lib.check(plan.dev.lib.rk_dalton_layout(C.byref(plan.cfg), _lib.MODE_FILTER, 1, C.byref(lay)))
        cfg_lay.append(lay.value)
        return v
    tile, lane = _both_routes(run, monkeypatch)
    assert cfg_lay == [_lib.LAYOUT_TILE3, _lib.LAYOUT_BATCH_MINOR]
    assert np.all(np.abs(tile - lane) <= 1e-9 * np.maximum(1.0, np.abs(lane))), (tile, lane)
    # one block (the linear ODE) and three blocks (Lorenz63) as well
    N, t_max = 60, 1.2
    W, init = ra.utils.first_order_pad(ra.ode.lorenz63, 3, 3)
    theta = np.array([28.0, 10.0, 8.0 / 3.0])
    x0 = init(np.array([-12.0, -5.0, 38.0]), 0.0, theta=theta)
    prior = priors.ibm_init(t_max / N, 3, np.array([5.0] * 3))
    y, times, D, Om = _obs(N, t_max, 3, 3, 1, np.linspace(0.0, t_max, 7))
    y = y + x0[None, :, :1]
    tile, lane = _both_routes(lambda: _module().dalton(None, ra.ode.lorenz63, W, x0, 0.0, t_max, N, ITG[itg][0], prior, y, times,
                                                       D, Om, theta=theta), monkeypatch)
    assert abs(tile - lane) <= 1e-9 * max(1.0, abs(lane)), (tile, lane)
    Wh = np.array([[[0.0, 0.0, 1.0]]]); xh = np.array([[-1.0, 0.0, 1.0]])
    ph = priors.ibm_init(0.1, 3, np.array([0.5]))
    yh, th_, Dh, Omh = _obs(10, 1.0, 1, 3, 1, np.array([0.0, 0.2, 0.55, 1.0]))
    tile, lane = _both_routes(lambda: _module().dalton(None, ra.ode.higher_order, Wh, xh, 0.0, 1.0, 10, ITG[itg][0], ph, yh, th_,
                                                       Dh, Omh), monkeypatch)
    assert abs(tile - lane) <= 1e-9 * max(1.0, abs(lane)), (tile, lane)


def test_lorenz_example_dalton_recovers_the_solution_beyond_7_5():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "lorenz_dalton.py")
    spec = importlib.util.spec_from_file_location("lorenz_dalton", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    err = mod.main()
    assert np.isfinite(err["dalton"]) and err["dalton"] < err["fenrir"], err
