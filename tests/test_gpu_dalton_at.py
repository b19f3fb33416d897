"""
``rodeo_amd.inference.dalton.dalton_at`` on the device (DALTON's log-likelihood with the observations at their own times)
against its NumPy restatement tests/dalton_at_oracle.py, on the MFMA-tile route (dalton_at_tile3_kernels.hpp) and the
lane-per-trajectory route (dalton_at_kernels.hpp).
"""
import sys
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd.interrogate import interrogate_kramer, interrogate_rodeo, interrogate_schober
from oracle import odes, priors, interrogations as oi
import dalton_at_oracle as dat

pytestmark = pytest.mark.gpu

ITG = {"kramer": (interrogate_kramer, oi.interrogate_kramer), "rodeo": (interrogate_rodeo, oi.interrogate_rodeo),
       "schober": (interrogate_schober, oi.interrogate_schober)}
THETA = np.array([0.2, 0.2, 3.0])
# N = 40, t_max = 4 (dt = 0.1): seven observations, two on nodes (4 and 17) and five between nodes
TIMES = np.array([0.4, 0.537, 1.062, 1.7, 2.251, 2.918, 3.649])
FINE = dict(N=80, t_max=2.0)      # dt = 0.025, where schober's filter stays finite for every theta (tests/test_gpu_dalton.py)
# (grids and prior scales of tests/test_gpu_dalton.py that keep every forecast variance far above utils.py:60-78's threshold)
LANE = {2: {}, 3: {}, 4: dict(N=20, sigma=10.0), 5: dict(N=20, sigma=10.0), 6: dict(N=10, t_max=2.0, sigma=1000.0)}


def _module():
    import rodeo_amd.inference.dalton  # noqa: F401
    return sys.modules["rodeo_amd.inference.dalton"]


def _obs(times, d, p, n_bobs, seed=0):
    """Observations at `times`; D picks the first n_bobs state components, with one dense row."""
    n = len(times)
    rng = np.random.default_rng(seed)
    D = np.zeros((n, d, n_bobs, p))
    for j in range(n_bobs):
        D[:, :, j, j] = 1.0
    D[:, :, 0, -1] = 0.05
    L = rng.standard_normal((n, d, n_bobs, n_bobs)) * 0.1
    Om = 0.05 * np.eye(n_bobs) + L @ np.swapaxes(L, -1, -2)
    return rng.standard_normal((n, d, n_bobs)) * 0.5, D, Om


def _fhn(p=3, N=40, t_max=4.0, B=None, n_bobs=1, times=None, sigma=0.1):
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    thetas = THETA if B is None else THETA * (1 + 0.01 * (np.arange(B) % 7))[:, None]
    x0 = init(np.array([-1.0, 1.0]), 0.0, theta=THETA)
    sig = np.array([sigma, sigma])
    times = TIMES * (t_max / 4.0) if times is None else np.asarray(times, dtype=np.float64)
    return dict(W=W, x0=x0, N=N, t_max=t_max, p=p, sigma=sig, prior=priors.ibm_init(t_max / N, p, sig), thetas=thetas,
                times=times, obs=_obs(times, 2, p, n_bobs))


def _device(c, itg, ode_fun=ra.ode.fitzhugh_nagumo, prior_at=None, fn=None):
    y, D, Om = c["obs"]
    if prior_at is None:
        def prior_at(h):
            return ra.ibm_init(h, c["p"], c["sigma"])
    if fn is None:
        return _module().dalton_at(None, ode_fun, c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[itg][0], c["prior"], y,
                                   c["times"], D, Om, prior_at, theta=c["thetas"])
    return fn(None, ode_fun, c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[itg][0], c["prior"], y, c["times"], D, Om,
              theta=c["thetas"])


def _oracle(c, itg, theta, ode=odes.fitzhugh_nagumo, sigma=None, prior=None):
    y, D, Om = c["obs"]
    sigma = c["sigma"] if sigma is None else sigma
    return dat.dalton_at(ode, c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[itg][1], c["prior"] if prior is None else prior, y,
                         c["times"], D, Om, lambda h: priors.ibm_init(h, c["p"], sigma), theta=theta)


def _check_ll(val, ref, rtol=1e-7):
    print(f"device {val!r}, oracle {ref!r}, relative difference {abs(val - ref) / max(1.0, abs(ref)):.3e}")
    assert abs(val - ref) <= rtol * max(1.0, abs(ref)), (val, ref)


@pytest.mark.parametrize("lanes", ["0", "1"])
@pytest.mark.parametrize("itg", ["kramer", "rodeo", "schober"])
def test_dalton_at_fhn_single_and_batched(itg, lanes, monkeypatch):
    monkeypatch.setenv("RK_DALTON_LANES", lanes)
    c = _fhn(**FINE)
    val = _device(c, itg)
    assert isinstance(val, float)
    _check_ll(val, _oracle(c, itg, THETA))
    cb = _fhn(B=3, **FINE)
    vals = _device(cb, itg)
    assert vals.shape == (3,)
    for b in range(3):
        _check_ll(vals[b], _oracle(cb, itg, cb["thetas"][b]))


@pytest.mark.parametrize("lanes", ["0", "1"])
@pytest.mark.parametrize("itg", ["kramer", "rodeo"])
def test_dalton_at_default_grid_single_and_batched(itg, lanes, monkeypatch):
    """N = 40, t_max = 4 (dt = 0.1), where kramer's and rodeo's filters are stable; schober's is not (see FINE)."""
    monkeypatch.setenv("RK_DALTON_LANES", lanes)
    c = _fhn()
    _check_ll(_device(c, itg), _oracle(c, itg, THETA))
    cb = _fhn(B=3)
    vals = _device(cb, itg)
    assert vals.shape == (3,)
    for b in range(3):
        _check_ll(vals[b], _oracle(cb, itg, cb["thetas"][b]))


@pytest.mark.parametrize("lanes", ["0", "1"])
def test_dalton_at_batch_spanning_waves(lanes, monkeypatch):
    """B = 70: more than one wave on the tiles (2 trajectories per wave) and on the lanes (32 per wave, a ragged last one)."""
    monkeypatch.setenv("RK_DALTON_LANES", lanes)
    c = _fhn(B=70)
    vals = _device(c, "kramer")
    assert vals.shape == (70,)
    ref = {b: _oracle(c, "kramer", c["thetas"][b]) for b in range(7)}       # (the parameters repeat with period 7)
    for b in range(70):
        _check_ll(vals[b], ref[b % 7])


@pytest.mark.parametrize("lanes", ["0", "1"])
def test_dalton_at_batched_sigma(lanes, monkeypatch):
    """A prior scale per trajectory: R batched, Q shared, in prior_pars and in what prior_at returns."""
    monkeypatch.setenv("RK_DALTON_LANES", lanes)
    c = _fhn(B=3)
    sig = np.array([[0.1, 0.1], [0.15, 0.08], [0.07, 0.2]])
    c["prior"] = ra.ibm_init(c["t_max"] / c["N"], 3, sig)
    assert c["prior"][0].ndim == 3 and c["prior"][1].ndim == 4
    vals = _device(c, "kramer", prior_at=lambda h: ra.ibm_init(h, 3, sig))
    for b in range(3):
        _check_ll(vals[b], _oracle(c, "kramer", c["thetas"][b], sigma=sig[b], prior=priors.ibm_init(c["t_max"] / c["N"], 3, sig[b])))


@pytest.mark.parametrize("lanes", ["0", "1"])
@pytest.mark.parametrize("N", [1, 2])
def test_dalton_at_short_horizons(N, lanes, monkeypatch):
    """An observation in the first interval and one in the last (the same interval at N = 1)."""
    monkeypatch.setenv("RK_DALTON_LANES", lanes)
    t_max = 0.1 * N
    c = _fhn(N=N, t_max=t_max, times=[0.031, t_max - 0.042])
    _check_ll(_device(c, "kramer"), _oracle(c, "kramer", THETA))


@pytest.mark.parametrize("lanes", ["0", "1"])
@pytest.mark.parametrize("times", [[0.537, 1.012, 1.051, 1.093, 2.9], [0.0, 0.05, 1.7, 3.97]],
                         ids=["several_in_one_interval", "t_min_plus_off_grid"])
def test_dalton_at_placements(times, lanes, monkeypatch):
    monkeypatch.setenv("RK_DALTON_LANES", lanes)
    c = _fhn(times=times)
    _check_ll(_device(c, "kramer"), _oracle(c, "kramer", THETA))


@pytest.mark.parametrize("lanes", ["0", "1"])
def test_dalton_at_lorenz_three_blocks(lanes, monkeypatch):
    monkeypatch.setenv("RK_DALTON_LANES", lanes)
    N, t_max, p = 60, 1.2, 3
    W, init = ra.utils.first_order_pad(ra.ode.lorenz63, 3, p)
    theta = np.array([28.0, 10.0, 8.0 / 3.0])
    x0 = init(np.array([-12.0, -5.0, 38.0]), 0.0, theta=theta)
    sig = np.array([5.0] * 3)
    times = np.array([0.0, 0.113, 0.4, 0.617, 0.625, 1.191])
    y, D, Om = _obs(times, 3, p, 1)
    y = y + x0[None, :, :1]
    prior = priors.ibm_init(t_max / N, p, sig)
    val = _module().dalton_at(None, ra.ode.lorenz63, W, x0, 0.0, t_max, N, interrogate_kramer, prior, y, times, D, Om,
                              lambda h: ra.ibm_init(h, p, sig), theta=theta)
    ref = dat.dalton_at(odes.lorenz63, W, x0, 0.0, t_max, N, oi.interrogate_kramer, prior, y, times, D, Om,
                        lambda h: priors.ibm_init(h, p, sig), theta=theta)
    _check_ll(val, ref)


# (kramer where its filter is stable on these grids: at p = 5, 6 with LANE's prior scales the restatement itself diverges, 2e12)
@pytest.mark.parametrize("p,n_bobs,itg", [(3, 2, "rodeo"), (2, 1, "rodeo"), (4, 1, "rodeo"), (5, 2, "rodeo"), (6, 3, "rodeo"),
                                          (3, 2, "kramer"), (2, 1, "kramer"), (4, 1, "kramer")])
def test_dalton_at_lane_shapes(p, n_bobs, itg):
    c = _fhn(p, n_bobs=n_bobs, **LANE[p])
    _check_ll(_device(c, itg), _oracle(c, itg, THETA))


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


@pytest.mark.parametrize("itg", ["kramer", "rodeo"])
@pytest.mark.parametrize("p", [3, 4])
def test_dalton_at_traced_python_rhs(p, itg):
    """A Python right-hand side: the hiprtc kinds JIT_DALTON_AT_TILE3 (p = 3) and JIT_DALTON_AT (p = 4)."""
    c = _fhn(p, **LANE[p])
    c["W"], _ = ra.utils.first_order_pad(_fitz, 2, p)
    _check_ll(_device(c, itg, ode_fun=_fitz), _oracle(c, itg, THETA))


# ---- device checks that need no oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", ["0", "1"])
def test_all_times_on_nodes_is_dalton_bit_for_bit(lanes, monkeypatch):
    monkeypatch.setenv("RK_DALTON_LANES", lanes)
    nodes = np.array([0, 4, 5, 17, 40])
    c = _fhn(B=5, times=4.0 * nodes / 40)
    c["times"][2] += 0.5e-10 * 0.1                              # within the tolerance of node 5: that node

    def never(h):
        raise AssertionError("prior_at is not needed when every time is a node")
    at = _device(c, "kramer", prior_at=never)
    c["times"] = np.linspace(0.0, 4.0, 41)[nodes]                 # the grid's own values: dalton's searchsorted finds them
    np.testing.assert_array_equal(at, _device(c, "kramer", fn=_module().dalton))


@pytest.mark.parametrize("itg", ["kramer", "rodeo", "schober"])
def test_dalton_at_tile_and_lane_routes_agree(itg, monkeypatch):
    c = _fhn(B=7, **FINE)
    monkeypatch.setenv("RK_DALTON_LANES", "0")
    tile = _device(c, itg)
    monkeypatch.setenv("RK_DALTON_LANES", "1")
    lane = _device(c, itg)
    print("largest relative difference", np.max(np.abs(tile - lane) / np.maximum(1.0, np.abs(lane))))
    assert np.all(np.abs(tile - lane) <= 1e-9 * np.maximum(1.0, np.abs(lane))), (tile, lane)


@pytest.mark.parametrize("lanes", ["0", "1"])
def test_two_calls_give_identical_bits(lanes, monkeypatch):
    monkeypatch.setenv("RK_DALTON_LANES", lanes)
    c = _fhn(B=70)
    np.testing.assert_array_equal(_device(c, "kramer"), _device(c, "kramer"))


@pytest.mark.parametrize("lanes", ["0", "1"])
def test_dalton_at_linear_model_is_exact_on_the_device(lanes, monkeypatch):
    from test_oracle_dalton_at import DT, N, SIGMA, T_MAX, T_MIN, TIMES as LIN_TIMES, _exact_block, _observations, _problem
    monkeypatch.setenv("RK_DALTON_LANES", lanes)
    _, W, x0, model = _problem(3, 1)
    sigma = np.array([SIGMA])
    y, D, Om = _observations(3, 1, LIN_TIMES)
    val = _module().dalton_at(None, ra.ode.higher_order, W, x0, T_MIN, T_MAX, N, interrogate_kramer, priors.ibm_init(DT, 3, sigma),
                              y, LIN_TIMES, D, Om, lambda h: ra.ibm_init(h, 3, sigma))
    _check_ll(val, _exact_block(3, x0[0], model[0][0], model[0][1], LIN_TIMES, y[:, 0, 0]), 1e-8)


@pytest.mark.parametrize("lanes", ["0", "1"])
def test_moving_an_observation_off_its_node_changes_the_value(lanes, monkeypatch):
    """No silent snapping: dalton would place 1.663 on node 17 as well."""
    monkeypatch.setenv("RK_DALTON_LANES", lanes)
    c = _fhn()
    on_node = _device(c, "kramer")
    c["times"] = c["times"].copy()
    c["times"][3] = 1.7 - 0.37 * 0.1
    moved = _device(c, "kramer")
    assert np.isfinite(on_node) and np.isfinite(moved) and abs(moved - on_node) > 1e-6 * abs(on_node), (on_node, moved)
