"""
``rodeo_amd.inference.fenrir.fenrir_at`` on the device (Fenrir's log-likelihood with the observations at their own times)
against its NumPy restatement tests/fenrir_at_oracle.py, on the MFMA-tile route (fenrir_at_hops_kernel +
fenrir_bwd_at_tile3_kernel) and the lane-per-trajectory route (fenrir_at_hops_kernel + fenrir_bwd_at_kernel;
``RK_FENRIR_AT_LANES=1`` forces it where the tiles serve).

The tile consumer walks the steps N-1 .. 1 in chunks of 16 (N = 72: 71..56, 55..40, 39..24, 23..8, 7..1), so the base case puts
off-grid observations into the intervals 71 (the first step processed), 40 and 39 (last step of a full chunk, first of the
next), 1 (the last loop step) and 0 (after the loop), three into interval 50, and observations on the nodes t_min and t_max;
chunk 23..8 stays clear, so the branch-free chain runs between chunks on the per-step path.
"""
import functools
import sys
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd.interrogate import interrogate_kramer, interrogate_rodeo, interrogate_schober
from oracle import odes, priors, interrogations as oi
import fenrir_at_oracle as fat

pytestmark = pytest.mark.gpu

ITG = {"kramer": (interrogate_kramer, oi.interrogate_kramer), "rodeo": (interrogate_rodeo, oi.interrogate_rodeo),
       "schober": (interrogate_schober, oi.interrogate_schober)}
THETA = np.array([0.2, 0.2, 3.0])
ROUTES = pytest.mark.parametrize("lanes", ["0", "1"], ids=["tiles", "lanes"])
BASE = dict(N=72, t_max=4.0)
FINE = dict(N=80, t_max=2.0)      # dt = 0.025, where schober's filter stays finite for every theta (tests/test_gpu_dalton.py)
# (grids and prior scales of tests/test_gpu_dalton_at.py's lane shapes)
LANE = {2: {}, 3: {}, 4: dict(N=20, sigma=10.0), 5: dict(N=20, sigma=10.0), 6: dict(N=10, t_max=2.0, sigma=1000.0)}
# seven observations as fractions of t_max (tests/test_gpu_dalton_at.py's TIMES / 4): on nodes and between them on LANE's grids
SPREAD = np.array([0.4, 0.537, 1.062, 1.7, 2.251, 2.918, 3.649]) / 4.0


def _module():
    import rodeo_amd.inference.fenrir  # noqa: F401
    return sys.modules["rodeo_amd.inference.fenrir"]


def _chunk_times(N, t_max):
    """The base case's placements for a grid of N >= 48 steps, in units of dt."""
    a = N - 1 - 31                                                 # last step of the second chunk; a - 1 opens the third
    u = np.array([0.0, 0.4, 1.55, a - 1 + 0.3, a + 0.7, a + 10.2, a + 10.5, a + 10.81, N - 1 + 0.37, N])
    t = u * (t_max / N)
    t[-1] = t_max
    return t


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


def _fhn(p=3, N=72, t_max=4.0, B=None, n_bobs=1, times=None, sigma=0.1):
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    thetas = THETA if B is None else THETA * (1 + 0.01 * (np.arange(B) % 7))[:, None]
    x0 = init(np.array([-1.0, 1.0]), 0.0, theta=THETA)
    sig = np.array([sigma, sigma])
    times = _chunk_times(N, t_max) if times is None else np.asarray(times, dtype=np.float64)
    return dict(W=W, x0=x0, N=N, t_max=t_max, p=p, sigma=sig, prior=priors.ibm_init(t_max / N, p, sig), thetas=thetas,
                times=times, obs=_obs(times, 2, p, n_bobs))


def _device(c, itg, ode_fun=ra.ode.fitzhugh_nagumo, prior_at=None, fn=None):
    y, D, Om = c["obs"]
    if prior_at is None:
        def prior_at(h):
            return ra.ibm_init(h, c["p"], c["sigma"])
    if fn is None:
        return _module().fenrir_at(None, ode_fun, c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[itg][0], c["prior"], y,
                                   c["times"], D, Om, prior_at, theta=c["thetas"])
    return fn(None, ode_fun, c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[itg][0], c["prior"], y, c["times"], D, Om,
              theta=c["thetas"])


def _oracle(c, itg, theta, ode=odes.fitzhugh_nagumo, sigma=None, prior=None):
    y, D, Om = c["obs"]
    sigma = c["sigma"] if sigma is None else sigma
    return fat.fenrir_at(ode, c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[itg][1], c["prior"] if prior is None else prior, y,
                         c["times"], D, Om, lambda h: priors.ibm_init(h, c["p"], sigma), theta=theta)


@functools.lru_cache(maxsize=None)
def _base_reference(itg, k):
    """The restatement of the base case (FINE's grid for schober) for the k-th of the seven parameter sets; computed once."""
    c = _fhn(B=7, **(FINE if itg == "schober" else BASE))
    return _oracle(c, itg, c["thetas"][k])


def _check_ll(val, ref, rtol=1e-7):
    print(f"device {val!r}, oracle {ref!r}, relative difference {abs(val - ref) / max(1.0, abs(ref)):.3e}")
    assert abs(val - ref) <= rtol * max(1.0, abs(ref)), (val, ref)


def test_the_base_case_covers_the_chunk_boundaries():
    for grid, want in ((BASE, [0, 1, 39, 40, 50, 50, 50, 71]), (FINE, [0, 1, 47, 48, 58, 58, 58, 79])):
        t = _chunk_times(**grid)
        node = np.floor(t[1:-1] / (grid["t_max"] / grid["N"]) + 1e-9).astype(int)
        assert list(node) == want and t[0] == 0.0 and t[-1] == grid["t_max"]
        assert not any(8 <= n <= 23 for n in node) if grid is BASE else not any(16 <= n <= 31 for n in node)


@ROUTES
@pytest.mark.parametrize("itg", ["kramer", "rodeo", "schober"])
def test_fenrir_at_base_case_single_and_batched(itg, lanes, monkeypatch):
    monkeypatch.setenv("RK_FENRIR_AT_LANES", lanes)
    grid = FINE if itg == "schober" else BASE
    val = _device(_fhn(**grid), itg)
    assert isinstance(val, float)
    _check_ll(val, _base_reference(itg, 0))
    vals = _device(_fhn(B=3, **grid), itg)
    assert vals.shape == (3,)
    for b in range(3):
        _check_ll(vals[b], _base_reference(itg, b))


@ROUTES
def test_fenrir_at_batch_spanning_waves(lanes, monkeypatch):
    """B = 70: 35 workgroups of four tiles on the tile route, three waves (a ragged last one) on the lanes."""
    monkeypatch.setenv("RK_FENRIR_AT_LANES", lanes)
    vals = _device(_fhn(B=70), "kramer")
    assert vals.shape == (70,)
    for b in range(70):
        _check_ll(vals[b], _base_reference("kramer", b % 7))     # (the parameters repeat with period 7)


@ROUTES
def test_fenrir_at_batched_sigma(lanes, monkeypatch):
    """A prior scale per trajectory: R batched, Q shared, in prior_pars and in what prior_at returns."""
    monkeypatch.setenv("RK_FENRIR_AT_LANES", lanes)
    c = _fhn(B=3)
    sig = np.array([[0.1, 0.1], [0.15, 0.08], [0.07, 0.2]])
    c["prior"] = ra.ibm_init(c["t_max"] / c["N"], 3, sig)
    assert c["prior"][0].ndim == 3 and c["prior"][1].ndim == 4
    vals = _device(c, "kramer", prior_at=lambda h: ra.ibm_init(h, 3, sig))
    for b in range(3):
        _check_ll(vals[b], _oracle(c, "kramer", c["thetas"][b], sigma=sig[b], prior=priors.ibm_init(c["t_max"] / c["N"], 3, sig[b])))


@ROUTES
def test_fenrir_at_one_full_chunk(lanes, monkeypatch):
    """N = 17: the steps 16 .. 1 are one full chunk, with observations in its first and its last interval."""
    monkeypatch.setenv("RK_FENRIR_AT_LANES", lanes)
    dt = 1.0 / 17
    c = _fhn(N=17, t_max=1.0, times=[1.45 * dt, 16.62 * dt])
    _check_ll(_device(c, "kramer"), _oracle(c, "kramer", THETA))


@ROUTES
@pytest.mark.parametrize("N", [1, 2])
def test_fenrir_at_short_horizons(N, lanes, monkeypatch):
    """An observation in the first interval and one in the last (the same interval at N = 1)."""
    monkeypatch.setenv("RK_FENRIR_AT_LANES", lanes)
    t_max = 0.1 * N
    c = _fhn(N=N, t_max=t_max, times=[0.031, t_max - 0.042])
    _check_ll(_device(c, "kramer"), _oracle(c, "kramer", THETA))


def _lorenz():
    N, t_max, p = 60, 1.2, 3
    W, init = ra.utils.first_order_pad(ra.ode.lorenz63, 3, p)
    theta = np.array([28.0, 10.0, 8.0 / 3.0])
    x0 = init(np.array([-12.0, -5.0, 38.0]), 0.0, theta=theta)
    sig = np.array([5.0] * 3)
    times = np.array([0.0, 0.013, 0.113, 0.4, 0.617, 0.625, 1.191, 1.2])
    y, D, Om = _obs(times, 3, p, 1)
    y = y + x0[None, :, :1]
    prior = priors.ibm_init(t_max / N, p, sig)

    def device():
        return _module().fenrir_at(None, ra.ode.lorenz63, W, x0, 0.0, t_max, N, interrogate_kramer, prior, y, times, D, Om,
                                   lambda h: ra.ibm_init(h, p, sig), theta=theta)

    def oracle():
        return fat.fenrir_at(odes.lorenz63, W, x0, 0.0, t_max, N, oi.interrogate_kramer, prior, y, times, D, Om,
                             lambda h: priors.ibm_init(h, p, sig), theta=theta)
    return device, oracle


@ROUTES
def test_fenrir_at_lorenz_three_blocks(lanes, monkeypatch):
    monkeypatch.setenv("RK_FENRIR_AT_LANES", lanes)
    device, oracle = _lorenz()
    val = device()
    _check_ll(val, oracle())
    # three blocks are three atomic addends per trajectory: their order may differ between two calls, by rounding only
    again = device()
    assert abs(val - again) <= 1e-12 * max(1.0, abs(val)), (val, again)


# (kramer where its filter is stable on these grids, as in tests/test_gpu_dalton_at.py)
@pytest.mark.parametrize("p,n_bobs,itg", [(3, 2, "rodeo"), (2, 1, "rodeo"), (4, 1, "rodeo"), (5, 2, "rodeo"), (6, 3, "rodeo"),
                                          (3, 2, "kramer"), (2, 1, "kramer"), (4, 1, "kramer")])
def test_fenrir_at_lane_shapes(p, n_bobs, itg):
    g = dict(dict(N=40, t_max=4.0), **LANE[p])
    c = _fhn(p, n_bobs=n_bobs, times=SPREAD * g["t_max"], **g)
    _check_ll(_device(c, itg), _oracle(c, itg, THETA))


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


@pytest.mark.parametrize("itg", ["kramer", "rodeo"])
@pytest.mark.parametrize("p", [3, 4])
def test_fenrir_at_traced_python_rhs(p, itg):
    """A Python right-hand side: its forward filter is a hiprtc build (the tile form at p = 3), the backward kernels are the
    library's."""
    g = dict(dict(N=40, t_max=4.0), **LANE[p])
    c = _fhn(p, times=SPREAD * g["t_max"], **g)
    c["W"], _ = ra.utils.first_order_pad(_fitz, 2, p)
    _check_ll(_device(c, itg, ode_fun=_fitz), _oracle(c, itg, THETA))


# ---- device checks that need no oracle -------------------------------------------------------------------------------------
@ROUTES
@pytest.mark.parametrize("p", [3, 4])
def test_all_times_on_nodes_is_fenrir_bit_for_bit(p, lanes, monkeypatch):
    """The call is then ``fenrir`` itself on those nodes, whatever the switch says (p = 4: fenrir's blocked-tile route)."""
    monkeypatch.setenv("RK_FENRIR_AT_LANES", lanes)
    nodes = np.array([0, 4, 5, 17, 40])
    c = _fhn(p, B=5, N=40, times=4.0 * nodes / 40, sigma=LANE[p].get("sigma", 0.1))
    c["times"][2] += 0.5e-10 * 0.1                              # within the tolerance of node 5: that node

    def never(h):
        raise AssertionError("prior_at is not needed when every time is a node")
    at = _device(c, "kramer", prior_at=never)
    c["times"] = np.linspace(0.0, 4.0, 41)[nodes]                 # the grid's own values: fenrir's searchsorted finds them
    np.testing.assert_array_equal(at, _device(c, "kramer", fn=ra.inference.fenrir))


@pytest.mark.parametrize("itg", ["kramer", "rodeo", "schober"])
def test_fenrir_at_tile_and_lane_routes_agree(itg, monkeypatch):
    c = _fhn(B=7, **(FINE if itg == "schober" else BASE))
    monkeypatch.setenv("RK_FENRIR_AT_LANES", "0")
    tile = _device(c, itg)
    monkeypatch.setenv("RK_FENRIR_AT_LANES", "1")
    lane = _device(c, itg)
    print("largest relative difference", np.max(np.abs(tile - lane) / np.maximum(1.0, np.abs(lane))))
    assert np.all(np.abs(tile - lane) <= 1e-9 * np.maximum(1.0, np.abs(lane))), (tile, lane)


@ROUTES
def test_the_routes_run_their_own_kernels(lanes, monkeypatch):
    monkeypatch.setenv("RK_FENRIR_AT_LANES", lanes)
    dev = ra.default_device()
    dev.profile_enable(True)
    try:
        _device(_fhn(), "kramer")
        names = [k for k, _ in dev.profile_last()]
    finally:
        dev.profile_enable(False)
    want = "fenrir_bwd_at_kernel" if lanes == "1" else "fenrir_bwd_at_tile3_kernel"
    assert "fenrir_at_hops_kernel" in names and want in names, names


@ROUTES
def test_two_calls_give_identical_bits(lanes, monkeypatch):
    """Two blocks are two atomic addends onto zero per trajectory, and a + b = b + a: the same bits on both routes."""
    monkeypatch.setenv("RK_FENRIR_AT_LANES", lanes)
    c = _fhn(B=70)
    np.testing.assert_array_equal(_device(c, "kramer"), _device(c, "kramer"))


@ROUTES
def test_fenrir_at_linear_model_is_exact_on_the_device(lanes, monkeypatch):
    from test_oracle_dalton_at import DT, N, SIGMA, T_MAX, T_MIN, _exact_block, _observations, _problem
    from test_oracle_fenrir_at import TIMES as LIN_TIMES
    monkeypatch.setenv("RK_FENRIR_AT_LANES", lanes)
    _, W, x0, model = _problem(3, 1)
    sigma = np.array([SIGMA])
    y, D, Om = _observations(3, 1, LIN_TIMES)
    val = _module().fenrir_at(None, ra.ode.higher_order, W, x0, T_MIN, T_MAX, N, interrogate_kramer, priors.ibm_init(DT, 3, sigma),
                              y, LIN_TIMES, D, Om, lambda h: ra.ibm_init(h, 3, sigma))
    _check_ll(val, _exact_block(3, x0[0], model[0][0], model[0][1], LIN_TIMES, y[:, 0, 0]), 1e-8)


@ROUTES
def test_moving_an_observation_off_its_node_changes_the_value(lanes, monkeypatch):
    """No silent snapping: fenrir would place 1.663 on node 17 as well."""
    monkeypatch.setenv("RK_FENRIR_AT_LANES", lanes)
    c = _fhn(N=40, times=[0.4, 0.537, 1.7, 2.918])
    on_node = _device(c, "kramer")
    c["times"] = c["times"].copy()
    c["times"][2] = 1.7 - 0.37 * 0.1
    moved = _device(c, "kramer")
    assert np.isfinite(on_node) and np.isfinite(moved) and abs(moved - on_node) > 1e-6 * abs(on_node), (on_node, moved)
