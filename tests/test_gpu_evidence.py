"""
``rodeo_amd.solve_evidence`` on the device against the NumPy restatement tests/evidence_oracle.py, on its three routes: the
p = 3 MFMA tiles (evidence_tile3_kernels.hpp), the lanes of the standard form and of the square-root form
(evidence_kernels.hpp).  Bars for logdens, quad and logdet: 1e-7 max(1, |ref|) for n_bstate <= 4, 1e-5 for 5 and 6, 1e-4 for
7 and 8 (those of test_fenrir_parity_square_root).  Every comparison prints its largest difference in units of
max(1, |ref|) ("evidence-check ..." lines: profiles/evidence_checks.txt keeps them).
"""
import functools
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd.interrogate import interrogate_kramer, interrogate_rodeo, interrogate_schober
from oracle import odes, interrogations as oi
import evidence_oracle as evo

pytestmark = pytest.mark.gpu

ITG = {"kramer": (interrogate_kramer, oi.interrogate_kramer), "rodeo": (interrogate_rodeo, oi.interrogate_rodeo),
       "schober": (interrogate_schober, oi.interrogate_schober)}
THETA = np.array([0.2, 0.2, 3.0])
SIGMA = np.array([0.5, 0.3])
LORENZ = np.array([28.0, 10.0, 8.0 / 3.0])


def _bar(p):
    return 1e-7 if p <= 4 else (1e-5 if p <= 6 else 1e-4)


@functools.lru_cache(maxsize=None)
def _fhn(p, N, t_max, B=None, batched_sigma=False, form="standard"):
    """The quick start's FitzHugh-Nagumo problem; a batch varies theta, the initial value and (batched_sigma) sigma."""
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    if B is None:
        theta, v0, sigma = THETA, np.array([-1.0, 1.0]), SIGMA
    else:
        k = np.arange(B)[:, None]
        theta = THETA * (1 + 0.002 * k)
        v0 = np.array([-1.0, 1.0]) + 0.001 * k
        sigma = SIGMA * (1 + 0.01 * k) if batched_sigma else SIGMA
    x0 = init(v0, 0.0, theta=theta)
    Q, R = ra.ibm_init(t_max / N, p, sigma)
    if form == "square-root":
        if p >= 7:                                      # the IBM variance is singular in fp64 there: a well-conditioned factor
            R = np.tril(0.02 * np.random.default_rng(40 + p).standard_normal((2, p, p))) + np.eye(p) * 0.1
        else:
            R = np.linalg.cholesky(R)
    return dict(ode=ra.ode.fitzhugh_nagumo, oracle_ode=odes.fitzhugh_nagumo, W=W, x0=x0, N=N, t_max=t_max, prior=(Q, R),
                theta=theta, form=form, p=p)


@functools.lru_cache(maxsize=None)
def _lorenz(p, B=None, form="standard", N=60, t_max=1.2):
    W, init = ra.utils.first_order_pad(ra.ode.lorenz63, 3, p)
    theta = LORENZ if B is None else LORENZ * (1 + 0.002 * np.arange(B)[:, None])
    v0 = np.array([-12.0, -5.0, 38.0])
    x0 = init(v0 if B is None else v0 + 0.01 * np.arange(B)[:, None], 0.0, theta=theta)
    Q, R = ra.ibm_init(t_max / N, p, np.array([5.0, 4.0, 6.0]))
    if form == "square-root":
        R = np.linalg.cholesky(R)
    return dict(ode=ra.ode.lorenz63, oracle_ode=odes.lorenz63, W=W, x0=x0, N=N, t_max=t_max, prior=(Q, R), theta=theta,
                form=form, p=p)


def _device(c, name, ode=None, prior=None):
    return ra.solve_evidence(None, ode or c["ode"], c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[name][0], prior or c["prior"],
                             kalman_type=c["form"], theta=c["theta"])


_refs = {}


def _oracle(c, name):
    """The restatement of a case, computed once (the cases are cached objects)."""
    key = (id(c), name)
    if key not in _refs:
        _refs[key] = evo.evidence(c["oracle_ode"], c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[name][1], c["prior"], c["form"],
                                  theta=c["theta"])
    return _refs[key]


def _check(ev, ref, bar, label):
    worst = 0.0
    for got, want in zip((ev.logdens, ev.quad, ev.logdet), ref):
        assert np.shape(got) == np.shape(want), (np.shape(got), np.shape(want))
        worst = max(worst, float(np.max(np.abs(np.asarray(got) - want) / np.maximum(1.0, np.abs(want)))))
    print(f"evidence-check {label}: largest difference {worst:.3e} of max(1, |ref|), bar {bar:.0e}")
    assert worst <= bar, (label, worst)


def _same_bits(c, name, first):
    again = _device(c, name)
    for a, b in zip(first[:3], again[:3]):
        np.testing.assert_array_equal(a, b)


# ---- tiles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,t_max", [("kramer", 72, 4.0), ("rodeo", 72, 4.0), ("schober", 80, 2.0)])
def test_tiles_fitzhugh(name, N, t_max):
    """Unbatched (a float comes back), a half-filled wave, several workgroups with a batched sigma; identical bits."""
    one = _fhn(3, N, t_max)
    ev = _device(one, name)
    assert isinstance(ev.logdens, float) and ev.quad.shape == (2,) and ev.logdet.shape == (2,) and ev.n_steps == N
    _check(ev, _oracle(one, name), _bar(3), f"tiles fhn {name} N={N} unbatched")
    for B, bs in ((3, False), (70, True)):
        c = _fhn(3, N, t_max, B, bs)
        ev = _device(c, name)
        assert ev.logdens.shape == (B,) and ev.quad.shape == (B, 2)
        _check(ev, _oracle(c, name), _bar(3), f"tiles fhn {name} N={N} B={B}")
    _same_bits(c, name, ev)


@pytest.mark.parametrize("N", [1, 2, 17])
def test_tiles_short_horizons(N):
    c = _fhn(3, N, 0.1 * N, 3)
    _check(_device(c, "kramer"), _oracle(c, "kramer"), _bar(3), f"tiles fhn kramer N={N} B=3")


@pytest.mark.parametrize("name", ["kramer", "rodeo"])
def test_tiles_lorenz_three_blocks(name):
    """d = 3: the tile3 form of the right-hand side, one trajectory per wave; identical bits at d = 3."""
    one = _lorenz(3)
    _check(_device(one, name), _oracle(one, name), _bar(3), f"tiles lorenz {name} unbatched")
    c = _lorenz(3, 5)
    ev = _device(c, name)
    assert ev.quad.shape == (5, 3)
    _check(ev, _oracle(c, name), _bar(3), f"tiles lorenz {name} B=5")
    _same_bits(c, name, ev)


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


def test_tiles_traced_python_right_hand_side():
    """The README's plain-Python ode_fun: the hiprtc build of the tile kernel (the generic step, no tile form)."""
    c = _fhn(3, 72, 4.0, 3)
    _check(_device(c, "kramer", ode=_fitz), _oracle(c, "kramer"), _bar(3), "tiles traced fhn kramer B=3")


def _kernels(call):
    """Names of the kernels that `call` launched (the handle's per-launch profile)."""
    dev = ra.default_device()
    dev.profile_enable(True)
    try:
        call()
        return [name for name, _ in dev.profile_last()]
    finally:
        dev.profile_enable(False)


def test_each_route_runs_its_own_kernel(monkeypatch):
    """The comparisons above cannot tell a route from another that computes the same numbers: the launch's name does."""
    monkeypatch.setenv("RK_EVIDENCE_LANES", "0")
    c, sq = _fhn(3, 72, 4.0, 3), _fhn(3, 40, 2.0, 3, False, "square-root")
    assert _kernels(lambda: _device(c, "kramer")) == ["evidence_tile3_kernel"]
    assert _kernels(lambda: _device(_lorenz(3, 5), "kramer")) == ["evidence_tile3_kernel"]
    assert _kernels(lambda: _device(c, "kramer", ode=_fitz)) == ["evidence_tile3_kernel<user>"]
    assert _kernels(lambda: _device(_fhn(4, 40, 2.0, 3), "kramer")) == ["evidence_kernel"]
    assert _kernels(lambda: _device(_fhn(4, 40, 2.0, 3), "kramer", ode=_fitz)) == ["evidence_kernel<user>"]
    assert _kernels(lambda: _device(sq, "kramer")) == ["evidence_sqrt_kernel"]
    assert _kernels(lambda: _device(sq, "kramer", ode=_fitz)) == ["evidence_sqrt_kernel<user>"]
    monkeypatch.setenv("RK_EVIDENCE_LANES", "1")
    assert _kernels(lambda: _device(c, "kramer")) == ["evidence_kernel"]
    assert _kernels(lambda: _device(c, "kramer", ode=_fitz)) == ["evidence_kernel<user>"]


# ---- lanes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,name", [(2, "kramer"), (3, "rodeo"), (4, "kramer"), (5, "rodeo"), (6, "rodeo")])
def test_lanes(p, name, monkeypatch):
    if p == 3:
        monkeypatch.setenv("RK_EVIDENCE_LANES", "1")
    c = _fhn(p, 40, 2.0, 70, True)
    ev = _device(c, name)
    _check(ev, _oracle(c, name), _bar(p), f"lanes fhn {name} p={p} B=70")
    _same_bits(c, name, ev)


def test_lanes_lorenz_and_traced_right_hand_side():
    c = _lorenz(5, 5, N=40, t_max=0.2)                             # (three blocks at their largest n_bstate; a short horizon: the
    _check(_device(c, "rodeo"), _oracle(c, "rodeo"), _bar(5), "lanes lorenz rodeo p=5 B=5")       # filter leaves the attractor later)
    c = _fhn(4, 40, 2.0, 3)
    _check(_device(c, "kramer", ode=_fitz), _oracle(c, "kramer"), _bar(4), "lanes traced fhn kramer p=4 B=3")


@pytest.mark.parametrize("name", ["kramer", "rodeo", "schober"])
def test_tile_route_against_lane_route(name, monkeypatch):
    cases = [_fhn(3, 80, 2.0, 70, True), _lorenz(3, 5)] if name != "schober" else [_fhn(3, 80, 2.0, 70, True)]
    for c in cases:
        monkeypatch.setenv("RK_EVIDENCE_LANES", "0")
        tile = _device(c, name)
        monkeypatch.setenv("RK_EVIDENCE_LANES", "1")
        lane = _device(c, name)
        worst = max(float(np.max(np.abs(t - l) / np.abs(l))) for t, l in zip(tile[:3], lane[:3]))
        print(f"evidence-check tile against lane {name} d={c['W'].shape[0]}: largest relative difference {worst:.3e}, bar 1e-09")
        assert worst <= 1e-9, worst


# ---- square-root lanes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,B,name", [(3, 5, "kramer"), (3, 5, "schober"), (3, 70, "rodeo"), (5, 5, "rodeo"), (5, 70, "kramer"),
                                      (8, 5, "kramer"), (8, 70, "rodeo")])
def test_square_root(p, B, name):
    c = _fhn(p, 40, 2.0, B, p < 7, "square-root")
    ev = _device(c, name)
    _check(ev, _oracle(c, name), _bar(p), f"square-root fhn {name} p={p} B={B}")
    if B == 70:
        _same_bits(c, name, ev)


def test_square_root_lorenz_idle_lanes():
    """d = 3 at B = 23: 21 trajectories per wave, so a wave with idle lanes and a second workgroup."""
    c = _lorenz(3, 23, "square-root")
    ev = _device(c, "kramer")
    assert ev.quad.shape == (23, 3)
    _check(ev, _oracle(c, "kramer"), _bar(3), "square-root lorenz kramer p=3 B=23")
    _same_bits(c, "kramer", ev)


@pytest.mark.parametrize("p", [3, 8])
def test_square_root_traced_python_right_hand_side(p):
    """A Python ode_fun has the built-in right-hand sides' range in the square-root form, n_bstate 8 included."""
    c = _fhn(p, 40, 2.0, 3, False, "square-root")
    _check(_device(c, "kramer", ode=_fitz), _oracle(c, "kramer"), _bar(p), f"square-root traced fhn kramer p={p} B=3")


def test_square_root_against_standard_under_kramer():
    std, sq = _fhn(3, 40, 2.0, 70, True), _fhn(3, 40, 2.0, 70, True, "square-root")
    a, b = _device(std, "kramer"), _device(sq, "kramer")
    worst = max(float(np.max(np.abs(x - y) / np.maximum(1.0, np.abs(x)))) for x, y in zip(a[:3], b[:3]))
    print(f"evidence-check square-root against standard kramer p=3: largest difference {worst:.3e}, bar 1e-06")
    assert worst <= 1e-6, worst


# ---- end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,form,lanes", [(3, "standard", False), (3, "standard", True), (4, "standard", False),
                                          (3, "square-root", False)])
def test_calibration_on_the_device(p, form, lanes, monkeypatch):
    """Run, rescale sigma by sqrt(evidence_scale), run again: quad / N = 1 and the second log-evidence is the one
    ``evidence_at`` predicted from the first."""
    monkeypatch.setenv("RK_EVIDENCE_LANES", "1" if lanes else "0")
    c = _fhn(p, 72, 4.0, 3, False, form)
    first = _device(c, "kramer")
    scale = ra.evidence_scale(first)                                # (B, d)
    assert scale.shape == (3, 2) and np.all(scale > 1.0)            # sigma = (0.5, 0.3) is too small on this problem
    Q, R = c["prior"]
    grow = (np.sqrt(scale) if form == "square-root" else scale)[:, :, None, None]     # sigma * sqrt(c): R * c, the factor * sqrt(c)
    second = _device(c, "kramer", prior=(Q, R * grow))
    off = float(np.max(np.abs(ra.evidence_scale(second) - 1.0)))
    pred = ra.evidence_at(first, scale)
    rel = float(np.max(np.abs(second.logdens - pred) / np.abs(pred)))
    print(f"evidence-check calibration p={p} {form} lanes={lanes}: |quad / N - 1| {off:.3e}, logdens against evidence_at {rel:.3e}, "
          "bars 1e-09")
    assert off <= 1e-9 and rel <= 1e-9
    assert np.all(second.logdens > first.logdens)
    np.testing.assert_allclose(ra.evidence_at(first, np.ones(2)), first.logdens, rtol=1e-15)
