"""
solve_mv at p = 3 with the filtered rows packed in place (rodeo_amd/csrc/tile3_pack.hpp): four steps of 72-byte records in
three natural rows of the tile array, written by fwd_tile3_kernel's headline loop and read by bwd_mv_tile3_kernel's
producers, which at the same time overwrite them with the smoothed natural rows.

Shapes: B in {1, 3, 5} trajectories = 2, 6, 10 tiles (a lone ragged tile-wave, which never packs; full tile-waves plus a
ragged one), N around the gate (15 | 16), every N % 4 (the tail of the forward loop, 12 or 15 stripe rows per chunk) and the
chunk boundaries N - 1 = 16, 32.  RK_TILE3_PACK = 0 (read per call) is the natural-row route; both take Sigma_f's lower
triangle from the upper one, so they agree bit for bit.
"""
import numpy as np
import pytest
from oracle import scan, odes, joint_gaussian as jg, interrogations as oi

pytestmark = pytest.mark.gpu

NS = [15, 16, 17, 18, 19, 20, 31, 32, 33, 35, 50]
BS = [1, 3, 5]
CASES = [(B, N, "kramer") for B in BS for N in NS] + [(5, 35, "rodeo")]


@pytest.fixture(scope="module")
def ra():
    import rodeo_amd
    return rodeo_amd


def problem(ra, B, N):
    """FitzHugh-Nagumo, n_deriv = 3, batched theta and x0 (tests/test_gpu_solver.py's fitz_problem at step 0.05)"""
    rng = np.random.default_rng(7000 + 100 * B + N)
    theta = np.array([0.2, 0.2, 3.0]) * np.exp(0.1 * rng.standard_normal((B, 3)))
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, 3)
    x0 = init(np.array([-1., 1.]) + 0.1 * rng.standard_normal((B, 2)), 0.0, theta=theta)
    t_max = 0.05 * N
    prior = ra.ibm_init(t_max / N, 3, np.array([.1, .1]))
    return dict(W=W, x0=x0, theta=theta, prior=prior, args=(W, x0, 0.0, t_max, N))


def _state(plan):
    m, v = plan.state_host()
    return np.array(m), np.array(v)


@pytest.mark.parametrize("B,N,name", CASES)
def test_packed_solve_mv(ra, monkeypatch, B, N, name):
    g, o = getattr(ra.interrogate, "interrogate_" + name), getattr(oi, "interrogate_" + name)
    s = problem(ra, B, N)
    new_plan = lambda: ra.SolvePlan(ra.ode.fitzhugh_nagumo, *s["args"], g, s["prior"], theta=s["theta"])
    monkeypatch.delenv("RK_TILE3_PACK", raising=False)
    plan = new_plan()
    plan.mv(None)
    assert plan.layout == ra._lib.LAYOUT_TILE3
    m, v = _state(plan)
    # (a) the oracle, at the bounds of test_gpu_solver.py::test_fitz_mv_and_filter_parity
    mo, vo = scan.solve_mv(None, odes.fitzhugh_nagumo, *s["args"], o, s["prior"], theta=s["theta"])
    assert m.shape == mo.shape == (B, N + 1, 2, 3) and v.shape == vo.shape
    em, ev = np.max(np.abs(m - mo)), np.max(np.abs(v - vo)) / np.max(np.abs(vo))
    print(f"B {B} N {N} {name}: max|mean - oracle| {em:.3e}, max|var - oracle| / max|var| {ev:.3e}")
    assert em < 1e-9
    assert ev <= 1e-9
    assert jg.rel_err(mo, m) < 5e-8 and jg.rel_err(vo, v) < 5e-8
    # (c) the two natural rows: time 0 is the initial value, time N the filter's last row
    np.testing.assert_array_equal(m[:, 0], s["x0"])
    assert np.all(v[:, 0] == 0)
    # (d) the same plan: filter-only leaves no packed residue in its natural rows, and mv again gives the same bits
    plan.filter(None)
    mf, vf = _state(plan)
    np.testing.assert_allclose(m[:, -1], mf[:, -1], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(v[:, -1], vf[:, -1], rtol=1e-9, atol=1e-9)
    plan.mv(None)
    m2, v2 = _state(plan)
    np.testing.assert_array_equal(m2, m); np.testing.assert_array_equal(v2, v)
    fresh = new_plan()
    fresh.filter(None)
    mf2, vf2 = _state(fresh)
    np.testing.assert_array_equal(mf, mf2); np.testing.assert_array_equal(vf, vf2)
    # (b) the natural-row route, a fresh plan: bit for bit
    monkeypatch.setenv("RK_TILE3_PACK", "0")
    nat = new_plan()
    nat.mv(None)
    m0, v0 = _state(nat)
    np.testing.assert_array_equal(m0, m); np.testing.assert_array_equal(v0, v)
    nat.filter(None)
    mf0, vf0 = _state(nat)
    np.testing.assert_array_equal(mf0, mf); np.testing.assert_array_equal(vf0, vf)


def test_other_tile3_callers_keep_the_natural_rows(ra, monkeypatch):
    """(e) solve_sim and Fenrir run the same forward kernel and read whole natural tiles: at the bounds of their own tests
    (test_gpu_solver.py::test_solve_sim_parity, test_gpu_inference.py::test_fenrir_tile_short_horizons), with and without
    the switch."""
    from oracle import fenrir as ofen
    B, N = 3, 33
    s = problem(ra, B, N)
    t_max = s["args"][3]
    rng = np.random.default_rng(5)
    obs_times = np.array([0.0, 0.05 * (N // 2), t_max])
    y = rng.standard_normal((3, 2, 1))
    Dw = np.zeros((3, 2, 1, 3)); Dw[..., 0] = 1.0
    Om = np.full((3, 2, 1, 1), 0.01)
    xo = scan.solve_sim(42, odes.fitzhugh_nagumo, *s["args"], oi.interrogate_kramer, s["prior"], theta=s["theta"])
    ref = ofen.fenrir(None, odes.fitzhugh_nagumo, *s["args"], oi.interrogate_kramer, s["prior"], y, obs_times, Dw, Om, theta=s["theta"])
    got = []
    for switch in (None, "0"):
        monkeypatch.delenv("RK_TILE3_PACK", raising=False)
        if switch is not None:
            monkeypatch.setenv("RK_TILE3_PACK", switch)
        x = ra.solve_sim(42, ra.ode.fitzhugh_nagumo, *s["args"], ra.interrogate.interrogate_kramer, s["prior"], theta=s["theta"])
        assert x.shape == xo.shape == (B, N + 1, 2, 3)
        assert np.max(np.abs(x - xo)) < 1e-7
        val = ra.inference.fenrir(None, ra.ode.fitzhugh_nagumo, *s["args"], ra.interrogate.interrogate_kramer, s["prior"], y,
                                  obs_times, Dw, Om, theta=s["theta"])
        np.testing.assert_allclose(val, ref, rtol=1e-7, atol=1e-7)
        got.append((np.array(x), np.array(val)))
    np.testing.assert_array_equal(got[0][0], got[1][0]); np.testing.assert_array_equal(got[0][1], got[1][1])
