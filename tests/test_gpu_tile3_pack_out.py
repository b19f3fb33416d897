"""
solve_mv at p = 3 with the SMOOTHED rows packed in place (RK_FLAG_TILE3_PACKED_MV -> RK_LAYOUT_TILE3_PACKED,
include/rodeo_kalman.h): bwd_mv_tile3_kernel's chain wave stores the smoothed state of step n as a 72-byte record over the
filtered record of step n (rodeo_amd/csrc/tile3_pack.hpp); rows 0 and N stay natural tiles.  ``SolvePlan.mv()`` asks for it
at n_bstate = 3; the host gathers (``state_host``, ``mean_rows_host``) and the device readers (``rk_gauss_obs_logpost``,
``rk_eval_at``) read both forms.

Shapes: B in {1, 3, 5} trajectories = 2, 6, 10 tiles (a lone ragged tile-wave, which never packs; full tile-waves plus a
ragged one), N around the gate (15 | 16), every (N - 1) & 3 (the four per-lane store offsets), the chunk boundaries N - 1 =
16, 32 and partial last chunks (the pointer path).  Inputs: tests/test_gpu_tile3_pack.py's ``problem()``, rebuilt here.
RK_TILE3_PACK = 0 (read per call) is the natural-row route; smoothed p = 3 results take Sigma's lower triangle from the upper
one in both layouts, so the two agree bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest
from oracle import scan, odes, joint_gaussian as jg, interrogations as oi

pytestmark = pytest.mark.gpu

NS = [15, 16, 17, 18, 19, 20, 31, 32, 33, 35, 50]
BS = [1, 3, 5]
CASES = [(B, N, "kramer") for B in BS for N in NS] + [(5, 35, "rodeo")]
SIGMA = np.array([.1, .1])


@pytest.fixture(scope="module")
def ra():
    import rodeo_amd
    return rodeo_amd


def problem(ra, B, N):
    """FitzHugh-Nagumo, n_deriv = 3, batched theta and x0 (tests/test_gpu_tile3_pack.py's problem())"""
    rng = np.random.default_rng(7000 + 100 * B + N)
    theta = np.array([0.2, 0.2, 3.0]) * np.exp(0.1 * rng.standard_normal((B, 3)))
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, 3)
    x0 = init(np.array([-1., 1.]) + 0.1 * rng.standard_normal((B, 2)), 0.0, theta=theta)
    t_max = 0.05 * N
    prior = ra.ibm_init(t_max / N, 3, SIGMA)
    return dict(W=W, x0=x0, theta=theta, prior=prior, args=(W, x0, 0.0, t_max, N))


@functools.lru_cache(maxsize=None)
def _oracle(B, N, name):
    """the reference, once per case and never written to"""
    import rodeo_amd as ra
    s = problem(ra, B, N)
    mo, vo = scan.solve_mv(None, odes.fitzhugh_nagumo, *s["args"], getattr(oi, "interrogate_" + name), s["prior"], theta=s["theta"])
    mo, vo = np.array(mo), np.array(vo)
    mo.setflags(write=False); vo.setflags(write=False)
    return mo, vo


def _state(plan):
    m, v = plan.state_host()
    return np.array(m), np.array(v)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("B,N,name", CASES)
def test_packed_smoothed_rows(ra, monkeypatch, B, N, name):
    _lib = ra._lib
    g = getattr(ra.interrogate, "interrogate_" + name)
    s = problem(ra, B, N)
    new_plan = lambda: ra.SolvePlan(ra.ode.fitzhugh_nagumo, *s["args"], g, s["prior"], theta=s["theta"])
    monkeypatch.delenv("RK_TILE3_PACK", raising=False)
    plan = new_plan()
    plan.mv(None)
    assert plan.layout == _lib.LAYOUT_TILE3 and plan.records_layout == _lib.LAYOUT_TILE3_PACKED
    assert plan.cfg.flags & _lib.FLAG_TILE3_PACKED_MV
    assert plan.packed_waves() == (2 * B // 4 if N >= 16 else 0)
    assert len(plan._bufs) == 1                                   # the packed and the natural form share ONE buffer
    m, v = _state(plan)
    # (a) the oracle, at the bounds of tests/test_gpu_tile3_pack.py
    mo, vo = _oracle(B, N, name)
    assert m.shape == mo.shape == (B, N + 1, 2, 3) and v.shape == vo.shape == (B, N + 1, 2, 3, 3)
    em, ev = np.max(np.abs(m - mo)), np.max(np.abs(v - vo)) / np.max(np.abs(vo))
    print(f"B {B} N {N} {name}: max|mean - oracle| {em:.3e}, max|var - oracle| / max|var| {ev:.3e}")
    assert em < 1e-9
    assert ev <= 1e-9
    assert jg.rel_err(mo, m) < 5e-8 and jg.rel_err(vo, v) < 5e-8
    np.testing.assert_array_equal(v, np.swapaxes(v, -1, -2))      # the mirror rule: exactly symmetric
    # (c) rows 0 and N are natural tiles: the initial value, and the filter's last row
    fresh = new_plan()
    fresh.filter(None)
    assert fresh.records_layout == _lib.LAYOUT_TILE3 and not fresh.cfg.flags & _lib.FLAG_TILE3_PACKED_MV
    mf2, vf2 = _state(fresh)
    first, last = plan.var_state.slice0_host(0), plan.var_state.slice0_host(-1)
    np.testing.assert_array_equal(first[..., 3], s["x0"])
    assert np.all(first[..., :3] == 0)
    np.testing.assert_array_equal(last, fresh.var_state.slice0_host(-1))
    np.testing.assert_array_equal(m[:, 0], s["x0"])
    np.testing.assert_array_equal(m[:, -1], mf2[:, -1])
    # (d) the same plan: mv -> filter -> mv gives the same bits, and its filter is a fresh plan's filter
    plan.filter(None)
    assert plan.records_layout == _lib.LAYOUT_TILE3 and plan.packed_waves() == 0
    mf, vf = _state(plan)
    np.testing.assert_array_equal(mf, mf2); np.testing.assert_array_equal(vf, vf2)
    plan.mv(None)
    m2, v2 = _state(plan)
    np.testing.assert_array_equal(m2, m); np.testing.assert_array_equal(v2, v)
    # (e) the readers on the packed plan: the observation log-posterior, single rows, the posterior at and between nodes
    rng = np.random.default_rng(N)
    ind = np.unique(np.concatenate([[0, 1, N - 1, N], rng.integers(0, N + 1, 6)]))
    obs = rng.standard_normal((len(ind), 2))
    t_max = s["args"][3]
    t_eval = np.concatenate([0.05 * ind, 0.05 * (rng.integers(0, N, 5) + rng.uniform(0.1, 0.9, 5)), [t_max - 0.02]])
    prior_at = lambda h: ra.ibm_init(h, 3, SIGMA)

    def readers(pl):
        lp = ra.inference.gauss_obs_logpost(pl, obs, ind, 0.3, which="mean").to_host()
        rows = pl.mean_rows_host(ind)
        at = ra.solve_mv_at(None, ra.ode.fitzhugh_nagumo, *s["args"], g, s["prior"], t_eval, prior_at, theta=s["theta"])
        return np.array(lp), np.array(rows), np.array(at[0]), np.array(at[1])

    got = readers(plan)
    np.testing.assert_array_equal(got[1], m[:, ind])
    np.testing.assert_array_equal(got[2][:, :len(ind)], m[:, ind])           # on a node: solve_mv's own value, bit for bit
    np.testing.assert_array_equal(got[3][:, :len(ind)], v[:, ind])
    z = (obs[None] - m[:, ind][..., 0]) / 0.3
    np.testing.assert_allclose(got[0], np.sum(-0.5 * z * z - np.log(0.3) - 0.5 * np.log(2 * np.pi), axis=(1, 2)), rtol=1e-12)
    # (f) the C ABI without the flag: today's bytes, i.e. natural rows everywhere
    plan.launch(plan.dev.lib.rk_solve_mv, None, _lib.MODE_MV)
    assert plan.records_layout == _lib.LAYOUT_TILE3 and not plan.cfg.flags & _lib.FLAG_TILE3_PACKED_MV
    raw_unflagged = plan.var_state.to_host()
    np.testing.assert_array_equal(raw_unflagged[..., 3], np.moveaxis(m, 0, 1))
    # (b) the natural-row route, a fresh plan: bit for bit, through state_host() and through every reader
    monkeypatch.setenv("RK_TILE3_PACK", "0")
    lay = C.c_int32(-1)
    cfg = _lib.SolveCfg.from_buffer_copy(plan.cfg)
    cfg.flags |= _lib.FLAG_TILE3_PACKED_MV
    _lib.check(plan.dev.lib.rk_solve_layout(C.byref(cfg), _lib.MODE_MV, C.byref(lay)))
    assert lay.value == _lib.LAYOUT_TILE3                           # the switch keeps the natural layout, flag or not
    nat = new_plan()
    nat.mv(None)
    assert nat.records_layout == _lib.LAYOUT_TILE3 and nat.packed_waves() == 0
    m0, v0 = _state(nat)
    np.testing.assert_array_equal(m0, m); np.testing.assert_array_equal(v0, v)
    for a, b in zip(readers(nat), got):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(_bits(nat.var_state.to_host()), _bits(raw_unflagged))       # (f): byte-identical arrays


def test_basic_reads_packed_rows(ra, monkeypatch):
    """inference.basic with a host callable downloads single rows of the packed array (SolvePlan.mean_rows_host), and with the
    Gaussian log-likelihood reduces on the device: both equal the natural-row route."""
    from rodeo_amd.inference.basic import GaussianObsLoglik
    B, N = 5, 35
    s = problem(ra, B, N)
    t_max = s["args"][3]
    obs_times = np.array([0.0, 0.05, 0.05 * 17, 0.05 * 18, t_max - 0.05, t_max])
    obs = np.random.default_rng(3).standard_normal((len(obs_times), 2))
    host = lambda obs_data, ode_data, **params: float(np.sum((obs_data - ode_data[..., 0]) ** 2))
    out = []
    for switch in (None, "0"):
        monkeypatch.delenv("RK_TILE3_PACK", raising=False)
        if switch is not None:
            monkeypatch.setenv("RK_TILE3_PACK", switch)
        vals = []
        for loglik in (host, GaussianObsLoglik(0.2)):
            ll, Xt = ra.inference.basic(None, ra.ode.fitzhugh_nagumo, *s["args"], ra.interrogate.interrogate_kramer, s["prior"],
                                        obs, obs_times, loglik, theta=s["theta"])
            vals += [np.array(ll), np.array(Xt)]
        out.append(vals)
    mo, _ = _oracle(B, N, "kramer")
    assert np.max(np.abs(out[0][1] - mo)) < 1e-9
    ind = ra.inference.obs_index(0.0, t_max, N, obs_times)
    np.testing.assert_allclose(out[0][0], np.sum((obs[None] - out[0][1][:, ind][..., 0]) ** 2, axis=(1, 2)), rtol=1e-12)
    for a, b in zip(out[0], out[1]):
        np.testing.assert_array_equal(a, b)
