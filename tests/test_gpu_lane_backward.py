"""
The five lane-per-(block, trajectory) backward kernels of the standard form -- ``bwd_mv_kernel``, ``bwd_sim_kernel``,
``dynamic_bwd_mv_kernel``, ``dynamic_bwd_sim_kernel``, ``bwd_sim_draws_kernel`` -- run one walk (csrc/lane_backward.hpp).  This
file pins, at the smallest shapes where that walk can go wrong, what they owe their oracles and each other.

Shapes: N = 1 (the loop does not run), 2 (one iteration, nothing prefetched inside the loop), 3 (the first prefetch and
rotation); FitzHugh-Nagumo (two blocks) at n_bstate 3 with B = 1 (two lanes) and B = 65 (130 lanes: two full waves and a partial
third, whose idle lanes the guard past B * D sends home), sigma batched.  The grid is test_gpu_dynamic's short-horizon one, dt =
0.025.  The samplers run under interrogate_rodeo, whose filtered variances are regular (under kramer and schober they are
singular at n_bstate 3 and the draw's factor amplifies rounding: test_gpu_dynamic.test_solve_sim_dynamic_parity).

Bars, unchanged from the tests whose oracles these are: tests/test_gpu_solver.py -- mean 1e-9 absolute, var 1e-9 of max|var|
(test_batched_ragged_sizes), sample paths 1e-7 absolute (test_solve_sim_parity); tests/test_gpu_dynamic.py -- ``_check`` at
``_bar(3)`` = 1e-7, sample paths 1e-7 absolute with sqrt(scale) and logdens at 1e-7 (test_solve_sim_dynamic_parity).  They were
set at N = 40 and more; fewer steps accumulate less rounding.  Draw s of ``solve_sim_draws`` against ``solve_sim`` under key + s
and ``x[..., 0, :, :]`` against ``ode_init`` are equalities of bits.  Every comparison prints its figure before it asserts
("lane-backward-check ..." lines).
"""
import numpy as np
import pytest
import rodeo_amd as ra
import dynamic_oracle as dyo
from oracle import scan
from test_gpu_evidence import ITG, _bar, _fhn, _kernels
from test_gpu_dynamic import _check

pytestmark = pytest.mark.gpu

P = 3
KEY = 42
SHAPES = [(N, B) for N in (1, 2, 3) for B in (1, 65)]


def _case(N, B):
    return _fhn(P, N, 0.025 * N, B, True)               # (cached: one object per shape, shared by the tests below)


def _args(c):
    return c["W"], c["x0"], 0.0, c["t_max"], c["N"]


def _sim(c, key):
    return ra.solve_sim(key, c["ode"], *_args(c), ITG["rodeo"][0], c["prior"], batch_minor=True, theta=c["theta"])


@pytest.mark.parametrize("N,B", SHAPES)
@pytest.mark.parametrize("name", ["kramer", "rodeo"])
def test_solve_mv_on_the_lanes(N, B, name):
    c = _case(N, B)
    m, v = ra.solve_mv(None, c["ode"], *_args(c), ITG[name][0], c["prior"], batch_minor=True, theta=c["theta"])
    mo, vo = scan.solve_mv(None, c["oracle_ode"], *_args(c), ITG[name][1], c["prior"], theta=c["theta"])
    assert m.shape == mo.shape == (B, N + 1, 2, P) and v.shape == vo.shape
    dm, dv = float(np.max(np.abs(m - mo))), float(np.max(np.abs(v - vo)) / np.max(np.abs(vo)))
    print(f"lane-backward-check solve_mv {name} N={N} B={B}: mean {dm:.3e} (absolute, bar 1e-09), var {dv:.3e} of max|var| "
          "(bar 1e-09)")
    assert dm < 1e-9 and dv <= 1e-9
    np.testing.assert_array_equal(m[:, 0], c["x0"])
    assert np.all(v[:, 0] == 0)


@pytest.mark.parametrize("N,B", SHAPES)
def test_solve_sim_on_the_lanes(N, B):
    c = _case(N, B)
    x = _sim(c, KEY)
    xo = scan.solve_sim(KEY, c["oracle_ode"], *_args(c), ITG["rodeo"][1], c["prior"], theta=c["theta"])
    assert x.shape == xo.shape == (B, N + 1, 2, P)
    dx = float(np.max(np.abs(x - xo)))
    print(f"lane-backward-check solve_sim rodeo N={N} B={B}: x {dx:.3e} (absolute, bar 1e-07)")
    assert dx < 1e-7
    np.testing.assert_array_equal(x[:, 0], c["x0"])


@pytest.mark.parametrize("N,B", SHAPES)
@pytest.mark.parametrize("name", ["kramer", "rodeo"])
def test_solve_mv_dynamic(N, B, name):
    c = _case(N, B)
    got = ra.solve_mv_dynamic(None, c["ode"], *_args(c), ITG[name][0], c["prior"], theta=c["theta"])
    ref = dyo.solve_mv_dynamic(c["oracle_ode"], *_args(c), ITG[name][1], c["prior"], theta=c["theta"])
    assert got.mean.shape == (B, N + 1, 2, P) and got.scale.shape == (B, N, 2)
    _check(got, ref, _bar(P), f"lane-backward fhn {name} p={P} N={N} B={B}")
    np.testing.assert_array_equal(got.mean[:, 0], c["x0"])


@pytest.mark.parametrize("N,B", SHAPES)
def test_solve_sim_dynamic(N, B):
    c = _case(N, B)
    got = ra.solve_sim_dynamic(KEY, c["ode"], *_args(c), ITG["rodeo"][0], c["prior"], theta=c["theta"])
    x, scale, ld = dyo.solve_sim_dynamic(KEY, c["oracle_ode"], *_args(c), ITG["rodeo"][1], c["prior"], theta=c["theta"])
    assert got.x.shape == x.shape == (B, N + 1, 2, P) and got.scale.shape == (B, N, 2)
    dx = float(np.max(np.abs(got.x - x)))
    ds = float(np.max(np.abs(np.sqrt(got.scale) - np.sqrt(scale)) / np.max(np.sqrt(scale), axis=-2, keepdims=True)))
    dl = float(np.max(np.abs(got.logdens - ld) / np.maximum(1.0, np.abs(ld))))
    print(f"lane-backward-check solve_sim_dynamic rodeo N={N} B={B}: x {dx:.3e} (absolute, bar 1e-07), sqrt(scale) {ds:.3e}, "
          f"logdens {dl:.3e} (bar 1e-07)")
    assert dx < 1e-7 and ds <= 1e-7 and dl <= 1e-7
    np.testing.assert_array_equal(got.x[:, 0], c["x0"])


@pytest.mark.parametrize("N,B", SHAPES)
def test_draw_s_is_solve_sim_under_key_plus_s(N, B, monkeypatch):
    """Five draws: one lane per draw, two chunks of two and a half-empty third, a full chunk of four and one draw of a second."""
    c = _case(N, B)
    want = np.stack([_sim(c, KEY + s) for s in range(5)], axis=1)
    for chunk in ("1", "2", "4"):
        monkeypatch.setenv("RK_SIM_DRAWS_CHUNK", chunk)
        x = ra.solve_sim_draws(KEY, c["ode"], *_args(c), ITG["rodeo"][0], c["prior"], n_draws=5, theta=c["theta"])
        assert x.shape == (B, 5, N + 1, 2, P)
        print(f"lane-backward-check solve_sim_draws N={N} B={B} chunk {chunk}: largest difference from solve_sim(key + s) "
              f"{float(np.max(np.abs(x - want))):.3e} (an equality of bits)")
        np.testing.assert_array_equal(x, want)
        np.testing.assert_array_equal(x[:, :, 0], np.broadcast_to(c["x0"][:, None], x[:, :, 0].shape))


def test_the_shapes_above_run_the_lane_kernels():
    """batch_minor=True puts solve_mv / solve_sim at n_bstate 3 on the lanes (their default route is the tiles)."""
    c = _case(3, 65)
    mv = lambda: ra.solve_mv(None, c["ode"], *_args(c), ITG["kramer"][0], c["prior"], batch_minor=True, theta=c["theta"])
    assert _kernels(mv) == ["fwd_kernel", "bwd_mv_kernel"]
    assert _kernels(lambda: _sim(c, KEY)) == ["fwd_kernel", "bwd_sim_kernel"]
