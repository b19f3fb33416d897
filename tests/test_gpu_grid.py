"""
``rodeo_amd.solve_mv_grid`` / ``solve_sim_grid`` on the device against the NumPy restatement tests/grid_oracle.py, and against
``SolvePlan.mv()`` / ``sim()`` of the batch-minor lane route where the grid is uniform and the two are the same solver.

Cases: tests/grid_cases.py (FitzHugh-Nagumo at N = 40 on a three-level, a 40-distinct-step and a uniform grid, n_bstate 2 .. 6
under rodeo and 3, 4 under kramer, schober at t_max = 2, chkrebtii with an integer key; B absent, 1, 3 and 65 -- a second wave,
which in the backward kernels straddles two blocks and in the forward kernel's LDS route (n_bstate 5) leaves one live lane among
63 helpers -- a batched sigma at 65; N = 1, 2, 3; Lorenz63 with three blocks; x'' = sin 2t - x, which reads the table's times; a
traced Python right-hand side).  n_bstate <= 4 holds two pair sets in registers, 5 and 6 (Lorenz63: 4) stage them in LDS.

Bars: tests/test_gpu_solver.py's -- |mean - restatement| <= 1e-9 absolute (Lorenz63: 1e-6), var within 1e-9 of max|var| -- and
for sample paths tests/test_gpu_draws.py's ``_bar(p)`` of max|x|.  tests/test_oracle_grid.py (d) checks on the CPU that the
restatement's own move under R (1 + 1e-15) stays below these for every case but the named ones, ``Case.yardstick``: n_bstate 6
(FitzHugh-Nagumo on [0, 1], three grids, and higher_order), where the mean's highest derivatives are of order 1e5 and the
restatement moves by 3e-8 .. 9e-6; those are held to 20 x that move (the perturbation yardstick of DESIGN.md section 2).
Every comparison prints its largest difference ("grid-check ..." lines: profiles/grid_checks.txt keeps them).
"""
import numpy as np
import pytest
import rodeo_amd as ra
import grid_cases as gc

pytestmark = pytest.mark.gpu


def _kernels(call):
    """Names of the kernels that `call` launched (the handle's per-launch profile)."""
    dev = ra.default_device()
    dev.profile_enable(True)
    try:
        call()
        return [name for name, _ in dev.profile_last()]
    finally:
        dev.profile_enable(False)


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


def _mv(c, ode=None):
    return ra.solve_mv_grid(c["key"], *c.device_args(ode), **c["params"])


def _sim(c, key, ode=None):
    return ra.solve_sim_grid(key, *c.device_args(ode), **c["params"])


_refs = {}


def _oracle(c):
    """The restatement of a case and its own move under the perturbation, computed once and left unchanged."""
    if id(c) not in _refs:
        _refs[id(c)] = gc.mv_moves(c)
    return _refs[id(c)]


def _check_mv(got, c, label=None):
    (mean, var), move_m, move_v = _oracle(c)
    m, v = got
    N1 = len(c["t"])
    lead = () if c["B"] is None else (c["B"],)
    assert m.shape == mean.shape == lead + (N1,) + c["W"].shape[-3::2] and v.shape == var.shape
    bar_m, bar_v = gc.mv_bars(c)
    if c.yardstick:
        bar_m, bar_v = max(bar_m, 20.0 * move_m), max(bar_v, 20.0 * move_v)
    dm, dv = float(np.max(np.abs(m - mean))), float(np.max(np.abs(v - var)) / np.max(np.abs(var)))
    print(f"grid-check {label or c['label']}: mean {dm:.3e} (absolute, bar {bar_m:.1e}), var {dv:.3e} of max|var| (bar {bar_v:.1e})"
          f"{' [yardstick: 20 x the restatement move]' if c.yardstick else ''}")
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(v))
    assert dm <= bar_m and dv <= bar_v, (c["label"], dm, dv)
    np.testing.assert_array_equal(m[..., 0, :, :], c["x0"])             # node 0 is (ode_init, 0)
    assert np.all(v[..., 0, :, :, :] == 0)


# ---- parity with the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", gc.mv_cases(), ids=lambda c: c["label"])
def test_solve_mv_grid_parity(c):
    _check_mv(_mv(c), c)


@pytest.mark.parametrize("p", [3, 4])
def test_traced_python_right_hand_side(p):
    """The README's plain-Python ode_fun: the hiprtc build of the forward kernel."""
    c = gc.fhn(p, "kramer", "distinct", B=3)
    _check_mv(_mv(c, ode=_fitz), c, f"traced {c['label']}")


@pytest.mark.parametrize("c,key", gc.sim_cases(), ids=lambda v: v["label"] if isinstance(v, dict) else str(v))
def test_solve_sim_grid_parity(c, key):
    """Same Philox stream on both sides; another key gives another path after node 0; x[0] is ode_init."""
    x = _sim(c, key)
    ref = c.restate_sim(key)
    assert x.shape == ref.shape
    bar = gc.sim_bar(c["p"])
    dx = float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))
    print(f"grid-check sim {c['label']} key={key}: x {dx:.3e} of max|x| (bar {bar:.0e})")
    assert np.all(np.isfinite(x)) and dx <= bar, (c["label"], dx)
    np.testing.assert_array_equal(x[..., 0, :, :], c["x0"])
    other = _sim(c, key + 1)
    np.testing.assert_array_equal(other[..., 0, :, :], c["x0"])
    assert np.all(np.max(np.abs(other[..., 1:, :, :] - x[..., 1:, :, :]), axis=(-1, -2)) > 0)     # every node after 0


# ---- a uniform grid is the solver -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,itg,B", [(2, "kramer", 3), (3, "kramer", 65), (3, "rodeo", None), (4, "rodeo", 3), (5, "kramer", 65),
                                     (6, "rodeo", 3), (3, "chkrebtii", 3)])
def test_uniform_grid_against_the_lane_route(p, itg, B):
    """``plan.mv()`` / ``plan.sim(key)`` of a batch-minor plan: fwd_kernel + bwd_mv_kernel / bwd_sim_kernel with one (Q, R).  Within
    1e-12 of max|.|, and on one MI355X the bits were equal in all seven cases (the printed line records it), so equality is
    asserted: the step is fwd_kernel's, term for term, and FitzHugh-Nagumo does not read the time, where ``np.linspace`` and
    step_time's t_min + (t_max - t_min) (n + 1) / N may differ in a last bit."""
    c = gc.fhn(p, itg, "uniform", t_max=gc.T_MAX[p], B=B, key=11 if itg == "chkrebtii" else None)
    t = c["t"]
    N = len(t) - 1
    calls = []

    def prior_at(h):
        calls.append(h)
        return ra.ibm_init(h, p, c["sigma"])
    args = (c["ode"], c["W"], c["x0"])
    m, v = ra.solve_mv_grid(c["key"], *args, t, gc.ITG[itg][0], prior_at, **c["params"])
    x = ra.solve_sim_grid(5, *args, t, gc.ITG[itg][0], prior_at, **c["params"])
    assert len(calls) == 2                                              # once per call: one slot
    plan = ra.SolvePlan(*args, t[0], t[-1], N, gc.ITG[itg][0], ra.ibm_init(calls[0], p, c["sigma"]), batch_minor=True, **c["params"])
    assert _kernels(lambda: plan.mv(c["key"])) == ["fwd_kernel", "bwd_mv_kernel"]
    mo, vo = plan.state_host()
    plan.sim(5)
    xo = plan.x_host()
    dm = float(np.max(np.abs(m - mo)) / np.max(np.abs(mo)))
    dv = float(np.max(np.abs(v - vo)) / np.max(np.abs(vo)))
    dx = float(np.max(np.abs(x - xo)) / np.max(np.abs(xo)))
    bits = np.array_equal(m, mo) and np.array_equal(v, vo) and np.array_equal(x, xo)
    print(f"grid-check uniform {itg} p={p} B={B} against plan.mv() / plan.sim(): mean {dm:.3e} var {dv:.3e} x {dx:.3e} of max|.| "
          f"(bar 1e-12); bits equal: {bits}")
    assert max(dm, dv, dx) <= 1e-12
    assert bits


# ---- launch and determinism ----------------------------------------------------------------------------------------------
def test_the_launched_kernels():
    c, c5, lz = gc.fhn(3, "kramer", "distinct", B=3), gc.fhn(5, "rodeo", "levels", B=3), gc.lorenz(3, "kramer", "distinct", B=5)
    assert _kernels(lambda: _mv(c)) == ["grid_fwd_kernel", "grid_bwd_mv_kernel"]
    assert _kernels(lambda: _mv(c5)) == ["grid_fwd_kernel", "grid_bwd_mv_kernel"]
    assert _kernels(lambda: _mv(lz)) == ["grid_fwd_kernel", "grid_bwd_mv_kernel"]
    assert _kernels(lambda: _mv(c, ode=_fitz)) == ["grid_fwd_kernel<user>", "grid_bwd_mv_kernel"]
    assert _kernels(lambda: _sim(c, 1)) == ["grid_fwd_kernel", "grid_bwd_sim_kernel"]
    assert _kernels(lambda: _sim(c, 1, ode=_fitz)) == ["grid_fwd_kernel<user>", "grid_bwd_sim_kernel"]


@pytest.mark.parametrize("c", [gc.fhn(3, "kramer", "distinct", B=65), gc.fhn(5, "rodeo", "levels", B=65, batched_sigma=True),
                               gc.fhn(5, "rodeo", "levels", B=65), gc.lorenz(3, "kramer", "distinct", B=5)], ids=lambda c: c["label"])
def test_two_calls_give_identical_bytes(c):
    first, again = _mv(c), _mv(c)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    assert _sim(c, 5).tobytes() == _sim(c, 5).tobytes()


def test_prior_at_is_called_once_per_slot():
    c = gc.fhn(3, "kramer", "levels", B=3)
    calls = []

    def prior_at(h):
        calls.append(h)
        return ra.ibm_init(h, 3, c["sigma"])
    ra.solve_mv_grid(None, c["ode"], c["W"], c["x0"], c["t"], gc.ITG["kramer"][0], prior_at, **c["params"])
    assert len(calls) == 3 == len(ra.grid_slots(c["t"])[0])
