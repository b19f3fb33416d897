"""
``rodeo_amd.solve_mv_dynamic`` / ``solve_sim_dynamic`` on the device against the NumPy restatement tests/dynamic_oracle.py, and
against ``solve_mv`` itself where a floor above every estimate makes the two the same solver.

Bars (``test_gpu_evidence._bar``): 1e-7 for n_bstate <= 4, 1e-5 at 5 -- mean within bar max|mean|, var within bar max|var|,
logdens within bar max(1, |ref|), and the scales as |sqrt(c_dev) - sqrt(c_ref)| <= bar max_n sqrt(c_ref) per block, the
normalised innovation in absolute terms (what rounding governs, so no entry is excluded).  The restatement's own movement under
the rounding-level perturbation sigma x 3 (tests/test_oracle_dynamic.py (c)) is 1.5e-10 at n_bstate 4 (670 times below its bar),
2e-12 at 5 and below 1e-12 otherwise (1e5 times and more).  Every comparison prints its largest difference ("dynamic-check ..."
lines: profiles/dynamic_checks.txt keeps them).
"""
import numpy as np
import pytest
import rodeo_amd as ra
import dynamic_oracle as dyo
from test_gpu_evidence import ITG, _bar, _fhn, _lorenz, _fitz, _kernels

pytestmark = pytest.mark.gpu

FLOOR = {"kramer": 2.0 ** 14, "schober": 2.0 ** 14, "rodeo": 2.0 ** 20}      # tests/test_oracle_dynamic.py (d), n_bstate 3, N 40, t_max 1


def _device(c, name, ode=None, prior=None, **kw):
    return ra.solve_mv_dynamic(None, ode or c["ode"], c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[name][0], prior or c["prior"],
                               theta=c["theta"], **kw)


_refs = {}


def _oracle(c, name):
    """The restatement of a case, computed once and left unchanged (the cases are cached objects)."""
    key = (id(c), name)
    if key not in _refs:
        _refs[key] = dyo.solve_mv_dynamic(c["oracle_ode"], c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[name][1], c["prior"],
                                          theta=c["theta"])
    return _refs[key]


def _check(got, ref, bar, label):
    mean, var, scale, ld = ref
    assert got.mean.shape == mean.shape and got.var.shape == var.shape and got.scale.shape == scale.shape
    assert np.shape(got.logdens) == np.shape(ld)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var)) and np.all(np.isfinite(scale))
    dm = float(np.max(np.abs(got.mean - mean)) / np.max(np.abs(mean)))
    dv = float(np.max(np.abs(got.var - var)) / np.max(np.abs(var)))
    root, root_ref = np.sqrt(got.scale), np.sqrt(scale)
    ds = float(np.max(np.abs(root - root_ref) / np.max(root_ref, axis=-2, keepdims=True)))      # per block (and trajectory)
    dl = float(np.max(np.abs(np.asarray(got.logdens) - ld) / np.maximum(1.0, np.abs(ld))))
    print(f"dynamic-check {label}: mean {dm:.3e} var {dv:.3e} of the largest entry, sqrt(scale) {ds:.3e} of the block's largest, "
          f"logdens {dl:.3e} of max(1, |ref|), bar {bar:.0e}")
    assert max(dm, dv, ds, dl) <= bar, (label, dm, dv, ds, dl)


# ---- parity with the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,name,N,t_max", [(2, "kramer", 40, 1.0), (3, "kramer", 40, 1.0), (3, "rodeo", 40, 1.0),
                                            (3, "schober", 40, 1.0), (4, "kramer", 40, 1.0), (5, "rodeo", 40, 1.0),
                                            (3, "kramer", 72, 4.0)])
def test_parity_fitzhugh(p, name, N, t_max):
    """Unbatched (a float logdens), a part of a wave, and a ragged second wave with a batched sigma."""
    one = _fhn(p, N, t_max)
    got = _device(one, name)
    assert isinstance(got.logdens, float) and got.mean.shape == (N + 1, 2, p) and got.scale.shape == (N, 2)
    _check(got, _oracle(one, name), _bar(p), f"fhn {name} p={p} N={N} unbatched")
    for B, bs in ((3, False), (70, True)):
        c = _fhn(p, N, t_max, B, bs)
        got = _device(c, name)
        assert got.logdens.shape == (B,) and got.scale.shape == (B, N, 2) and got.var.shape == (B, N + 1, 2, p, p)
        _check(got, _oracle(c, name), _bar(p), f"fhn {name} p={p} N={N} B={B}")


@pytest.mark.parametrize("N", [1, 2])
def test_parity_short_horizons(N):
    c = _fhn(3, N, 0.025 * N, 3)
    _check(_device(c, "kramer"), _oracle(c, "kramer"), _bar(3), f"fhn kramer p=3 N={N} B=3")


@pytest.mark.parametrize("name", ["rodeo", "kramer"])
def test_parity_lorenz_three_blocks(name):
    """d = 3 at N = 60, t_max = 1.2 (``test_gpu_evidence._lorenz``'s grid, not shortened: the restatement is finite there and
    moves by 4e-14 of the largest entry under sigma x 3, far below bar / 1000 = 1e-10)."""
    one = _lorenz(3)
    _check(_device(one, name), _oracle(one, name), _bar(3), f"lorenz {name} p=3 unbatched")
    c = _lorenz(3, 5)
    got = _device(c, name)
    assert got.scale.shape == (5, 60, 3)
    _check(got, _oracle(c, name), _bar(3), f"lorenz {name} p=3 B=5")


@pytest.mark.parametrize("p", [3, 4])
def test_traced_python_right_hand_side(p):
    """The README's plain-Python ode_fun: the hiprtc build of the forward kernel."""
    c = _fhn(p, 40, 1.0, 3)
    _check(_device(c, "kramer", ode=_fitz), _oracle(c, "kramer"), _bar(p), f"traced fhn kramer p={p} B=3")


# ---- the two properties, on the device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("p,name", [(3, "kramer"), (3, "rodeo"), (4, "kramer")])
def test_scale_invariance_on_the_device(p, name):
    c = _fhn(p, 40, 1.0, 3)
    Q, R = c["prior"]
    one, nine = _device(c, name), _device(c, name, prior=(Q, 9.0 * R))       # sigma x 3
    dm = float(np.max(np.abs(nine.mean - one.mean)) / np.max(np.abs(one.mean)))
    dv = float(np.max(np.abs(nine.var - one.var)) / np.max(np.abs(one.var)))
    ds = float(np.max(np.abs(nine.scale / one.scale * 9.0 - 1.0)))
    print(f"dynamic-check invariance {name} p={p}: mean {dm:.3e} var {dv:.3e} of the largest entry (bar 1e-09), scale ratio off by "
          f"{ds:.3e} (bar 1e-05)")
    assert dm <= 1e-9 and dv <= 1e-9 and ds <= 1e-5


@pytest.mark.parametrize("name", ["kramer", "schober", "rodeo"])
def test_floor_limit_against_solve_mv(name):
    """With a floor above every estimate every scale is the floor and the result is ``solve_mv``'s under (Q, floor R): the
    existing solver as the yardstick, independent of the restatement."""
    c = _fhn(3, 40, 1.0, 3)
    Q, R = c["prior"]
    floor = FLOOR[name]
    got = _device(c, name, scale_min=floor)
    assert np.all(got.scale == floor)
    mean, var = ra.solve_mv(None, c["ode"], c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[name][0], (Q, floor * R), theta=c["theta"])
    dm = float(np.max(np.abs(got.mean - mean)) / np.max(np.abs(mean)))
    dv = float(np.max(np.abs(got.var - var)) / np.max(np.abs(var)))
    print(f"dynamic-check floor 2^{int(np.log2(floor))} {name} against solve_mv: mean {dm:.3e} var {dv:.3e} of the largest entry, "
          "bar 1e-09")
    assert dm <= 1e-9 and dv <= 1e-9
    ev = ra.solve_evidence(None, c["ode"], c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[name][0], (Q, floor * R), theta=c["theta"])
    assert np.max(np.abs(got.logdens - ev.logdens) / np.abs(ev.logdens)) <= 1e-9


# ---- solve_sim_dynamic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,name", [(3, "rodeo"), (2, "kramer")])
def test_solve_sim_dynamic_parity(p, name):
    """Same Philox stream on both sides: the sample paths agree to the bar of tests/test_gpu_solver.py's test_solve_sim_parity
    (1e-7, absolute), another key gives another path after node 0, x[0] is ode_init.

    The cases are those where that bar can tell a fault from rounding: under the rounding-level perturbation sigma x 3 the
    restatement's own path moves by 6e-9 (rodeo, n_bstate 3) and 9e-9 (kramer, n_bstate 2).  Under kramer and schober at
    n_bstate 3 it moves by 2.8e-7 and 5.3e-7 itself -- their filtered variances are singular and the draw's factor turns a
    rounding-level pivot of a variance of order 1e2 into its square root -- so no comparison at 1e-7 is possible there (the
    device differed from the restatement by 6.1e-7 under kramer); dynamic_bwd_sim_kernel does not depend on the interrogation."""
    c = _fhn(p, 40, 1.0, 9)
    args = (c["W"], c["x0"], 0.0, c["t_max"], c["N"])
    got = ra.solve_sim_dynamic(42, c["ode"], *args, ITG[name][0], c["prior"], theta=c["theta"])
    x, scale, ld = dyo.solve_sim_dynamic(42, c["oracle_ode"], *args, ITG[name][1], c["prior"], theta=c["theta"])
    assert got.x.shape == (9, 41, 2, p) and got.scale.shape == (9, 40, 2) and got.logdens.shape == (9,)
    np.testing.assert_array_equal(got.x[:, 0], c["x0"])
    dx = float(np.max(np.abs(got.x - x)))
    ds = float(np.max(np.abs(np.sqrt(got.scale) - np.sqrt(scale)) / np.max(np.sqrt(scale), axis=-2, keepdims=True)))
    dl = float(np.max(np.abs(got.logdens - ld) / np.maximum(1.0, np.abs(ld))))
    print(f"dynamic-check sim {name} p={p} B=9: x {dx:.3e} (absolute, bar 1e-07), sqrt(scale) {ds:.3e}, logdens {dl:.3e} (bar 1e-07)")
    assert dx < 1e-7 and ds <= 1e-7 and dl <= 1e-7
    other = ra.solve_sim_dynamic(43, c["ode"], *args, ITG[name][0], c["prior"], theta=c["theta"])
    np.testing.assert_array_equal(other.x[:, 0], c["x0"])
    assert np.all(np.max(np.abs(other.x[:, 1:] - got.x[:, 1:]), axis=(2, 3)) > 0)            # every node after 0, every trajectory
    np.testing.assert_array_equal(other.scale, got.scale)                                    # (the filter draws nothing)


# ---- launch and determinism ----------------------------------------------------------------------------------------------
def test_the_launched_kernels():
    c = _fhn(3, 40, 1.0, 3)
    assert _kernels(lambda: _device(c, "kramer")) == ["dynamic_fwd_kernel", "dynamic_bwd_mv_kernel"]
    assert _kernels(lambda: _device(c, "kramer", ode=_fitz)) == ["dynamic_fwd_kernel<user>", "dynamic_bwd_mv_kernel"]
    assert _kernels(lambda: _device(_lorenz(3, 5), "rodeo")) == ["dynamic_fwd_kernel", "dynamic_bwd_mv_kernel"]
    sim = lambda: ra.solve_sim_dynamic(1, c["ode"], c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG["kramer"][0], c["prior"],
                                       theta=c["theta"])
    assert _kernels(sim) == ["dynamic_fwd_kernel", "dynamic_bwd_sim_kernel"]


@pytest.mark.parametrize("case", ["fhn B=70", "lorenz d=3"])
def test_two_calls_give_identical_bits(case):
    c, name = (_fhn(3, 40, 1.0, 70, True), "kramer") if case == "fhn B=70" else (_lorenz(3, 5), "rodeo")
    first, again = _device(c, name), _device(c, name)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    args = (c["ode"], c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[name][0], c["prior"])
    s1, s2 = (ra.solve_sim_dynamic(5, *args, theta=c["theta"]) for _ in range(2))
    for a, b in zip(s1, s2):
        np.testing.assert_array_equal(a, b)
