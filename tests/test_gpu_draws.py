"""
``rodeo_amd.solve_sim_draws`` on the device.  The yardstick is the existing solver: draw s against the lane route's
``plan.sim(key + s)`` on the same batch-minor plan (every s) and draw 0 against the default route's ``solve_sim(key)`` (the
tiles at n_bstate 3), with the draws per lane fixed at the full chunk (``RK_SIM_DRAWS_CHUNK``) so that full and ragged chunks
run, and 1, 2, 4 and the launch's own choice against one another; then ``keep`` against the rows of the full result (bit for bit), the NumPy restatement
tests/draws_oracle.py, a traced Python right-hand side, determinism and the seed law seen from outside, and the statistical
pin of tests/test_oracle_draws.py on the device's own 2048 draws.  Bars are ``test_gpu_evidence._bar(p)`` of max|x|: 1e-7 for
n_bstate <= 4, 1e-5 at 5 and 6.  Every comparison prints its largest difference ("draws-check ..." lines:
profiles/sim_draws_checks.txt keeps them).
"""
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd import draws
from rodeo_amd.solve import cached_plan
from oracle import interrogations as oi
from test_gpu_evidence import ITG, _bar, _fhn, _fitz, _lorenz
import draws_oracle as dro

pytestmark = pytest.mark.gpu

KEY = 11


def _draws(c, name, key=KEY, n_draws=1, keep=None, ode=None):
    return ra.solve_sim_draws(key, ode or c["ode"], c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[name][0], c["prior"],
                              n_draws=n_draws, keep=keep, theta=c["theta"])


def _lane_paths(c, name, key, n):
    """The yardstick: plan.sim(key + s) on the batch-minor plan (bwd_sim_kernel on the lanes), s = 0 .. n - 1, draws axis -4."""
    plan = cached_plan(c["ode"], c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[name][0], c["prior"], "standard", batch_minor=True,
                       theta=c["theta"])
    out = []
    for s in range(n):
        plan.sim(key + s)
        out.append(np.array(plan.x_host()))
    return np.stack(out, axis=-4)


def _close(got, want, p, label):
    assert got.shape == want.shape, (label, got.shape, want.shape)
    scale = float(np.max(np.abs(want)))
    worst = float(np.max(np.abs(got - want))) / scale
    print(f"draws-check {label}: largest difference {worst:.3e} of max|x|, bar {_bar(p):.0e}")
    assert worst <= _bar(p), (label, worst)
    return worst


# ---- 1. against the existing solver ---------------------------------------------------------------------------------------
def _ways(make):
    """unbatched; B = 3, part of a wave; B = 70 with a batched sigma, a ragged second wave"""
    return [("unbatched", make()), ("B=3", make(3)), ("B=70", make(70, True))]


CASES = [("fhn", 2, "kramer"), ("fhn", 3, "kramer"), ("fhn", 3, "rodeo"), ("fhn", 3, "schober"), ("fhn", 4, "kramer"),
         ("fhn", 6, "rodeo"), ("lorenz", 3, "kramer")]


@pytest.mark.parametrize("problem,p,name", CASES)
def test_draw_s_is_solve_sim_under_seed_plus_s(problem, p, name, monkeypatch):
    C = draws.chunk()
    monkeypatch.setenv("RK_SIM_DRAWS_CHUNK", str(C))      # (these small batches would run one draw per lane: fix the full chunk)
    if problem == "fhn":
        ways = _ways(lambda *b: _fhn(p, 40, 1.0, *b))
    else:
        ways = [("unbatched", _lorenz(p)), ("B=5", _lorenz(p, 5))]               # _lorenz's grid: N = 60, t_max = 1.2
    bits = True
    for way, c in ways:
        B, d, N = (c["x0"].shape[0],) if c["x0"].ndim == 3 else (), c["W"].shape[-3], c["N"]
        want = _lane_paths(c, name, KEY, 2 * C + 1)
        for n_draws in (1, C, C + 1, 2 * C + 1):                              # one chunk, a full one, a ragged second and third
            x = _draws(c, name, KEY, n_draws)
            assert x.shape == B + (n_draws, N + 1, d, p)
            ref = want[..., :n_draws, :, :, :]
            _close(x, ref, p, f"{problem} p={p} {name} {way} n_draws={n_draws} against the lane route")
            bits = bits and np.array_equal(x, ref)
            np.testing.assert_array_equal(x[..., 0, :, :], np.broadcast_to(c["x0"][..., None, :, :], x[..., 0, :, :].shape))
        default = ra.solve_sim(KEY, c["ode"], c["W"], c["x0"], 0.0, c["t_max"], N, ITG[name][0], c["prior"], theta=c["theta"])
        _close(x[..., 0, :, :, :], default, p, f"{problem} p={p} {name} {way} draw 0 against the default route")
    print(f"draws-check {problem} p={p} {name}: bit-identical to the lane route: {bits}")


@pytest.mark.parametrize("p", [3, 6])
def test_the_draws_do_not_depend_on_the_chunk(p, monkeypatch):
    """One, two or four draws per lane, or the launch's own choice: the same bytes, and those of the lane route."""
    C = draws.chunk()
    c = _fhn(p, 40, 1.0, 70, True)
    want = _lane_paths(c, "rodeo", KEY, 2 * C + 1)
    for chunk in ("1", "2", str(C), None):
        if chunk is None:
            monkeypatch.delenv("RK_SIM_DRAWS_CHUNK")
        else:
            monkeypatch.setenv("RK_SIM_DRAWS_CHUNK", chunk)
        x = _draws(c, "rodeo", KEY, 2 * C + 1, keep=[0, 1, 17, 40])
        _close(x, want[:, :, [0, 1, 17, 40]], p, f"chunk {chunk or 'chosen by the launch'} p={p} B=70 against the lane route")
        if chunk == "1":
            first = x
        np.testing.assert_array_equal(x, first)


def test_the_launches_are_the_filter_and_the_draws_kernel():
    dev = ra.default_device()
    dev.profile_enable(True)
    try:
        _draws(_fhn(3, 40, 1.0, 3), "kramer", n_draws=5)
        names = [name for name, _ in dev.profile_last()]
        _draws(_fhn(3, 40, 1.0, 3), "kramer", n_draws=5, ode=_fitz)
        traced = [name for name, _ in dev.profile_last()]
    finally:
        dev.profile_enable(False)
    assert names == ["fwd_kernel", "bwd_sim_draws_kernel"], names
    assert len(traced) == 2 and traced[0].startswith("fwd_kernel") and traced[1] == "bwd_sim_draws_kernel", traced


# ---- 2. keep ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B", [(40, 70), (1, 3), (2, 3)])
def test_keep_gives_the_rows_of_the_full_result(N, B, monkeypatch):
    C = draws.chunk()
    monkeypatch.setenv("RK_SIM_DRAWS_CHUNK", str(C))                          # C + 1 draws: a full and a ragged chunk
    c = _fhn(3, N, 0.025 * N, B, B == 70)
    full = _draws(c, "kramer", n_draws=C + 1)
    assert full.shape == (B, C + 1, N + 1, 2, 3)
    _close(full, _lane_paths(c, "kramer", KEY, C + 1), 3, f"keep: full result N={N} B={B} against the lane route")
    keeps = [[0], [N], [0, N], [1], list(range(N + 1))] + ([[N // 4, N // 2, 3 * N // 4]] if N >= 4 else [])
    for keep in keeps:
        x = _draws(c, "kramer", n_draws=C + 1, keep=np.array(keep))
        assert x.shape == (B, C + 1, len(keep), 2, 3)
        np.testing.assert_array_equal(x, full[:, :, keep])
    print(f"draws-check keep N={N} B={B}: {len(keeps)} index sets equal the rows of keep=None bit for bit")


# ---- 3. the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,keep", [(3, None), (4, [0, 7, 39, 40])])
def test_against_the_oracle(p, keep):
    c = _fhn(p, 40, 1.0, 3)
    x = _draws(c, "kramer", n_draws=5, keep=keep)
    want = dro.solve_sim_draws(KEY, c["oracle_ode"], c["W"], c["x0"], 0.0, c["t_max"], c["N"], oi.interrogate_kramer, c["prior"],
                               n_draws=5, keep=keep, theta=c["theta"])
    _close(x, want, p, f"oracle fhn kramer p={p} B=3 n_draws=5 keep={'all' if keep is None else keep}")


# ---- 4. a traced Python right-hand side -------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [3, 4])
def test_traced_python_right_hand_side(p):
    c = _fhn(p, 40, 1.0, 3)
    built_in = _draws(c, "kramer", n_draws=5, keep=[0, 20, 40])
    traced = _draws(c, "kramer", n_draws=5, keep=[0, 20, 40], ode=_fitz)
    _close(traced, built_in, p, f"traced fhn kramer p={p} B=3 against the built-in right-hand side")


# ---- 5. determinism and the seed law from outside ---------------------------------------------------------------------------
def test_same_key_same_bytes_and_next_key_shifts_the_draws():
    C = draws.chunk()
    c = _fhn(3, 40, 1.0, 70, True)
    n = 2 * C + 1
    a, again, b = _draws(c, "rodeo", 5, n), _draws(c, "rodeo", 5, n), _draws(c, "rodeo", 6, n)
    assert a.tobytes() == again.tobytes()
    worst = _close(a[:, 1:], b[:, :-1], 3, "seed law: draws 1.. of key 5 against draws ..-1 of key 6")
    print(f"draws-check seed law: bit-identical across chunk positions: {worst == 0.0}")
    assert not np.array_equal(a[:, 0], a[:, 1])                               # another seed, another path


# ---- 6. statistics ----------------------------------------------------------------------------------------------------------
def test_the_statistical_pin_on_the_device_output():
    c = dro.pin_problem(ra)
    x = ra.solve_sim_draws(dro.PIN_KEY, ra.ode.fitzhugh_nagumo, c["W"], c["x0"], 0.0, dro.PIN_T_MAX, dro.PIN_N,
                           ITG["kramer"][0], c["prior"], n_draws=dro.PIN_DRAWS, theta=c["theta"])
    assert x.shape == (dro.PIN_DRAWS, dro.PIN_N + 1, 2, dro.PIN_P)
    mean, var = dro.pin_posterior(c)
    zmax, rmin, rmax = dro.pin_statistics(x, mean, var)
    zbar, lo, hi = dro.pin_bounds()
    print(f"draws-check device pin: largest z-score {zmax:.2f} (bar {zbar:.0f}), variance ratios {rmin:.3f} .. {rmax:.3f} "
          f"(allowed {lo:.3f} .. {hi:.3f})")
    assert zmax <= zbar and lo <= rmin and rmax <= hi
