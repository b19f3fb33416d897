"""
``rodeo_amd.solve_sim_draws_grid`` and ``rodeo_amd.inference.dalton.solve_sim_draws_grid`` on the device.  The yardstick is the
existing device sampler: draw s against ``solve_sim_grid(key + s)`` (DALTON: ``dalton.solve_sim_grid(key + s)``) for every s, with
the draws per lane fixed at the full chunk (``RK_SIM_DRAWS_CHUNK``) so that one chunk, a full one and a ragged second and third
run; then short grids (N = 1, 2, 3), ``keep`` against the rows of the full result (bit for bit), 1, 2, 4 draws per lane and the
launch's own choice against one another, a uniform grid against ``solve_sim_draws`` (DALTON: per-draw ``dalton.solve_sim`` on the
lanes), the NumPy restatement tests/draws_grid_oracle.py on the cases that tests/test_oracle_draws_grid.py (c) vetted, a traced
Python right-hand side, determinism, the seed law seen from outside and the launched kernels, and the two statistical pins of
tests/test_oracle_draws_grid.py on the device's own 2048 draws.

Bars are ``grid_cases.sim_bar(p)`` of max|x|: 1e-7 for n_bstate <= 4, 1e-5 at 5 and 6.  Every comparison prints its largest
difference and whether the bits are equal ("grid-draws-check ..." lines: profiles/grid_draws_checks.txt keeps them).  On one
MI355X every comparison with the device samplers and with ``solve_sim_draws`` found identical bits (all 291 lines), so those
comparisons assert equality behind the bar.
"""
import functools
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401
from rodeo_amd import draws
import grid_cases as gc
import dalton_grid_cases as dc
import draws_oracle as dro
import draws_grid_oracle as dgr
from test_oracle_draws_grid import N_DRAWS, TRACED_KEY, restated_cases, traced_cases

pytestmark = pytest.mark.gpu
dmod = sys.modules["rodeo_amd.inference.dalton"]         # (rodeo_amd.inference.dalton, the attribute, is the function)

KEY = 11


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


def _draws(c, key=KEY, n_draws=1, keep=None, ode=None):
    """The function under test for a grid_cases.Case (p(X | Z)) or a dalton_grid_cases.DCase (p(X | Z, Y))."""
    if isinstance(c, dc.DCase):
        return c.device_call(functools.partial(dmod.solve_sim_draws_grid, n_draws=n_draws, keep=keep), key, ode)
    return ra.solve_sim_draws_grid(key, *c.device_args(ode), n_draws=n_draws, keep=keep, **c["params"])


def _sampler_paths(c, key, n):
    """The yardstick: the existing device sampler under the seeds key .. key + n - 1, draws on axis -4."""
    if isinstance(c, dc.DCase):
        return np.stack([np.array(c.device_call(dmod.solve_sim_grid, key + s)) for s in range(n)], axis=-4)
    return np.stack([np.array(ra.solve_sim_grid(key + s, *c.device_args(), **c["params"])) for s in range(n)], axis=-4)


def _close(got, want, p, label):
    """The bar; returns whether the bits are equal as well.  Where the yardstick itself is not finite (one case: n_bstate 6 on the
    distinct steps at B = 70, whose problem overflows in most trajectories, in the restatement too -- tests/test_oracle_draws_grid.py
    (d)) the non-finite entries must be the same entries, and the finite ones are held to the bar."""
    assert got.shape == want.shape, (label, got.shape, want.shape)
    finite = np.isfinite(want)
    assert finite.any() and np.array_equal(np.isfinite(got), finite), label
    worst = float(np.max(np.abs(got[finite] - want[finite]))) / float(np.max(np.abs(want[finite])))
    bits = np.array_equal(got, want, equal_nan=True)
    gaps = "" if finite.all() else f"; {int((~finite).sum())} of {finite.size} entries are not finite on both sides"
    print(f"grid-draws-check {label}: largest difference {worst:.3e} of max|x|, bar {gc.sim_bar(p):.0e}; bits equal: {bits}{gaps}")
    assert worst <= gc.sim_bar(p), (label, worst)
    return bits


def _node0_is_ode_init(x, c):
    np.testing.assert_array_equal(x[..., 0, :, :], np.broadcast_to(c["x0"][..., None, :, :], x[..., 0, :, :].shape))


def _against_the_sampler(c, label, C):
    """n_draws = 1, C, C + 1, 2 C + 1 against the sampler's paths: the bar, the shapes, node 0, and the bits."""
    lead = () if c["B"] is None else (c["B"],)
    d, p, N = c["W"].shape[-3], c["p"], len(c["t"]) - 1
    want = _sampler_paths(c, KEY, 2 * C + 1)
    for n_draws in (1, C, C + 1, 2 * C + 1):                                  # one chunk, a full one, a ragged second and third
        x = _draws(c, KEY, n_draws)
        assert x.shape == lead + (n_draws, N + 1, d, p)
        ref = want[..., :n_draws, :, :, :]
        _close(x, ref, p, f"{label} n_draws={n_draws} against the device sampler")
        np.testing.assert_array_equal(x, ref)
        _node0_is_ode_init(x, c)


# ---- 1. draw s against the existing device sampler ------------------------------------------------------------------------
def _ways(p, itg, kind, t_max):
    """unbatched; B = 3, part of a wave; B = 70 with a batched sigma: batched pairs and a ragged second wave"""
    return [("unbatched", gc.fhn(p, itg, kind, t_max=t_max)), ("B=3", gc.fhn(p, itg, kind, t_max=t_max, B=3)),
            ("B=70", gc.fhn(p, itg, kind, t_max=t_max, B=70, batched_sigma=True))]


CASES = [(2, "kramer", 4.0), (3, "kramer", 4.0), (4, "kramer", 4.0), (3, "rodeo", 4.0), (3, "schober", 2.0), (5, "rodeo", 4.0),
         (6, "rodeo", 1.0)]


@pytest.mark.parametrize("kind", ["levels", "distinct"])
@pytest.mark.parametrize("p,itg,t_max", CASES)
def test_draw_s_is_solve_sim_grid_under_seed_plus_s(p, itg, t_max, kind, monkeypatch):
    C = draws.chunk()
    monkeypatch.setenv("RK_SIM_DRAWS_CHUNK", str(C))      # (these small batches would run one draw per lane: fix the full chunk)
    for way, c in _ways(p, itg, kind, t_max):
        _against_the_sampler(c, f"fhn p={p} {itg} {kind} {way}", C)


def test_three_blocks(monkeypatch):
    C = draws.chunk()
    monkeypatch.setenv("RK_SIM_DRAWS_CHUNK", str(C))
    _against_the_sampler(gc.lorenz(3, "kramer", "distinct", B=5), "lorenz p=3 kramer distinct B=5", C)


# ---- 2. the same for DALTON -----------------------------------------------------------------------------------------------
DALTON_BASES = [gc.fhn(3, "kramer", "distinct", B=65), gc.fhn(4, "kramer", "distinct", B=3), gc.fhn(5, "rodeo", "levels", B=3)]


@pytest.mark.parametrize("n_bobs", [1, 2])
@pytest.mark.parametrize("nodes", [dc.NODES, (0, 1, 20, 21, 40)], ids=lambda n: "obs@" + ",".join(map(str, n)))
@pytest.mark.parametrize("base", DALTON_BASES, ids=lambda c: c["label"])
def test_dalton_draw_s_is_dalton_solve_sim_grid_under_seed_plus_s(base, nodes, n_bobs, monkeypatch):
    C = draws.chunk()
    monkeypatch.setenv("RK_SIM_DRAWS_CHUNK", str(C))
    c = dc.make(base, nodes, n_bobs)
    _against_the_sampler(c, f"dalton {c['label']}", C)


@pytest.mark.parametrize("base", [gc.fhn(3, "kramer", "distinct", B=65), gc.fhn(5, "rodeo", "levels", B=3)], ids=lambda c: c["label"])
def test_dalton_without_observations_is_the_plain_function(base):
    c = dc.make(base, ())
    plain = gc.Case(c)                                    # (the same problem at the same prior scale, without the data)
    for keep in (None, [0, 7, 40]):
        x, want = _draws(c, KEY, 5, keep), _draws(plain, KEY, 5, keep)
        assert x.tobytes() == want.tobytes()
    assert _kernels(lambda: _draws(c, KEY, 5)) == ["grid_fwd_kernel", "grid_bwd_sim_draws_kernel"]


# ---- 3. short grids: no loop iteration at all (N = 1), the first prefetch only (N = 2), one rotation (N = 3) ------------
@pytest.mark.parametrize("dalton", [False, True], ids=["plain", "dalton"])
@pytest.mark.parametrize("B", [3, 65])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_short_grids(N, B, dalton, monkeypatch):
    C = draws.chunk()
    monkeypatch.setenv("RK_SIM_DRAWS_CHUNK", str(C))
    c = gc.fhn(3, "rodeo", "distinct", N=N, t_max=0.1 * N, B=B)
    if dalton:
        c = dc.make(c, dc.SHORT_NODES[N])
    label = f"{'dalton ' if dalton else ''}short grid N={N} B={B}"
    _against_the_sampler(c, label, C)
    full = _draws(c, KEY, C + 1)
    keeps = [k for k in ([0], [N], [0, N], [1]) if max(k) <= N and len(set(k)) == len(k)]
    for keep in keeps:
        x = _draws(c, KEY, C + 1, keep=keep)
        assert x.shape == (B, C + 1, len(keep), 2, 3)
        np.testing.assert_array_equal(x, full[:, :, keep])
    print(f"grid-draws-check {label}: {len(keeps)} index sets equal the rows of keep=None bit for bit")


# ---- 4. keep ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dalton", [False, True], ids=["plain", "dalton"])
def test_keep_gives_the_rows_of_the_full_result(dalton, monkeypatch):
    C = draws.chunk()
    monkeypatch.setenv("RK_SIM_DRAWS_CHUNK", str(C))                          # C + 1 draws: a full and a ragged chunk
    N, B = 40, 70
    c = gc.fhn(3, "kramer", "distinct", B=B, batched_sigma=True)
    if dalton:
        c = dc.make(c)
    full = _draws(c, KEY, C + 1)
    assert full.shape == (B, C + 1, N + 1, 2, 3)
    _close(full, _sampler_paths(c, KEY, C + 1), 3, f"keep: full result {c['label']} against the device sampler")
    keeps = [[0], [N], [0, N], [1], [N // 4, N // 2, 3 * N // 4], list(dc.NODES), list(range(N + 1))]
    for keep in keeps:
        x = _draws(c, KEY, C + 1, keep=np.array(keep))
        assert x.shape == (B, C + 1, len(keep), 2, 3)
        np.testing.assert_array_equal(x, full[:, :, keep])
    print(f"grid-draws-check keep {'dalton ' if dalton else ''}N={N} B={B}: {len(keeps)} index sets equal the rows of keep=None "
          "bit for bit")


# ---- 5. the draws do not depend on the chunk --------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [3, 6])
def test_the_draws_do_not_depend_on_the_chunk(p, monkeypatch):
    """One, two or four draws per lane, or the launch's own choice: the same bytes, and those of the device sampler.  (6 is the
    largest n_bstate served; no (P, C) instance is capped, and a cap would have to pass here unseen.  On "levels": at 6 the problem
    on the distinct steps is not finite at B = 70.)"""
    C = draws.chunk()
    c = gc.fhn(p, "rodeo", "levels", t_max=gc.T_MAX[p], B=70, batched_sigma=True)
    keep = [0, 1, 17, 40]
    want = _sampler_paths(c, KEY, 2 * C + 1)[:, :, keep]
    for chunk in ("1", "2", str(C), None):
        if chunk is None:
            monkeypatch.delenv("RK_SIM_DRAWS_CHUNK")
        else:
            monkeypatch.setenv("RK_SIM_DRAWS_CHUNK", chunk)
        x = _draws(c, KEY, 2 * C + 1, keep=keep)
        _close(x, want, p, f"chunk {chunk or 'chosen by the launch'} p={p} B=70 against the device sampler")
        if chunk == "1":
            first = x
        assert x.tobytes() == first.tobytes()


# ---- 6. a uniform grid is solve_sim_draws -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,batched_sigma", [(3, False), (70, True)])
@pytest.mark.parametrize("p", [2, 3, 4, 5, 6])
def test_uniform_grid_against_solve_sim_draws(p, B, batched_sigma, monkeypatch):
    """An ``np.linspace`` grid is one slot: ``prior_at`` is called once, and the kernels differ from ``solve_sim_draws``'s only in
    where the one pair is read (FitzHugh-Nagumo does not read the time)."""
    C = draws.chunk()
    monkeypatch.setenv("RK_SIM_DRAWS_CHUNK", str(C))
    c = gc.fhn(p, "rodeo", "uniform", t_max=gc.T_MAX[p], B=B, batched_sigma=batched_sigma)
    t, calls = c["t"], []

    def prior_at(h):
        calls.append(h)
        return ra.ibm_init(h, p, c["sigma"])
    args = (c["ode"], c["W"], c["x0"])
    keep = [0, 1, 20, 40]
    x = ra.solve_sim_draws_grid(KEY, *args, t, gc.ITG["rodeo"][0], prior_at, n_draws=2 * C + 1, keep=keep, **c["params"])
    assert len(calls) == 1                                              # one slot
    want = ra.solve_sim_draws(KEY, *args, t[0], t[-1], len(t) - 1, gc.ITG["rodeo"][0], ra.ibm_init(calls[0], p, c["sigma"]),
                              n_draws=2 * C + 1, keep=keep, **c["params"])
    _close(x, want, p, f"uniform rodeo p={p} B={B} against solve_sim_draws")
    np.testing.assert_array_equal(x, want)


@pytest.mark.parametrize("p,itg,B,n_bobs", [(3, "kramer", 65, 1), (4, "kramer", 3, 2), (5, "rodeo", 3, 1)])
def test_dalton_uniform_grid_against_dalton_solve_sim_on_the_lanes(p, itg, B, n_bobs, monkeypatch):
    """Per-draw ``dalton.solve_sim(key + s)`` under RK_DALTON_LANES=1: dalton_fwd_kernel<store> with one (Q, R), then
    bwd_sim_kernel."""
    monkeypatch.setenv("RK_DALTON_LANES", "1")
    c = dc.make(gc.fhn(p, itg, "uniform", B=B), n_bobs=n_bobs)
    t = c["t"]
    obs = (c["y"], t[list(c["nodes"])], c["D"], c["Om"])
    unif = (c["ode"], c["W"], c["x0"], t[0], t[-1], len(t) - 1, gc.ITG[itg][0], ra.ibm_init(t[1] - t[0], p, c["sigma"])) + obs
    assert _kernels(lambda: dmod.solve_sim(KEY, *unif, **c["params"])) == ["dalton_fwd_kernel<store>", "bwd_sim_kernel"]
    want = np.stack([np.array(dmod.solve_sim(KEY + s, *unif, **c["params"])) for s in range(5)], axis=-4)
    x = _draws(c, KEY, 5)
    _close(x, want, p, f"dalton uniform {itg} p={p} B={B} n_bobs={n_bobs} against dalton.solve_sim on the lanes")
    np.testing.assert_array_equal(x, want)


# ---- 7. the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,key", restated_cases(), ids=lambda v: v["label"] if isinstance(v, dict) else str(v))
def test_against_the_restatement(c, key):
    N = len(c["t"]) - 1
    keep = None if N < 40 else [0, 1, 7, 39, 40]
    x = _draws(c, key, N_DRAWS, keep)
    want = dgr.restate(c, key, N_DRAWS, keep)
    assert np.all(np.isfinite(want))
    _close(x, want, c["p"], f"restatement {c['label']} key={key} n_draws={N_DRAWS} keep={'all' if keep is None else keep}")
    _node0_is_ode_init(x, c)


# ---- 8. a traced Python right-hand side -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", traced_cases(), ids=lambda c: c["label"])
def test_traced_python_right_hand_side(c):
    """The two right-hand sides round differently, so only a case whose restatement holds still under R (1 + 1e-15) can be judged
    by the bar: tests/test_oracle_draws_grid.py (c) vets these four."""
    built_in = _draws(c, TRACED_KEY, N_DRAWS, keep=[0, 20, 40])
    traced = _draws(c, TRACED_KEY, N_DRAWS, keep=[0, 20, 40], ode=_fitz)
    assert np.all(np.isfinite(traced))
    _close(traced, built_in, c["p"], f"traced {c['label']} against the built-in right-hand side")


# ---- 9. determinism, the seed law from outside, the launched kernels -------------------------------------------------------
@pytest.mark.parametrize("dalton", [False, True], ids=["plain", "dalton"])
def test_same_key_same_bytes_and_next_key_shifts_the_draws(dalton):
    C = draws.chunk()
    c = gc.fhn(3, "rodeo", "distinct", B=70, batched_sigma=True)
    if dalton:
        c = dc.make(c)
    n = 2 * C + 1
    a, again, b = _draws(c, 5, n), _draws(c, 5, n), _draws(c, 6, n)
    assert a.tobytes() == again.tobytes()
    np.testing.assert_array_equal(a[:, 1:], b[:, :-1])                        # draws 1 .. of key 5 are draws 0 .. of key 6
    assert not np.array_equal(a[:, 0], a[:, 1])                               # another seed, another path
    print(f"grid-draws-check seed law {'dalton ' if dalton else ''}: draws 1.. of key 5 are draws ..-1 of key 6 bit for bit")


def test_the_launches_are_the_filter_and_the_draws_kernel():
    c, c5, lz = gc.fhn(3, "kramer", "distinct", B=3), gc.fhn(5, "rodeo", "levels", B=3), gc.lorenz(3, "kramer", "distinct", B=5)
    for case in (c, c5, lz):
        assert _kernels(lambda: _draws(case, KEY, 5)) == ["grid_fwd_kernel", "grid_bwd_sim_draws_kernel"]
        assert _kernels(lambda: _draws(dc.make(case), KEY, 5)) == ["dalton_grid_fwd_kernel<store>", "grid_bwd_sim_draws_kernel"]
    assert _kernels(lambda: _draws(c, KEY, 5, ode=_fitz)) == ["grid_fwd_kernel<user>", "grid_bwd_sim_draws_kernel"]
    assert _kernels(lambda: _draws(dc.make(c), KEY, 5, ode=_fitz)) == ["dalton_grid_fwd_kernel<store, user>",
                                                                       "grid_bwd_sim_draws_kernel"]


# ---- 10. statistics -----------------------------------------------------------------------------------------------------------
def _pin(x, c, label):
    mean, var = dgr.pin_posterior(c)
    zmax, rmin, rmax = dro.pin_statistics(x, mean, var)
    zbar, lo, hi = dro.pin_bounds()
    print(f"grid-draws-check device pin {label}: largest z-score {zmax:.2f} (bar {zbar:.0f}), variance ratios {rmin:.3f} .. "
          f"{rmax:.3f} (allowed {lo:.3f} .. {hi:.3f})")
    return zmax, zmax <= zbar and lo <= rmin and rmax <= hi


def test_the_statistical_pin_on_the_device_output():
    c = dgr.pin_case()
    x = _draws(c, dro.PIN_KEY, dro.PIN_DRAWS)
    assert x.shape == (dro.PIN_DRAWS, dro.PIN_N + 1, 2, dro.PIN_P)
    assert _pin(x, c, "p(X | Z)")[1]


def test_the_dalton_pin_on_the_device_output():
    c = dgr.pin_dalton_case()
    x = _draws(c, dro.PIN_KEY, dro.PIN_DRAWS)
    assert x.shape == (dro.PIN_DRAWS, dro.PIN_N + 1, 2, dro.PIN_P)
    assert _pin(x, c, "p(X | Z, Y)")[1]
    zmax, ok = _pin(x, dgr.pin_data_free(c), "p(X | Z, Y) draws against p(X | Z)")
    assert zmax > dro.pin_bounds()[0] and not ok          # the pin tells these draws from a sample of the data-free posterior
