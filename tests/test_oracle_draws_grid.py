"""
``solve_sim_draws_grid``'s law on the oracle alone (no GPU), tests/draws_grid_oracle.py:
(a) the statistical pin of tests/test_oracle_draws.py on a grid: 2048 draws under the seeds key, key + 1, .. of FitzHugh-Nagumo
    (n_bstate 3, kramer, 8 distinct steps on [0, 0.2], key 7) are a sample of ``grid_oracle.solve_mv_grid``'s posterior, within
    ``draws_oracle.pin_bounds()`` -- |z| <= 5 and variance ratios 0.844 .. 1.156 (found: 2.10 and 0.903 .. 1.041);
(b) the DALTON pin: the same problem with observations on nodes (0, 1, 4, 5, 8) at 100 x the prior scale, against
    ``dalton_grid_oracle.solve_mv_grid``'s posterior (found: 2.10 and 0.903 .. 1.041) -- and the same draws against the data-free
    posterior p(X | Z) at that scale FAIL the bound (found: |z| = 161.7), so the pin tells a sampler that ignores the data;
(c) every (case, seed + s) that tests/test_gpu_draws_grid.py compares with the restatement is a case its bar can judge: the
    restatement's own move under R (1 + 1e-15) stays below ``grid_cases.sim_bar(p)``.  (The pin problems are not among them: at
    scale 100 their move is 4.5e-7.)  The same for the four cases of its traced-against-built-in comparison: DALTON's at n_bstate 4
    runs at the plain prior scale, because at dalton_grid_cases' 100 x the restatement moves by 1.3e-7, above the 1e-7 bar;
(d) FitzHugh-Nagumo at n_bstate 6 on the 40 distinct steps of [0, 1] at B = 70 with a batched sigma has no finite solution in
    most of its trajectories -- the restatement overflows as the device does (steps down to 0.009, prior variances down to
    1e-29) -- so the device test compares the non-finite entries of that case as a pattern and holds the finite ones to the bar.
The device output goes through the same functions with the same bounds: the Philox stream is the oracle's.
"""
import numpy as np
import pytest
import grid_cases as gc
import dalton_grid_cases as dgc
import draws_oracle as dro
import draws_grid_oracle as dgr

N_DRAWS = 5                                               # of the restatement comparisons on the device


def restated_cases():
    """(case, key) of tests/test_gpu_draws_grid.py's comparison with the restatement: the vetted sampler cases of the two grid
    families, without the chkrebtii one (not served: its forward pass depends on the key)."""
    return [(c, key) for c, key in gc.sim_cases() if c["itg"] != "chkrebtii"] + list(dgc.sim_cases())


TRACED_KEY = 11


def traced_cases():
    """The cases of tests/test_gpu_draws_grid.py's traced-against-built-in comparison (the key is TRACED_KEY): plain and DALTON at
    n_bstate 3 and 4; DALTON's at 4 at the plain prior scale (at 100 x its restatement moves by 1.3e-7 under R (1 + 1e-15))."""
    plain = [gc.fhn(p, "kramer", "distinct", B=3) for p in (3, 4)]
    return plain + [dgc.make(plain[0]), dgc.make(plain[1], scale=1.0)]


def _pin(x, c, label):
    mean, var = dgr.pin_posterior(c)
    assert np.all(var[1:] > 0)
    zmax, rmin, rmax = dro.pin_statistics(x, mean, var)
    zbar, lo, hi = dro.pin_bounds()
    print(f"grid-draws-check oracle pin {label}: largest z-score {zmax:.2f} (bar {zbar:.0f}), variance ratios {rmin:.3f} .. "
          f"{rmax:.3f} (allowed {lo:.3f} .. {hi:.3f})")
    return zmax, zmax <= zbar and lo <= rmin and rmax <= hi


def test_draws_are_a_sample_of_the_grid_posterior():
    c = dgr.pin_case()
    x = dgr.restate(c, dro.PIN_KEY, dro.PIN_DRAWS)
    assert x.shape == (dro.PIN_DRAWS, dro.PIN_N + 1, 2, dro.PIN_P)
    np.testing.assert_array_equal(x[:, 0], np.broadcast_to(c["x0"], x[:, 0].shape))         # node 0 is ode_init in every draw
    assert _pin(x, c, "p(X | Z)")[1]
    assert np.unique(x[:, -1, 0, 0]).size == dro.PIN_DRAWS                                  # a sample, not one path repeated


def test_dalton_draws_are_a_sample_of_the_posterior_given_the_data():
    c = dgr.pin_dalton_case()
    x = dgr.restate(c, dro.PIN_KEY, dro.PIN_DRAWS)
    assert x.shape == (dro.PIN_DRAWS, dro.PIN_N + 1, 2, dro.PIN_P)
    np.testing.assert_array_equal(x[:, 0], np.broadcast_to(c["x0"], x[:, 0].shape))
    assert _pin(x, c, "p(X | Z, Y)")[1]
    zmax, ok = _pin(x, dgr.pin_data_free(c), "p(X | Z, Y) draws against p(X | Z)")
    assert zmax > dro.pin_bounds()[0] and not ok          # the pin tells these draws from a sample of the data-free posterior


def test_keep_restricts_the_restatement():
    c = dgr.pin_case()
    full = dgr.restate(c, 3, 2)
    np.testing.assert_array_equal(dgr.restate(c, 3, 2, keep=[0, 5, 8]), full[:, [0, 5, 8]])


@pytest.mark.parametrize("c,key", restated_cases() + [(c, TRACED_KEY) for c in traced_cases()], ids=lambda v: v["label"] if isinstance(v, dict) else str(v))
def test_gpu_restated_cases_are_well_conditioned(c, key):
    bar = gc.sim_bar(c["p"])
    x, x2 = dgr.restate(c, key, N_DRAWS), dgr.restate(c, key, N_DRAWS, r_scale=1.0 + 1e-15)
    assert np.all(np.isfinite(x))
    moves = np.max(np.abs(x2 - x), axis=tuple(i for i in range(x.ndim) if i != x.ndim - 4)) / np.max(np.abs(x))
    print(f"grid-draws-case {c['label']} key={key}: restatement moves by {', '.join(f'{m:.3e}' for m in moves)} of max|x| under "
          f"R (1 + 1e-15), seeds key .. key + {N_DRAWS - 1} (bar {bar:.0e})")
    assert np.all(moves < bar), (c["label"], moves)


def test_the_n_bstate_six_batch_on_distinct_steps_overflows_in_the_restatement_too():
    """(d): trajectories from 20 on are not finite, on "distinct" only; the first trajectories are."""
    for kind, finite in (("levels", True), ("distinct", False)):
        c = gc.fhn(6, "rodeo", kind, t_max=gc.T_MAX[6], B=70, batched_sigma=True)
        with np.errstate(all="ignore"):
            ok = np.all(np.isfinite(c.restate_sim(11)), axis=(1, 2, 3))
        print(f"grid-draws-case {c['label']}: {int(ok.sum())} of 70 restated paths are finite")
        assert ok.all() == finite and ok[:3].all()
