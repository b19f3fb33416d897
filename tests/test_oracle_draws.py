"""
A statistical pin of ``solve_sim_draws``'s law on the oracle alone (no GPU), independent of ``solve_sim`` as a yardstick: 2048
draws under the seeds key, key + 1, .. of FitzHugh-Nagumo (n_bstate 3, N = 8, t_max = 0.2, kramer, key 7) are a sample of
``solve_mv``'s posterior -- at every node >= 1 every entry's sample mean lies within 5 sd / sqrt(S) of the smoothed mean and its
sample variance over the smoothed variance within 1 +- 5 sqrt(2 / (S - 1)) (0.844 .. 1.156).  The device output goes through
the same function with the same bounds (tests/test_gpu_draws.py): the Philox stream is the oracle's, so this run predicts it.
"""
import numpy as np
import rodeo_amd as ra
from oracle import odes, interrogations as oi
import draws_oracle as dro


def test_draws_are_a_sample_of_the_smoothed_posterior():
    c = dro.pin_problem(ra)
    x = dro.solve_sim_draws(dro.PIN_KEY, odes.fitzhugh_nagumo, c["W"], c["x0"], 0.0, dro.PIN_T_MAX, dro.PIN_N, oi.interrogate_kramer,
                            c["prior"], n_draws=dro.PIN_DRAWS, theta=c["theta"])
    assert x.shape == (dro.PIN_DRAWS, dro.PIN_N + 1, 2, dro.PIN_P)
    np.testing.assert_array_equal(x[:, 0], np.broadcast_to(c["x0"], x[:, 0].shape))         # node 0 is ode_init in every draw
    mean, var = dro.pin_posterior(c)
    assert np.all(var[1:] > 0)
    zmax, rmin, rmax = dro.pin_statistics(x, mean, var)
    zbar, lo, hi = dro.pin_bounds()
    print(f"draws-check oracle pin: largest z-score {zmax:.2f} (bar {zbar:.0f}), variance ratios {rmin:.3f} .. {rmax:.3f} "
          f"(allowed {lo:.3f} .. {hi:.3f})")
    assert zmax <= zbar and lo <= rmin and rmax <= hi
    # the draws differ from one another (a sample, not one path repeated)
    assert np.unique(x[:, -1, 0, 0]).size == dro.PIN_DRAWS
