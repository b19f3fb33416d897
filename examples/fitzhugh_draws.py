"""
The quick start (FitzHugh-Nagumo, theta = (0.2, 0.2, 3), x0 = (-1, 1), n_deriv = 3, 800 steps on [0, 40], sigma = 0.1,
interrogate_kramer) with ``solve_sim_draws``: 100 sample paths from one forward filter, stored and downloaded at 50 of the 801
nodes only.  Prints, for V at every fifth kept node, the 5 % and 95 % quantiles of the draws next to ``solve_mv``'s
mean -+ 1.645 sd -- the same 90 % band from the smoothed moments -- and how many of the 50 x 2 bands agree to a tenth of their
width.  Draw s is ``solve_sim(key + s, ...)`` at those nodes; one such call is made to show it.

    python examples/fitzhugh_draws.py            (needs an MI355X)
"""
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rodeo_amd as rodeo


def main(n_draws=100, key=0):
    n_vars, n_deriv = 2, 3
    theta = np.array([.2, .2, 3])
    W, fitz_init_pad = rodeo.utils.first_order_pad(rodeo.ode.fitzhugh_nagumo, n_vars, n_deriv)
    X0 = fitz_init_pad(np.array([-1., 1.]), 0., theta=theta)
    t_min, t_max, n_steps = 0., 40., 800
    dt = (t_max - t_min) / n_steps
    prior_pars = rodeo.prior.ibm_init(dt=dt, n_deriv=n_deriv, sigma=np.array([.1] * n_vars))
    args = (rodeo.ode.fitzhugh_nagumo, W, X0, t_min, t_max, n_steps, rodeo.interrogate.interrogate_kramer, prior_pars)
    keep = np.arange(16, n_steps + 1, 16)                           # 50 nodes: t = 0.8, 1.6, .., 40

    x = rodeo.solve_sim_draws(key, *args, n_draws=n_draws, keep=keep, theta=theta)        # (100, 50, 2, 3)
    lo, hi = np.quantile(x[..., 0], [0.05, 0.95], axis=0)           # (50, 2): the band of V and R from the draws
    mean, var = rodeo.solve_mv(None, *args, theta=theta)
    m, sd = mean[keep, :, 0], np.sqrt(var[keep, :, 0, 0])
    print(f"solve_sim_draws: {x.shape[0]} draws at {x.shape[1]} of {n_steps + 1} nodes, output {x.shape}")
    print("     t    draws: 5 % .. 95 % of V        solve_mv: mean -+ 1.645 sd of V")
    for k in range(4, keep.size, 5):
        print(f"  {t_min + dt * keep[k]:5.1f}   {lo[k, 0]: .5f} .. {hi[k, 0]: .5f}         "
              f"{m[k, 0] - 1.645 * sd[k, 0]: .5f} .. {m[k, 0] + 1.645 * sd[k, 0]: .5f}")
    width = 2 * 1.645 * sd
    near = (np.abs(lo - (m - 1.645 * sd)) < 0.1 * width) & (np.abs(hi - (m + 1.645 * sd)) < 0.1 * width)
    print(f"bands whose two ends agree to a tenth of the width: {int(near.sum())} of {near.size}")
    one = rodeo.solve_sim(key + 3, *args, theta=theta)[keep]
    print(f"draw 3 against solve_sim(key + 3)[keep]: max difference {float(np.max(np.abs(x[3] - one))):.1e}")
    return x, lo, hi


if __name__ == "__main__":
    main()
