"""
The quick start (FitzHugh-Nagumo, theta = (0.2, 0.2, 3), x0 = (-1, 1), n_deriv = 3, interrogate_kramer on [0, 4]) on the 72
uniform steps plus ten irregular observation times put in as nodes by ``grid_with_times``, with the prior scale sigma calibrated
ON THAT GRID: ``solve_evidence_grid`` / ``evidence_scale`` give one scale per variable for the horizon, which is fed to
``solve_mv_grid``; ``solve_mv_dynamic_grid`` estimates a scale per step and needs no sigma at all.  Prints sigma before and after,
the log-evidence, and the posterior mean and standard deviation at the ten times under the three priors next to a ``solve_ivp``
reference.  The numbers only.

    python examples/fitzhugh_calibrate_grid.py            (needs an MI355X)
"""
import os
import sys
import numpy as np
from scipy.integrate import solve_ivp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rodeo_amd as rodeo


def main(sigma=(0.5, 0.3)):
    n_vars, n_deriv = 2, 3
    theta = np.array([.2, .2, 3])
    ode = rodeo.ode.fitzhugh_nagumo
    W, fitz_init_pad = rodeo.utils.first_order_pad(ode, n_vars, n_deriv)
    X0 = fitz_init_pad(np.array([-1., 1.]), 0., theta=theta)
    t_min, t_max, n_steps = 0., 4., 72
    sigma = np.asarray(sigma, dtype=float)
    itg = rodeo.interrogate.interrogate_kramer

    def prior_with(s):
        return lambda h: rodeo.prior.ibm_init(dt=h, n_deriv=n_deriv, sigma=s)

    t_obs = np.sort(np.random.default_rng(0).uniform(t_min + 0.05, t_max - 0.05, 10))
    t_grid, node = rodeo.grid_with_times(np.linspace(t_min, t_max, n_steps + 1), t_obs)
    h = np.diff(t_grid)
    print(f"{len(h)} steps, {len(rodeo.grid_slots(t_grid)[0])} slots, h = {h.min():.2e} .. {h.max():.2e}")

    ev = rodeo.solve_evidence_grid(None, ode, W, X0, t_grid, itg, prior_with(sigma), theta=theta)
    c = rodeo.evidence_scale(ev)
    sigma_hat = sigma * np.sqrt(c)
    ev_hat = rodeo.solve_evidence_grid(None, ode, W, X0, t_grid, itg, prior_with(sigma_hat), theta=theta)
    print(f"sigma = {sigma}: log-evidence {ev.logdens:.2f}, quad / N = {c}")
    print(f"sigma_hat = sigma sqrt(quad / N) = {sigma_hat}: log-evidence {ev_hat.logdens:.2f} (evidence_at predicts "
          f"{rodeo.evidence_at(ev, c):.2f}), quad / N = {rodeo.evidence_scale(ev_hat)}")

    mean_0, var_0 = rodeo.solve_mv_grid(None, ode, W, X0, t_grid, itg, prior_with(sigma), theta=theta)
    mean_c, var_c = rodeo.solve_mv_grid(None, ode, W, X0, t_grid, itg, prior_with(sigma_hat), theta=theta)
    dyn = rodeo.solve_mv_dynamic_grid(None, ode, W, X0, t_grid, itg, prior_with(sigma), theta=theta)
    root = sigma * np.sqrt(dyn.scale)                                   # the per-step estimate of sigma: scale multiplies R_n
    print(f"dynamic: log-evidence {dyn.logdens:.2f}; per-step sigma estimates {root.min(axis=0)} .. {root.max(axis=0)}, "
          f"median {np.median(root, axis=0)}")

    a, b, cc = theta
    ref = solve_ivp(lambda t, y: [cc * (y[0] - y[0] ** 3 / 3 + y[1]), -(y[0] - a + b * y[1]) / cc], (t_min, t_max), [-1., 1.],
                    rtol=1e-12, atol=1e-12, dense_output=True).sol(t_obs).T
    print("        t | sigma as given: mean V, sd V   | calibrated on the grid         | dynamic                        | solve_ivp V")
    for k, n in enumerate(node):
        cols = [f"{m[n, 0, 0]: .5f}  {np.sqrt(v[n, 0, 0, 0]):.2e}" for m, v in ((mean_0, var_0), (mean_c, var_c), (dyn.mean, dyn.var))]
        print(f"  {t_obs[k]:7.4f} | " + "           | ".join(cols) + f"           | {ref[k, 0]: .5f}")
    return ev, ev_hat, (mean_c, var_c), dyn, ref


if __name__ == "__main__":
    main()
