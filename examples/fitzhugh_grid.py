"""
The quick start (FitzHugh-Nagumo, theta = (0.2, 0.2, 3), x0 = (-1, 1), n_deriv = 3, interrogate_kramer on [0, 4]) on two
grids: the 72 uniform steps, and those nodes plus ten irregular observation times (``solve_mv_grid``: the solver on the grid it
is given).  Prints the posterior mean and standard deviation of both variables at the ten times from the grid that holds them
as nodes, next to ``solve_mv_at``'s (the uniform grid's posterior evaluated between its nodes) and a ``solve_ivp`` reference.
The numbers only.

    python examples/fitzhugh_grid.py            (needs an MI355X)
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
    W, fitz_init_pad = rodeo.utils.first_order_pad(rodeo.ode.fitzhugh_nagumo, n_vars, n_deriv)
    X0 = fitz_init_pad(np.array([-1., 1.]), 0., theta=theta)
    t_min, t_max, n_steps = 0., 4., 72
    sigma = np.asarray(sigma, dtype=float)
    itg = rodeo.interrogate.interrogate_kramer

    def prior_at(h):
        return rodeo.prior.ibm_init(dt=h, n_deriv=n_deriv, sigma=sigma)

    uniform = np.linspace(t_min, t_max, n_steps + 1)
    t_obs = np.sort(np.random.default_rng(0).uniform(t_min + 0.05, t_max - 0.05, 10))
    t_grid = np.union1d(uniform, t_obs)
    h_rep, slot = rodeo.grid_slots(t_grid)
    print(f"uniform grid: {len(uniform) - 1} steps, 1 slot; with the ten times: {len(t_grid) - 1} steps, {len(h_rep)} slots "
          f"(prior_at is called once per slot), h = {np.diff(t_grid).min():.2e} .. {np.diff(t_grid).max():.2e}")

    mean_u, var_u = rodeo.solve_mv_grid(None, rodeo.ode.fitzhugh_nagumo, W, X0, uniform, itg, prior_at, theta=theta)
    mean_g, var_g = rodeo.solve_mv_grid(None, rodeo.ode.fitzhugh_nagumo, W, X0, t_grid, itg, prior_at, theta=theta)
    mean_a, var_a = rodeo.solve_mv_at(None, rodeo.ode.fitzhugh_nagumo, W, X0, t_min, t_max, n_steps, itg,
                                      prior_at((t_max - t_min) / n_steps), t_obs, prior_at, theta=theta)
    a, b, c = theta
    ref = solve_ivp(lambda t, y: [c * (y[0] - y[0] ** 3 / 3 + y[1]), -(y[0] - a + b * y[1]) / c], (t_min, t_max), [-1., 1.],
                    rtol=1e-12, atol=1e-12, dense_output=True).sol(t_obs).T
    at = np.searchsorted(t_grid, t_obs)
    print("        t | solve_mv_grid (times as nodes): mean, sd     | solve_mv_at (72 uniform steps): mean, sd      | solve_ivp")
    for k, n in enumerate(at):
        g = (*mean_g[n, :, 0], *np.sqrt(var_g[n, :, 0, 0]))
        e = (*mean_a[k, :, 0], *np.sqrt(var_a[k, :, 0, 0]))
        print(f"  {t_obs[k]:7.4f} | ({g[0]: .5f}, {g[1]: .5f}) ({g[2]:.2e}, {g[3]:.2e}) | ({e[0]: .5f}, {e[1]: .5f}) ({e[2]:.2e}, {e[3]:.2e}) "
              f"| ({ref[k, 0]: .5f}, {ref[k, 1]: .5f})")
    print(f"uniform grid through solve_mv_grid, mean at t_max: {mean_u[-1, :, 0]}")
    return (mean_u, var_u), (mean_g, var_g), (mean_a, var_a), ref


if __name__ == "__main__":
    main()
