"""
examples/fitzhugh_dalton_grid.py's data and grid -- the quick-start problem with noisy observations at IRREGULAR times on a coarse
grid (dt = 0.2) -- with Fenrir, three ways side by side: ``fenrir``, which moves every observation to the next grid node;
``fenrir_at``, which conditions on it at its own time between two nodes; and ``fenrir_grid`` on ``grid_with_times(t_grid,
obs_times)``, the grid with the observation times put in as nodes, where the solver also interrogates the ODE at those times.
Then the data-adaptive solver on that grid: ``fenrir.solve_mv_grid``'s smoothed mean +- 2 sd of both variables at the first
observation times next to the plain ``solve_mv_grid``'s, which has not seen the data.  The solver runs with
``interrogate_rodeo``: Fenrir's smoothing sweep inverts the backward filter's predicted variances, which the exact measurement of
``interrogate_kramer`` can leave singular.  The script prints the numbers; it asserts nothing about them.

    python examples/fitzhugh_fenrir_grid.py          (needs an MI355X)
"""
import os
import sys
import numpy as np
from scipy.integrate import odeint
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rodeo_amd as rodeo
from rodeo_amd.inference.fenrir import fenrir, fenrir_at, fenrir_grid, solve_mv_grid


def main():
    n_vars, n_deriv = 2, 3
    x0 = np.array([-1., 1.])
    theta = np.array([.2, .2, 3])
    W, fitz_init_pad = rodeo.utils.first_order_pad(rodeo.ode.fitzhugh_nagumo, n_vars, n_deriv)
    X0 = fitz_init_pad(x0, 0., theta=theta)
    t_min, t_max, n_steps = 0., 40., 200
    sigma = np.array([.1] * n_vars)
    rng = np.random.default_rng(0)
    obs_times = (np.sort(rng.choice(np.arange(3, 200), 40, replace=False)) + rng.uniform(0.05, 0.95, 40)) * 0.2
    exact = odeint(lambda X, t: [theta[2] * (X[0] - X[0] ** 3 / 3 + X[1]), -(X[0] - theta[0] + theta[1] * X[1]) / theta[2]],
                   x0, np.concatenate([[t_min], obs_times]), rtol=1e-10, atol=1e-10)[1:]
    noise_sd = 0.05
    obs_data = (exact + noise_sd * rng.standard_normal(exact.shape))[:, :, None]
    obs_weight = np.zeros((len(obs_times), n_vars, 1, n_deriv))
    obs_weight[..., 0] = 1.0
    obs_var = np.full((len(obs_times), n_vars, 1, 1), noise_sd ** 2)
    thetas = theta * np.array([1.0, 0.9, 1.1, 1.25])[:, None]                      # the truth first
    itg = rodeo.interrogate.interrogate_kramer

    def prior_at(h):
        return rodeo.prior.ibm_init(dt=h, n_deriv=n_deriv, sigma=sigma)
    obs = (obs_data, obs_times, obs_weight, obs_var)
    uniform = (None, rodeo.ode.fitzhugh_nagumo, W, X0, t_min, t_max, n_steps, itg, prior_at((t_max - t_min) / n_steps)) + obs
    t_grid, node = rodeo.grid_with_times(np.linspace(t_min, t_max, n_steps + 1), obs_times)
    snapped = fenrir(*uniform, theta=thetas)
    at = fenrir_at(*uniform, prior_at, theta=thetas)
    grid = fenrir_grid(None, rodeo.ode.fitzhugh_nagumo, W, X0, t_grid, itg, prior_at, *obs, theta=thetas)
    print(f"dt = {(t_max - t_min) / n_steps:g}, {len(t_grid)} nodes after grid_with_times ({len(rodeo.grid_slots(t_grid)[0])} slots): theta scale"
          "    1.0       0.9       1.1       1.25")
    print("   fenrir      (snapped)         " + " ".join(f"{v:9.2f}" for v in snapped))
    print("   fenrir_at   (between nodes)   " + " ".join(f"{v:9.2f}" for v in at))
    print("   fenrir_grid (times are nodes) " + " ".join(f"{v:9.2f}" for v in grid))
    on_grid = (None, rodeo.ode.fitzhugh_nagumo, W, X0, t_grid, rodeo.interrogate.interrogate_rodeo, prior_at)
    mean, var = solve_mv_grid(*on_grid, *obs, theta=theta)
    plain_mean, plain_var = rodeo.solve_mv_grid(*on_grid, theta=theta)
    print("   t        data V   p(X | Z, Y): V +- 2 sd     p(X | Z): V +- 2 sd      exact V")
    for i in range(0, len(obs_times), 5):
        k = node[i]
        print(f"   {obs_times[i]:7.3f} {obs_data[i, 0, 0]:8.3f}   {mean[k, 0, 0]:8.3f} +- {2 * np.sqrt(var[k, 0, 0, 0]):.3f}       "
              f"{plain_mean[k, 0, 0]:8.3f} +- {2 * np.sqrt(plain_var[k, 0, 0, 0]):.3f}     {exact[i, 0]:8.3f}")
    return dict(snapped=snapped, at=at, grid=grid, mean=mean, var=var, plain_mean=plain_mean, plain_var=plain_var)


if __name__ == "__main__":
    main()
