"""
The quick start (FitzHugh-Nagumo, theta = (0.2, 0.2, 3), x0 = (-1, 1), n_deriv = 3, sigma = 0.1, interrogate_kramer) on a grid of
200 steps on [0, 40] with ten irregular observation times put in as nodes by ``grid_with_times``.  ``solve_sim_draws_grid`` draws
100 sample paths from one forward filter and stores them at those ten nodes only; ``dalton.solve_sim_draws_grid`` does the same
from the joint filter that has seen the (noisy) data.  Prints, for V at every observation time, the 5 % and 95 % quantiles of
the draws from p(X | Z) next to ``solve_mv_grid``'s mean -+ 1.645 sd -- the same 90 % band from the smoothed moments -- and the
band of the draws from p(X | Z, Y) next to ``dalton.solve_mv_grid``'s.  At the quick start's sigma the solver's own band is far
narrower than the observation noise, so the data move it little.  The script prints the numbers; it asserts nothing.

    python examples/fitzhugh_draws_grid.py            (needs an MI355X)
"""
import os
import sys
import numpy as np
from scipy.integrate import odeint
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rodeo_amd as rodeo
from rodeo_amd.inference.dalton import solve_mv_grid as dalton_solve_mv_grid, solve_sim_draws_grid as dalton_solve_sim_draws_grid


def main(n_draws=100, key=0):
    n_vars, n_deriv = 2, 3
    x0 = np.array([-1., 1.])
    theta = np.array([.2, .2, 3])
    W, fitz_init_pad = rodeo.utils.first_order_pad(rodeo.ode.fitzhugh_nagumo, n_vars, n_deriv)
    X0 = fitz_init_pad(x0, 0., theta=theta)
    t_min, t_max, n_steps = 0., 40., 200
    sigma = np.array([.1] * n_vars)
    rng = np.random.default_rng(0)
    obs_times = np.sort(rng.uniform(2.0, 39.0, 10))                 # ten times that are no nodes of the uniform grid
    exact = odeint(lambda X, t: [theta[2] * (X[0] - X[0] ** 3 / 3 + X[1]), -(X[0] - theta[0] + theta[1] * X[1]) / theta[2]],
                   x0, np.concatenate([[t_min], obs_times]), rtol=1e-10, atol=1e-10)[1:]
    noise_sd = 0.05
    obs_data = (exact + noise_sd * rng.standard_normal(exact.shape))[:, :, None]
    obs_weight = np.zeros((len(obs_times), n_vars, 1, n_deriv))
    obs_weight[..., 0] = 1.0
    obs_var = np.full((len(obs_times), n_vars, 1, 1), noise_sd ** 2)
    obs = (obs_data, obs_times, obs_weight, obs_var)

    def prior_at(h):
        return rodeo.prior.ibm_init(dt=h, n_deriv=n_deriv, sigma=sigma)
    t_grid, node = rodeo.grid_with_times(np.linspace(t_min, t_max, n_steps + 1), obs_times)
    on_grid = (rodeo.ode.fitzhugh_nagumo, W, X0, t_grid, rodeo.interrogate.interrogate_kramer, prior_at)

    x = rodeo.solve_sim_draws_grid(key, *on_grid, n_draws=n_draws, keep=node, theta=theta)                 # (100, 10, 2, 3)
    xy = dalton_solve_sim_draws_grid(key, *on_grid, *obs, n_draws=n_draws, keep=node, theta=theta)
    print(f"{len(t_grid)} nodes after grid_with_times ({len(rodeo.grid_slots(t_grid)[0])} slots); {x.shape[0]} draws at "
          f"{x.shape[1]} of them, output {x.shape}")
    out = {}
    for name, draws, (mean, var) in (("p(X | Z)", x, rodeo.solve_mv_grid(None, *on_grid, theta=theta)),
                                     ("p(X | Z, Y)", xy, dalton_solve_mv_grid(None, *on_grid, *obs, theta=theta))):
        lo, hi = np.quantile(draws[..., 0], [0.05, 0.95], axis=0)   # (10, 2): the band of V and R from the draws
        m, sd = mean[node, :, 0], np.sqrt(var[node, :, 0, 0])
        print(f"{name}:    t    data V    draws: 5 % .. 95 % of V      mean -+ 1.645 sd of V       exact V")
        for i, t in enumerate(obs_times):
            print(f"         {t:7.3f} {obs_data[i, 0, 0]:8.3f}    {lo[i, 0]: .4f} .. {hi[i, 0]: .4f}         "
                  f"{m[i, 0] - 1.645 * sd[i, 0]: .4f} .. {m[i, 0] + 1.645 * sd[i, 0]: .4f}       {exact[i, 0]:8.3f}")
        out[name] = (lo, hi, m, sd)
    one = rodeo.solve_sim_grid(key + 3, *on_grid, theta=theta)[node]
    print(f"draw 3 against solve_sim_grid(key + 3)[nodes]: max difference {float(np.max(np.abs(x[3] - one))):.1e}")
    return out


if __name__ == "__main__":
    main()
