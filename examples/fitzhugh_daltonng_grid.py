"""
FitzHugh-Nagumo observed through Poisson counts Y_ij ~ Poisson(exp(b0 + b1 x_j(t_i))) at IRREGULAR times t_i (the model of
examples/fitzhugh_daltonng.py): the log-likelihood of theta

* by ``daltonng`` on a uniform grid, which moves every observation time to a grid node (``searchsorted``), and
* by ``daltonng_grid`` on the grid ``grid_with_times`` returns, which has every observation time as a node and the uniform grid's
  nodes in between,

over a batch of values of c, the parameter the counts say most about.  ``solve_mv_nn_grid`` then gives the posterior mean of V at
the observation times themselves.  Both are imported from ``rodeo_amd.inference.dalton`` (the package does not re-export them).

    python examples/fitzhugh_daltonng_grid.py            (needs an MI355X)
"""
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rodeo_amd as rodeo
from rodeo_amd.inference.dalton import daltonng, daltonng_grid, solve_mv_nn_grid
from rodeo_amd.trace import gammaln

b0, b1 = 0.1, 0.5
n_deriv, sigma = 3, np.array([0.1, 0.1])
t_min, t_max, n_steps = 0.0, 40.0, 400
theta = np.array([0.2, 0.2, 3.0])


def obs_loglik_i(obs_data_i, ode_data_i, ind, **params):
    eta = b0 + b1 * ode_data_i[:, 0]
    y = obs_data_i.flatten()
    return np.sum(y * eta - np.exp(eta) - gammaln(y + 1.0))


def main():
    fitz = rodeo.ode.fitzhugh_nagumo
    W, init = rodeo.utils.first_order_pad(fitz, 2, n_deriv)
    X0 = init(np.array([-1.0, 1.0]), 0.0, theta=theta)
    kramer = rodeo.interrogate.interrogate_kramer
    rng = np.random.default_rng(0)
    obs_times = np.sort(rng.uniform(0.5, t_max, 60))                 # counts arrive at their own times
    t_uniform = np.linspace(t_min, t_max, n_steps + 1)
    t_grid, nodes = rodeo.grid_with_times(t_uniform, obs_times)
    print(f"{len(obs_times)} observation times; uniform grid {n_steps} steps, grid with the times {len(t_grid) - 1} steps in "
          f"{len(rodeo.grid_slots(t_grid)[0])} slots")

    def prior_at(h):
        return rodeo.ibm_init(h, n_deriv, sigma)

    # the data: counts at the true times, from a fine solve
    fine = 4000
    Xt, _ = rodeo.solve_mv(None, fitz, W, X0, t_min, t_max, fine, kramer, rodeo.ibm_init((t_max - t_min) / fine, n_deriv, sigma),
                           theta=theta)
    x_true = np.stack([np.interp(obs_times, np.linspace(t_min, t_max, fine + 1), Xt[:, j, 0]) for j in range(2)], axis=1)
    obs_data = rng.poisson(np.exp(b0 + b1 * x_true)).astype(np.float64)[:, :, None]

    # log-likelihood over a batch of c; the rounded times must still be distinct nodes of the uniform grid
    c_values = np.linspace(2.0, 4.0, 9)
    thetas = np.tile(theta, (len(c_values), 1))
    thetas[:, 2] = c_values
    X0s = np.stack([init(np.array([-1.0, 1.0]), 0.0, theta=th) for th in thetas])
    idx = np.searchsorted(t_uniform, obs_times)
    keep = np.concatenate([[True], np.diff(idx) > 0])                # daltonng takes one observation per node: later ones are dropped
    ll_round = daltonng(None, fitz, W, X0s, t_min, t_max, n_steps, kramer, prior_at((t_max - t_min) / n_steps), obs_data[keep],
                        obs_times[keep], obs_loglik_i, theta=thetas)
    ll_grid = daltonng_grid(None, fitz, W, X0s, t_grid, kramer, prior_at, obs_data, obs_times, obs_loglik_i, theta=thetas)
    print(f"daltonng on the uniform grid keeps {int(keep.sum())} of {len(obs_times)} observations (times moved by up to "
          f"{np.max(t_uniform[idx] - obs_times):.3f}); daltonng_grid keeps all, at their own times")
    print("   c                    ", np.array2string(c_values, precision=2))
    print("   daltonng, rounded    ", np.array2string(ll_round - ll_round.max(), precision=2))
    print("   daltonng_grid        ", np.array2string(ll_grid - ll_grid.max(), precision=2))
    mean, var = solve_mv_nn_grid(None, fitz, W, X0, t_grid, kramer, prior_at, obs_data, obs_times, obs_loglik_i, theta=theta)
    print("   posterior mean of V at the first five observation times", np.array2string(mean[nodes[:5], 0, 0], precision=4),
          "true", np.array2string(x_true[:5, 0], precision=4))
    return ll_round, ll_grid


if __name__ == "__main__":
    main()
