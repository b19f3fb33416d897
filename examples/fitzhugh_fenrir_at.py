"""
The quick-start problem of the reference's README (README.md:88-152) with noisy observations at IRREGULAR times: Fenrir's
log-likelihood of the true parameters and of a few wrong ones, once with ``fenrir`` -- which moves every observation to the
next grid node -- and once with ``fenrir_at``, which conditions the backward chain on it at its own time, on a coarse grid
(dt = 0.2) and on a fine one (dt = 0.025).  What to look for: on the coarse grid ``fenrir`` treats data taken up to 0.2 time
units earlier as if the solution had produced them at the node, so the two columns should differ there, and they should come
together as the grid is refined.  The script prints the numbers; it asserts nothing about them.

    python examples/fitzhugh_fenrir_at.py          (needs an MI355X)
"""
import os
import sys
import numpy as np
from scipy.integrate import odeint
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rodeo_amd as rodeo
from rodeo_amd.inference.fenrir import fenrir, fenrir_at


def main():
    n_vars, n_deriv = 2, 3
    x0 = np.array([-1., 1.])
    theta = np.array([.2, .2, 3])
    W, fitz_init_pad = rodeo.utils.first_order_pad(rodeo.ode.fitzhugh_nagumo, n_vars, n_deriv)
    X0 = fitz_init_pad(x0, 0., theta=theta)
    t_min, t_max = 0., 40.
    sigma = np.array([.1] * n_vars)
    rng = np.random.default_rng(0)
    # irregular: none sits on a grid node (fenrir, like the reference, takes one observation per node of the coarse grid)
    obs_times = (np.sort(rng.choice(np.arange(3, 200), 40, replace=False)) + rng.uniform(0.05, 0.95, 40)) * 0.2
    exact = odeint(lambda X, t: [theta[2] * (X[0] - X[0] ** 3 / 3 + X[1]), -(X[0] - theta[0] + theta[1] * X[1]) / theta[2]],
                   x0, np.concatenate([[t_min], obs_times]), rtol=1e-10, atol=1e-10)[1:]
    noise_sd = 0.05
    obs_data = (exact + noise_sd * rng.standard_normal(exact.shape))[:, :, None]
    obs_weight = np.zeros((len(obs_times), n_vars, 1, n_deriv))
    obs_weight[..., 0] = 1.0
    obs_var = np.full((len(obs_times), n_vars, 1, 1), noise_sd ** 2)
    thetas = theta * np.array([1.0, 0.9, 1.1, 1.25])[:, None]                      # the truth first
    out = {}
    for n_steps in (200, 1600):
        dt = (t_max - t_min) / n_steps
        prior_pars = rodeo.prior.ibm_init(dt=dt, n_deriv=n_deriv, sigma=sigma)
        args = (None, rodeo.ode.fitzhugh_nagumo, W, X0, t_min, t_max, n_steps, rodeo.interrogate.interrogate_kramer, prior_pars,
                obs_data, obs_times, obs_weight, obs_var)
        snapped = fenrir(*args, theta=thetas)
        at = fenrir_at(*args, lambda h: rodeo.prior.ibm_init(dt=h, n_deriv=n_deriv, sigma=sigma), theta=thetas)
        out[n_steps] = (snapped, at)
        print(f"dt = {dt:g}: theta scale    1.0       0.9       1.1       1.25")
        print("   fenrir   (snapped) " + " ".join(f"{v:9.2f}" for v in snapped))
        print("   fenrir_at (in place)" + " ".join(f"{v:9.2f}" for v in at))
    return out


if __name__ == "__main__":
    main()
