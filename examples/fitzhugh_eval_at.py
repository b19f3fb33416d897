"""
The quick-start problem of the reference's README (README.md:88-152) evaluated at 50 times that are NOT on the solver's
grid, with ``rodeo_amd.solve_mv_at``: the posterior between two nodes is a closed form of the filtered and smoothed moments
at the nodes around it (nothing is interrogated there), so the grid -- and with it the solver -- stays what it is, and only
the 50 records come back from the device.

    python examples/fitzhugh_eval_at.py            (needs an MI355X; prints the error against scipy's odeint)
"""
import os
import sys
import numpy as np
from scipy.integrate import odeint
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rodeo_amd as rodeo


def main():
    n_vars, n_deriv = 2, 3
    x0 = np.array([-1., 1.])
    theta = np.array([.2, .2, 3])
    W, fitz_init_pad = rodeo.utils.first_order_pad(rodeo.ode.fitzhugh_nagumo, n_vars, n_deriv)
    X0 = fitz_init_pad(x0, 0., theta=theta)
    t_min, t_max = 0., 40.
    sigma = np.array([.1] * n_vars)
    n_steps = 800
    dt = (t_max - t_min) / n_steps
    prior_pars = rodeo.prior.ibm_init(dt=dt, n_deriv=n_deriv, sigma=sigma)
    t_eval = np.sort(np.random.default_rng(0).uniform(t_min, t_max, 50))         # 50 times between the nodes
    mean, var = rodeo.solve_mv_at(
        key=0,
        ode_fun=rodeo.ode.fitzhugh_nagumo,
        ode_weight=W,
        ode_init=X0,
        t_min=t_min,
        t_max=t_max,
        n_steps=n_steps,
        interrogate=rodeo.interrogate.interrogate_kramer,
        prior_pars=prior_pars,
        t_eval=t_eval,
        prior_at=lambda h: rodeo.prior.ibm_init(dt=h, n_deriv=n_deriv, sigma=sigma),   # the same prior over a sub-step
        theta=theta
    )
    exact = odeint(lambda X, t: [theta[2] * (X[0] - X[0] ** 3 / 3 + X[1]), -(X[0] - theta[0] + theta[1] * X[1]) / theta[2]],
                   x0, np.concatenate([[t_min], t_eval]), rtol=1e-10, atol=1e-10)[1:]
    err = float(np.max(np.abs(mean[:, :, 0] - exact)))
    sd = float(np.max(np.sqrt(var[:, :, 0, 0])))
    print(f"solve_mv_at: output {mean.shape} / {var.shape}, max |rodeo - odeint| = {err:.3e}, largest posterior sd {sd:.3e}")
    return err


if __name__ == "__main__":
    main()
