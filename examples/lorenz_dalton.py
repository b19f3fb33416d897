"""
docs/examples/lorenz.md of the reference on this build: the chaotic Lorenz63 system with noisy observations, solved by
DALTON's data-adaptive solver (``rodeo.inference.dalton.solve_mv``, the document's ``dsolve``) and by Fenrir's
(``rodeo.inference.fenrir.solve_mv``), with the document's ``lorenz`` function (traced into device code) and its settings
(n_deriv = 3, sigma = 5e7, 20 observations, 200 solver steps between observations).  The document's conclusion is that only
dalton recovers the true ODE solution beyond t > 7.5; ``main()`` returns the largest distance of each solver's mean to the
``odeint`` solution between the observations on 7.5 <= t <= 20.

    python examples/lorenz_dalton.py        (needs an MI355X)
"""
import os
import sys
import numpy as np
from scipy.integrate import odeint

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from rodeo_amd.utils import first_order_pad
from rodeo_amd.prior import ibm_init
from rodeo_amd.interrogate import interrogate_kramer
from rodeo_amd.inference.dalton import solve_mv as dsolve
from rodeo_amd.inference.fenrir import solve_mv as fsolve


def lorenz0(X_t, t, theta):
    rho, sigma, beta = theta
    x, y, z = X_t
    return np.array([-sigma * x + sigma * y, rho * x - y - x * z, -beta * z + x * y])


def lorenz(X_t, t, theta):
    rho, sigma, beta = theta
    x, y, z = X_t[:, 0]
    dx = -sigma * x + sigma * y
    dy = rho * x - y - x * z
    dz = -beta * z + x * y
    return np.array([[dx], [dy], [dz]])


def main():
    tmin, tmax = 0., 20.
    theta = np.array([28, 10, 8 / 3])
    ode0 = np.array([-12., -5., 38.])
    n_obs = 20
    obs_times = np.linspace(tmin, tmax, n_obs + 1)
    exact_obs = odeint(lorenz0, ode0, obs_times, args=(theta,), rtol=1e-12, atol=1e-12)
    gamma = np.sqrt(.005)
    obs = exact_obs + gamma * np.random.default_rng(0).normal(loc=0.0, scale=1, size=exact_obs.shape)

    n_deriv, n_vars = 3, 3
    sigma = np.array([5e7] * n_vars)
    W, lorenz_init_pad = first_order_pad(lorenz, n_vars, n_deriv)
    x0 = lorenz_init_pad(ode0, 0, theta=theta)
    n_res = 200
    n_steps = n_obs * n_res
    dt = (tmax - tmin) / n_steps
    prior_pars = ibm_init(dt, n_deriv, sigma)
    key = 0

    n_meas = 1
    obs_data = np.expand_dims(obs, -1)
    obs_weight = np.zeros((len(obs_data), n_vars, n_meas, n_deriv)); obs_weight[:, :, :, 0] = 1
    obs_var = np.zeros((len(obs_data), n_vars, n_meas, n_meas)); obs_var[:, :, :, 0] = gamma ** 2

    dsol, _ = dsolve(key, lorenz, W, x0, tmin, tmax, n_steps, interrogate_kramer, prior_pars,
                     obs_data, obs_times, obs_weight, obs_var, theta=theta)
    fsol, _ = fsolve(key, lorenz, W, x0, tmin, tmax, n_steps, interrogate_kramer, prior_pars,
                     obs_data, obs_times, obs_weight, obs_var, theta=theta)

    tseq_sim = np.linspace(tmin, tmax, n_steps + 1)
    exact = odeint(lorenz0, ode0, tseq_sim, args=(theta,), rtol=1e-12, atol=1e-12)
    between = (tseq_sim >= 7.5) & (np.arange(n_steps + 1) % n_res != 0)
    err_d = float(np.max(np.abs(dsol[between, :, 0] - exact[between])))
    err_f = float(np.max(np.abs(fsol[between, :, 0] - exact[between])))
    print(f"largest distance to odeint between the observations on 7.5 <= t <= 20: dalton.solve_mv {err_d:.3f}, "
          f"fenrir.solve_mv {err_f:.3f}")
    return {"dalton": err_d, "fenrir": err_f}


if __name__ == "__main__":
    main()
