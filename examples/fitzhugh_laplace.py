"""
The Laplace fit of docs/examples/parameter.md (FitzHugh-Nagumo: theta = (a, b, c) and x(0) from 41 noisy observations)
on this build, for the Fenrir and the DALTON likelihood, call for call where the names exist: ``fitz_fun``,
``fitz_logprior``, ``fitz_constrain_pars``, ``fitz_laplace``, ``neglogpost_fenrir`` / ``neglogpost_dalton``
(parameter.md:61-69, 186-275, 431-501).  What differs, and why:

* the log-posteriors are BATCHED: ``upars`` is (B, 5) and ``fenrir`` / ``dalton`` get ``ode_init`` (B, 2, 3) and ``theta``
  (B, 3) in one call; ``rodeo_amd.inference.laplace`` asks for the 51 points of a central-difference stencil at once, where
  the document has ``jaxopt`` and ``jax.jacfwd(jax.jacrev(.))`` call a scalar function;
* they return the log-posterior, not its negative (the driver maximises);
* the document optimises over seven numbers (the two prior scales ``sigma`` ride along with a flat prior) and keeps the
  5 x 5 block of the Hessian; here ``sigma`` stays at the value the data were simulated with, so k = 5;
* NumPy in place of jax.numpy, an integer seed in place of a PRNG key.

    python examples/fitzhugh_laplace.py            (needs an MI355X)
"""
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rodeo_amd as rodeo
from rodeo_amd.utils import first_order_pad
from rodeo_amd.inference import laplace as rlaplace


def fitz_fun(X, t, **params):
    # V' = c (V - V^3/3 + R),  R' = -(V - a + b R) / c;  X[:, 0] holds (V, R), the return value one row per variable
    a, b, c = params["theta"]
    V, R = X[:, 0]
    return np.array(
        [[c * (V - V * V * V / 3 + R)],
         [-1 / c * (V - a + b * R)]]
    )


n_vars = 2
n_deriv = 3
x0 = np.array([-1., 1.])
theta = np.array([.2, .2, 3])
W, fitz_init_pad = first_order_pad(fitz_fun, n_vars, n_deriv)
t_min = 0.
t_max = 40.
sigma = np.array([.1] * n_vars)
dt_obs = 1.
n_steps_obs = int((t_max - t_min) / dt_obs)
obs_times = np.linspace(t_min, t_max, num=n_steps_obs + 1)
n_res = 20
n_steps = n_steps_obs * n_res
sim_times = np.linspace(t_min, t_max, num=n_steps + 1)
dt_sim = (t_max - t_min) / n_steps
noise_sd = np.sqrt(0.005)
key = 100


def fitz_logprior(upars):
    # independent N(0, 10^2) densities on the five unconstrained numbers, summed per row: upars (B, 5) -> (B,)
    return np.sum(-0.5 * (upars / 10.) ** 2 - np.log(10.) - 0.5 * np.log(2 * np.pi), axis=1)


def fitz_constrain_pars(upars, dt):
    # rows of upars are (log a, log b, log c, V(0), R(0)): -> theta (B, 3), X0 (B, n_vars, n_deriv), the shared prior
    theta = np.exp(upars[:, :3])
    X0 = np.stack([fitz_init_pad(upars[b, 3:5], 0, theta=theta[b]) for b in range(len(upars))])
    prior_pars = rodeo.prior.ibm_init(dt=dt, n_deriv=n_deriv, sigma=sigma)
    return theta, X0, prior_pars


def fitz_laplace(key, logpost, n_samples, upars_init):
    # the fit, and its n_samples draws with theta mapped back through exp: (n_samples, 5).  max_iter is twice the
    # default: the curvature here reaches 1.5e6, so the absolute gtol of 1e-5 asks for the mode to about 1e-11 and the
    # last iterations work at the rounding of the log-density (the dalton fit took 41)
    fit = rlaplace.laplace(logpost, upars_init, max_iter=100, n_samples=n_samples, key=key)
    ode_sample = fit.samples.copy()
    ode_sample[:, :3] = np.exp(ode_sample[:, :3])
    return ode_sample, fit


def main(n_samples=100000):
    prior_pars = rodeo.prior.ibm_init(dt=dt_sim, n_deriv=n_deriv, sigma=sigma)
    X0 = fitz_init_pad(x0, 0, theta=theta)
    Xt, _ = rodeo.solve_mv(key=key, ode_fun=fitz_fun, ode_weight=W, ode_init=X0, t_min=t_min, t_max=t_max, theta=theta,
                           n_steps=n_steps, interrogate=rodeo.interrogate.interrogate_kramer, prior_pars=prior_pars)
    obs_ind = np.searchsorted(sim_times, obs_times)
    Y = Xt[obs_ind, :, 0] + noise_sd * np.random.default_rng(key).standard_normal((obs_times.size, 2))
    obs_data = np.expand_dims(Y, -1)
    obs_weight = np.zeros((len(obs_data), n_vars, 1, n_deriv)); obs_weight[:, :, :, 0] = 1
    obs_var = np.zeros((len(obs_data), n_vars, 1, 1)); obs_var[:] = noise_sd ** 2

    def logpost_for(loglik):
        def logpost(upars):
            theta, X0, prior_pars = fitz_constrain_pars(upars, dt_sim)
            ll = loglik(
                key=key,  # no draws are made: both likelihoods are deterministic with interrogate_kramer
                ode_fun=fitz_fun, ode_weight=W, ode_init=X0, t_min=t_min, t_max=t_max, theta=theta,
                n_steps=n_steps, interrogate=rodeo.interrogate.interrogate_kramer, prior_pars=prior_pars,
                obs_data=obs_data, obs_times=obs_times, obs_weight=obs_weight, obs_var=obs_var
            )
            return ll + fitz_logprior(upars)
        return logpost

    upars_init = np.append(np.log(theta), x0)
    out = {}
    for name, loglik in (("fenrir", rodeo.inference.fenrir), ("dalton", rodeo.inference.dalton)):
        post, fit = fitz_laplace(key, logpost_for(loglik), n_samples, upars_init)
        out[name] = fit
        print(f"{name}: converged {bool(fit.converged)} after {fit.n_iter} iterations, log-posterior {fit.logpost:.3f}, "
              f"log-evidence {fit.log_evidence:.3f}")
        print("   a, b, c, V(0), R(0): true    ", np.array2string(np.append(theta, x0), precision=3))
        print("   posterior mean of the draws  ", np.array2string(post.mean(axis=0), precision=3))
        print("   posterior sd of the draws    ", np.array2string(post.std(axis=0), precision=3))
    return out


if __name__ == "__main__":
    main()
