"""
The last section of docs/examples/parameter.md (:525-591) on this build: FitzHugh-Nagumo observed through Poisson counts
Y_ij ~ Poisson(exp(b0 + b1 x_j(t_i))), b0 = 0.1, b1 = 0.5, fitted by ``daltonng`` under the Laplace approximation, call for call
where the names exist: ``obs_loglik_i``, ``neglogpost_daltonng`` (here ``logpost_daltonng``), ``fitz_laplace``.  Everything up to
the data is examples/fitzhugh_laplace.py's; what differs from the document, beyond what that file lists:

* ``daltonng`` is imported from ``rodeo_amd.inference.dalton`` (the package does not re-export it);
* ``obs_loglik_i`` is written with NumPy and ``rodeo_amd.trace.gammaln``: the Poisson log-pmf y eta - exp(eta) - log y! spelled
  out, where the document calls ``jax.scipy.stats.poisson.logpmf``.  It is traced once into device code and differentiated
  there, so b0 and b1 are constants of the compiled model;
* the counts are drawn with a seeded NumPy generator (JAX's stream cannot be reproduced);
* as in fitzhugh_laplace.py, ``sigma`` stays fixed, so the document's two extra entries of ``upars_init`` are absent (k = 5).

Counts with rates between 0.4 and 3 say little about b: the fit leaves log b at its prior's width.

    python examples/fitzhugh_daltonng.py            (needs an MI355X)
"""
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rodeo_amd as rodeo
from rodeo_amd.inference.dalton import daltonng
from rodeo_amd.trace import gammaln
from fitzhugh_laplace import (fitz_fun, fitz_logprior, fitz_constrain_pars, fitz_laplace, fitz_init_pad, W, x0, theta, t_min,
                              t_max, n_steps, obs_times, sim_times, dt_sim, n_deriv, sigma, key)

b0 = 0.1
b1 = 0.5


def obs_loglik_i(obs_data_i, ode_data_i, ind, **params):
    # log Poisson(y; exp(eta)) summed over the variables, eta = b0 + b1 x_j(t_i): reads X[:, 0] only
    eta = b0 + b1 * ode_data_i[:, 0]
    y = obs_data_i.flatten()
    return np.sum(y * eta - np.exp(eta) - gammaln(y + 1.0))


def main(n_samples=100000):
    prior_pars = rodeo.prior.ibm_init(dt=dt_sim, n_deriv=n_deriv, sigma=sigma)
    X0 = fitz_init_pad(x0, 0, theta=theta)
    Xt, _ = rodeo.solve_mv(key=key, ode_fun=fitz_fun, ode_weight=W, ode_init=X0, t_min=t_min, t_max=t_max, theta=theta,
                           n_steps=n_steps, interrogate=rodeo.interrogate.interrogate_kramer, prior_pars=prior_pars)
    x = Xt[np.searchsorted(sim_times, obs_times), :, 0]
    Yt = np.random.default_rng(key).poisson(lam=np.exp(b0 + b1 * x)).astype(np.float64)
    obs_data = np.expand_dims(Yt, -1)

    def logpost_daltonng(upars):
        theta, X0, prior_pars = fitz_constrain_pars(upars, dt_sim)
        ll = daltonng(
            key=key,  # immaterial, since not used
            ode_fun=fitz_fun, ode_weight=W, ode_init=X0, t_min=t_min, t_max=t_max, theta=theta,
            n_steps=n_steps, interrogate=rodeo.interrogate.interrogate_kramer, prior_pars=prior_pars,
            obs_data=obs_data, obs_times=obs_times, obs_loglik_i=obs_loglik_i
        )
        return ll + fitz_logprior(upars)

    upars_init = np.append(np.log(theta), x0)
    post, fit = fitz_laplace(key, logpost_daltonng, n_samples, upars_init)
    print(f"daltonng: converged {bool(fit.converged)} after {fit.n_iter} iterations, log-posterior {fit.logpost:.3f}, "
          f"log-evidence {fit.log_evidence:.3f}")
    print("   a, b, c, V(0), R(0): true    ", np.array2string(np.append(theta, x0), precision=3))
    print("   posterior mean of the draws  ", np.array2string(post.mean(axis=0), precision=3))
    print("   posterior sd of the draws    ", np.array2string(post.std(axis=0), precision=3))
    return fit


if __name__ == "__main__":
    main()
