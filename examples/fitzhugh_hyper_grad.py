"""
The two hyperparameters a user cannot read off the problem -- the prior scale sigma of the solver and the noise variance of the
data -- on the quick start's FitzHugh-Nagumo problem with ten observations, through ``fenrir_grad``'s two reserved names:

* ``wrt=(..., "log_sigma", "log_obs_var")``: the derivative of Fenrir's log p(Y | Z) in log sigma_b (both blocks' prior scales) and
  in a common log-scale of each block's observation variances, printed next to central differences of ``fenrir`` (sigma moved
  through ``ibm_init``, the variances through ``obs_var``);
* ``laplace_grad`` over seven unconstrained numbers, (log a, log b, log c, V(0), R(0), log s, log w) with sigma = s sigma_0 and
  obs_var = w obs_var_0: examples/fitzhugh_laplace_grad.py's chain rule with two more columns.  ``fenrir_grad`` takes one
  ``obs_var`` a call, so the rows of a stencil are grouped by w.

Whether the seven-parameter fit converges from the true values depends on the data; what happens is printed, nothing is asserted.

    python examples/fitzhugh_hyper_grad.py            (needs an MI355X)
"""
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rodeo_amd as rodeo
from rodeo_amd.inference import laplace as rlaplace
from rodeo_amd.inference.fenrir import fenrir_grad
import fitzhugh_laplace as base
from fitzhugh_laplace import fitz_fun, W, x0, theta, t_min, t_max, n_steps, n_vars, n_deriv, dt_sim, key
from fitzhugh_laplace_grad import fitz_init_jac, fitz_init_dv0, make_data

WRT = ("theta", "ode_init", "log_sigma", "log_obs_var")


def ten_observations():
    data = make_data()
    keep = np.arange(0, 40, 4)                                           # ten of the quick start's 41
    return {name: v[keep] for name, v in data.items()}


def call(fn, th, X0, sigma, data, w=1.0, **more):
    prior_pars = rodeo.prior.ibm_init(dt=dt_sim, n_deriv=n_deriv, sigma=sigma)
    return fn(key=key, ode_fun=fitz_fun, ode_weight=W, ode_init=X0, t_min=t_min, t_max=t_max, theta=th, n_steps=n_steps,
              interrogate=rodeo.interrogate.interrogate_kramer, prior_pars=prior_pars,
              **dict(data, obs_var=w * data["obs_var"]), **more)


def logprior(upars):
    return np.sum(-0.5 * (upars / 10.) ** 2 - np.log(10.) - 0.5 * np.log(2 * np.pi), axis=1)


def value_and_grad_for(data):
    def value_and_grad(upars):
        B = len(upars)
        th, v0, s, w = np.exp(upars[:, :3]), upars[:, 3:5], np.exp(upars[:, 5]), np.exp(upars[:, 6])
        X0 = np.stack([base.fitz_init_pad(v0[b], 0, theta=th[b]) for b in range(B)])
        J = fitz_init_jac(v0, th)
        value = np.zeros(B)
        grad = dict(theta=np.zeros((B, 3)), ode_init=np.zeros((B, n_vars, n_deriv)), log_sigma=np.zeros((B, n_vars)),
                    log_obs_var=np.zeros((B, n_vars)))
        for wv in np.unique(w):                                          # one obs_var a call
            rows = np.flatnonzero(w == wv)
            res = call(fenrir_grad, th[rows], X0[rows], s[rows, None] * base.sigma, data, wv, wrt=WRT, init_jac=dict(theta=J[rows]))
            value[rows] = res.value
            for name in grad:
                grad[name][rows] = res.grad[name]
        d_theta = np.zeros((B, 3, 7))
        d_theta[:, np.arange(3), np.arange(3)] = th                      # d theta / d log theta
        d_x0 = np.zeros((B, n_vars, n_deriv, 7))
        d_x0[..., 3:5] = fitz_init_dv0(v0, th)
        d_s, d_w = np.zeros((B, n_vars, 7)), np.zeros((B, n_vars, 7))
        d_s[:, :, 5] = d_w[:, :, 6] = 1.0                                # both blocks share log s and log w
        g = rlaplace.pull_back(grad, dict(theta=d_theta, ode_init=d_x0, log_sigma=d_s, log_obs_var=d_w)) - upars / 10. ** 2
        return value + logprior(upars), g
    return value_and_grad


def main(n_samples=10000):
    data = ten_observations()
    X0 = base.fitz_init_pad(x0, 0, theta=theta)
    res = call(fenrir_grad, theta, X0, base.sigma, data, wrt=("log_sigma", "log_obs_var"))
    print(f"fenrir_grad with ten observations: value {res.value:.6f}")
    h = 1e-3
    for name in ("log_sigma", "log_obs_var"):
        est = np.zeros(n_vars)
        for b in range(n_vars):
            e = np.eye(n_vars)[b] * h
            if name == "log_sigma":
                f = [call(rodeo.inference.fenrir, theta, X0, base.sigma * np.exp(s * e), data) for s in (1, -1)]
            else:
                scaled = [dict(data, obs_var=data["obs_var"] * np.exp(s * e)[None, :, None, None]) for s in (1, -1)]
                f = [call(rodeo.inference.fenrir, theta, X0, base.sigma, dd) for dd in scaled]
            est[b] = (f[0] - f[1]) / (2 * h)
        print(f"  d / d {name:<11}: device {np.array2string(res.grad[name], precision=6)}   central differences (h = {h:g}) "
              f"{np.array2string(est, precision=6)}")
    vg = value_and_grad_for(data)
    start = np.concatenate([np.log(theta), x0, [0.0, 0.0]])
    try:
        fit = rlaplace.laplace_grad(vg, start, max_iter=100, n_samples=n_samples, key=key)
    except ValueError as err:                                            # (the gradient test, or a Hessian that is not negative definite)
        print("laplace_grad over (log theta, x(0), log s, log w) raised:", err)
        return None
    post = fit.samples.copy()
    post[:, [0, 1, 2, 5, 6]] = np.exp(post[:, [0, 1, 2, 5, 6]])
    print(f"laplace_grad over (log theta, x(0), log s, log w): converged {bool(fit.converged)} after {fit.n_iter} iterations, "
          f"log-posterior {fit.logpost:.6f}, n_bad {int(fit.n_bad)}")
    print("   a, b, c, V(0), R(0), s, w: true   ", np.array2string(np.concatenate([theta, x0, [1.0, 1.0]]), precision=3))
    print("   mode                              ", np.array2string(np.concatenate([np.exp(fit.mode[:3]), fit.mode[3:5], np.exp(fit.mode[5:])]),
                                                                precision=4))
    print("   posterior mean of the draws       ", np.array2string(post.mean(axis=0), precision=4))
    print("   posterior sd of the draws         ", np.array2string(post.std(axis=0), precision=4))
    return fit


if __name__ == "__main__":
    main()
