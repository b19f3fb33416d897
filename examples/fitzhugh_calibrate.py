"""
Calibrating the prior scale sigma of the quick start (FitzHugh-Nagumo, theta = (0.2, 0.2, 3), x0 = (-1, 1), n_deriv = 3,
72 steps on [0, 4], interrogate_kramer) from the solver's own marginal likelihood, ``rodeo_amd.solve_evidence``:
log p(Z_{1:N} = 0) under the prior, and from its per-block parts the scale c = quad / N that maximises it in closed form
(``evidence_scale``; sigma_hat = sigma * sqrt(c)), from one forward pass.  Every variance that ``solve_mv`` reports scales with
sigma^2, so the posterior standard deviation at t_max is printed under both.

    python examples/fitzhugh_calibrate.py            (needs an MI355X)
"""
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rodeo_amd as rodeo


def main(sigma=(0.5, 0.3)):
    n_vars, n_deriv = 2, 3
    theta = np.array([.2, .2, 3])
    W, fitz_init_pad = rodeo.utils.first_order_pad(rodeo.ode.fitzhugh_nagumo, n_vars, n_deriv)
    X0 = fitz_init_pad(np.array([-1., 1.]), 0., theta=theta)
    t_min, t_max, n_steps = 0., 4., 72
    dt = (t_max - t_min) / n_steps
    sigma = np.asarray(sigma, dtype=float)

    def run(sig):
        prior_pars = rodeo.prior.ibm_init(dt=dt, n_deriv=n_deriv, sigma=sig)
        args = (rodeo.ode.fitzhugh_nagumo, W, X0, t_min, t_max, n_steps, rodeo.interrogate.interrogate_kramer, prior_pars)
        ev = rodeo.solve_evidence(None, *args, theta=theta)
        _, var = rodeo.solve_mv(None, *args, theta=theta)
        return ev, np.sqrt(var[-1, :, 0, 0])

    ev, sd = run(sigma)
    c = rodeo.evidence_scale(ev)                                    # mean normalised squared innovation per block; 1 if calibrated
    print(f"sigma     = {sigma}: quad / N = {c}, log p(Z = 0) = {ev.logdens:.2f}, sd at t_max = {sd}")
    print(f"            evidence_at predicts {rodeo.evidence_at(ev, c):.2f} after rescaling")
    sigma_hat = sigma * np.sqrt(c)                                  # the two-line rescaling
    ev2, sd2 = run(sigma_hat)
    print(f"sigma_hat = {sigma_hat}: quad / N = {rodeo.evidence_scale(ev2)}, log p(Z = 0) = {ev2.logdens:.2f}, sd at t_max = {sd2}")
    return ev, ev2


if __name__ == "__main__":
    main()
