"""
The quick start (FitzHugh-Nagumo, theta = (0.2, 0.2, 3), x0 = (-1, 1), n_deriv = 3, 72 steps on [0, 4], interrogate_kramer)
run three ways: ``solve_mv`` with the made-up sigma, ``solve_mv`` after one calibration by ``evidence_scale`` (one scale per
block for the whole horizon), and ``solve_mv_dynamic`` (one scale per block and step, estimated at that step before its
update).  Prints the posterior standard deviation of both variables at a few times and the three log-evidences; the range of
the per-step scales shows why one constant is too wide on the slow branch and too narrow at the spike.

    python examples/fitzhugh_dynamic.py            (needs an MI355X)
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
    at = [1, 9, 18, 36, 54, 72]                                     # nodes whose sd is printed

    def args(sig):
        prior_pars = rodeo.prior.ibm_init(dt=dt, n_deriv=n_deriv, sigma=sig)
        return (rodeo.ode.fitzhugh_nagumo, W, X0, t_min, t_max, n_steps, rodeo.interrogate.interrogate_kramer, prior_pars)

    def show(label, var, logdens):
        sd = np.sqrt(var[at][:, :, 0, 0])
        print(f"{label}: log p(Z = 0) = {logdens:.2f}")
        for n, row in zip(at, sd):
            print(f"    t = {t_min + dt * n:5.2f}: sd = ({row[0]:.3e}, {row[1]:.3e})")

    ev = rodeo.solve_evidence(None, *args(sigma), theta=theta)
    _, var = rodeo.solve_mv(None, *args(sigma), theta=theta)
    show(f"solve_mv, sigma = {sigma}", var, ev.logdens)
    sigma_hat = sigma * np.sqrt(rodeo.evidence_scale(ev))
    ev2 = rodeo.solve_evidence(None, *args(sigma_hat), theta=theta)
    _, var2 = rodeo.solve_mv(None, *args(sigma_hat), theta=theta)
    show(f"solve_mv, sigma_hat = {sigma_hat} (evidence_scale)", var2, ev2.logdens)
    dyn = rodeo.solve_mv_dynamic(None, *args(sigma), theta=theta)
    show("solve_mv_dynamic (any sigma)", dyn.var, dyn.logdens)
    root = sigma * np.sqrt(dyn.scale)                               # the sigma each step used
    print(f"    per-step sigma: {root.min(axis=0)} .. {root.max(axis=0)}; scale max / min per block = "
          f"{dyn.scale.max(axis=0) / dyn.scale.min(axis=0)}")
    return ev, ev2, dyn


if __name__ == "__main__":
    main()
