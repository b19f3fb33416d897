"""
The quick-start problem with ten noisy observations at irregular times, put into the grid by ``grid_with_times``:
``fenrir_grid_grad`` (Fenrir's log-likelihood, the one the reference's documentation fits parameters with) with respect to theta
and to the two initial values next to central differences of ``fenrir_grid`` (step 1e-5 max(1, |x|)), then a few steps of gradient ascent on theta from a wrong start, where the initial state
``init(v0, t, theta)`` depends on theta and ``init_jac`` makes the gradient the total derivative.  The script prints the numbers; it
asserts nothing about them.

    python examples/fitzhugh_fenrir_grad.py          (needs an MI355X)
"""
import os
import sys
import numpy as np
from scipy.integrate import odeint
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rodeo_amd as rodeo
from rodeo_amd.inference.fenrir import fenrir_grid, fenrir_grid_grad


def init_jac(v0, theta, n_deriv):
    """d init(v0, t, theta) / d theta (n_vars, n_deriv, 3): the first derivative of the padded state is f(v0, theta)."""
    (a, b, c), (V, R) = theta, v0
    J = np.zeros((2, n_deriv, 3))
    J[0, 1, 2] = V - V ** 3 / 3 + R
    J[1, 1] = [1 / c, -R / c, (V - a + b * R) / c ** 2]
    return J


def main():
    n_vars, n_deriv = 2, 3
    v0 = np.array([-1., 1.])
    theta = np.array([.2, .2, 3])
    W, fitz_init_pad = rodeo.utils.first_order_pad(rodeo.ode.fitzhugh_nagumo, n_vars, n_deriv)
    t_min, t_max, n_steps = 0., 10., 100
    sigma = np.array([.1] * n_vars)
    rng = np.random.default_rng(0)
    obs_times = np.sort(rng.uniform(0.5, 9.5, 10))
    exact = odeint(lambda X, t: [theta[2] * (X[0] - X[0] ** 3 / 3 + X[1]), -(X[0] - theta[0] + theta[1] * X[1]) / theta[2]],
                   v0, np.concatenate([[t_min], obs_times]), rtol=1e-10, atol=1e-10)[1:]
    noise_sd = 0.05
    obs_data = (exact + noise_sd * rng.standard_normal(exact.shape))[:, :, None]
    obs_weight = np.zeros((len(obs_times), n_vars, 1, n_deriv))
    obs_weight[..., 0] = 1.0
    obs_var = np.full((len(obs_times), n_vars, 1, 1), noise_sd ** 2)
    itg = rodeo.interrogate.interrogate_kramer
    t_grid, _ = rodeo.grid_with_times(np.linspace(t_min, t_max, n_steps + 1), obs_times)

    def prior_at(h):
        return rodeo.prior.ibm_init(dt=h, n_deriv=n_deriv, sigma=sigma)

    def call(fn, X0, th, **kw):
        return fn(None, rodeo.ode.fitzhugh_nagumo, W, X0, t_grid, itg, prior_at, obs_data, obs_times, obs_weight, obs_var, theta=th, **kw)

    # the partial derivatives, ode_init held fixed, next to central differences
    X0 = fitz_init_pad(v0, 0., theta=theta)
    res = call(fenrir_grid_grad, X0, theta, wrt=("theta", "ode_init"))
    print(f"{len(t_grid)} nodes ({len(rodeo.grid_slots(t_grid)[0])} slots); fenrir_grid = {res.value:.6f}")
    print("   derivative in        fenrir_grid_grad    central difference")
    fd = {}
    for j, name in enumerate("abc"):
        h = 1e-5 * max(1.0, abs(theta[j]))
        e = np.eye(3)[j] * h
        fd[name] = (call(fenrir_grid, X0, theta + e) - call(fenrir_grid, X0, theta - e)) / (2 * h)
        print(f"   theta {name}           {res.grad['theta'][j]:18.6f}  {fd[name]:18.6f}")
    for b, name in enumerate(("V(0)", "R(0)")):
        h = 1e-5 * max(1.0, abs(v0[b]))
        e = np.zeros_like(X0)
        e[b, 0] = h
        fd[name] = (call(fenrir_grid, X0 + e, theta) - call(fenrir_grid, X0 - e, theta)) / (2 * h)
        print(f"   {name}              {res.grad['ode_init'][b, 0]:18.6f}  {fd[name]:18.6f}")

    # gradient ascent on theta from a wrong start; the initial state is rebuilt from theta, init_jac gives the total derivative
    th = theta * np.array([1.3, 0.7, 0.9])
    print("   gradient ascent on theta (normalised steps), init_jac = d init / d theta:")
    path = []
    for step in range(8):
        r = call(fenrir_grid_grad, fitz_init_pad(v0, 0., theta=th), th, wrt=("theta",), init_jac=dict(theta=init_jac(v0, th, n_deriv)))
        path.append((th.copy(), r.value))
        print(f"   step {step}: theta = {np.round(th, 4)}, fenrir_grid = {r.value:10.4f}, |grad| = {np.linalg.norm(r.grad['theta']):.3e}")
        th = th + 0.02 * r.grad["theta"] / np.linalg.norm(r.grad["theta"])
    return dict(value=res.value, grad=res.grad, differences=fd, path=path)


if __name__ == "__main__":
    main()
