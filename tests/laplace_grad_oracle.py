"""
TEST INFRASTRUCTURE: NumPy restatement of the two device pieces of ``laplace_grad`` (csrc/laplace_kernels.hpp,
fd_grad_stencil_kernel and fd_hess_from_grad_kernel) with their order of operations, and a stand-in for
``rodeo_amd.inference.laplace.DeviceGradSteps`` built from them, so that the driver runs without a GPU.  ``pairs``,
``newton_step`` and ``quadratic`` are tests/laplace_oracle.py's.  float64 throughout; nothing here is imported by the product.
"""
import numpy as np
from laplace_oracle import pairs, newton_step, quadratic  # noqa: F401  (quadratic is re-exported for the tests)


def n_stencil_grad(k):
    return 2 * k + 1


def grad_stencil(u, step):
    """u (C, k), step (k,) -> (C, 2 k + 1, k): u;  u +- h_i e_i (i ascending, + first)."""
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    n_c, k = u.shape
    out = np.repeat(u[:, None, :], n_stencil_grad(k), axis=1)
    for i in range(k):
        out[:, 1 + 2 * i, i] += step[i]
        out[:, 2 + 2 * i, i] -= step[i]
    return out


def hess_from_grad(vals, grads, step):
    """vals (C, S), grads (C, S, k), step (k,) -> grad (C, k), hess (C, k, k), n_bad (C,), grad_fd (C, k), with the device's
    order of operations."""
    vals, grads = np.asarray(vals, dtype=np.float64), np.asarray(grads, dtype=np.float64)
    n_c, S = vals.shape
    k = len(step)
    assert S == n_stencil_grad(k) and grads.shape == (n_c, S, k)
    grad, hess, grad_fd = grads[:, 0].copy(), np.empty((n_c, k, k)), np.empty((n_c, k))
    with np.errstate(invalid="ignore"):
        for i in range(k):
            hess[:, i, i] = (grads[:, 1 + 2 * i, i] - grads[:, 2 + 2 * i, i]) / (2.0 * step[i])
            grad_fd[:, i] = (vals[:, 1 + 2 * i] - vals[:, 2 + 2 * i]) / (2.0 * step[i])
        for a, b in pairs(k):
            da = (grads[:, 1 + 2 * a, b] - grads[:, 2 + 2 * a, b]) / (2.0 * step[a])
            db = (grads[:, 1 + 2 * b, a] - grads[:, 2 + 2 * b, a]) / (2.0 * step[b])
            hess[:, a, b] = 0.5 * (da + db)
            hess[:, b, a] = hess[:, a, b]
    n_bad = np.sum(~np.isfinite(vals), axis=1) + np.sum(~np.isfinite(grads), axis=(1, 2))
    grad[n_bad > 0] = np.nan
    hess[n_bad > 0] = np.nan
    grad_fd[n_bad > 0] = np.nan
    return grad, hess, n_bad, grad_fd


def quadratic_vg(k, n_c, seed):
    """``quadratic`` with its exact gradient: (A, m, c0, starts, value_and_grad), gradient -A (u - m)."""
    A, m, c0, starts, logpost = quadratic(k, n_c, seed)

    def value_and_grad(u):
        return logpost(u), -(np.asarray(u) - m) @ A
    return A, m, c0, starts, value_and_grad


class HostGradSteps:
    """What ``DeviceGradSteps`` does, from the restatement: the driver under test runs on it without a device."""

    def __init__(self, n_c, k, h):
        self.n_c, self.k, self.S, self.h = n_c, k, n_stencil_grad(k), np.asarray(h, dtype=np.float64)

    def grad_stencil(self, u):
        return grad_stencil(u, self.h).reshape(self.n_c * self.S, self.k)

    def hess_from_grad(self, vals, grads):
        return hess_from_grad(vals.reshape(self.n_c, self.S), grads.reshape(self.n_c, self.S, self.k), self.h)

    def newton(self, grad, hess, damping):
        return newton_step(grad, hess, damping)


# ---- the FitzHugh-Nagumo case of tests/test_laplace_grad_host.py and tests/test_gpu_laplace_grad.py ------------------------------
# theta = (a, b, c) and x(0) = (V, R) from noisy observations of both variables, u = (log theta, x(0)), k = 5; p = 3, kramer,
# N(0, 10^2) priors on u as in examples/fitzhugh_laplace.py.  The log-likelihood and its gradient come from a BACKEND with
# ``fenrir_grad``'s contract -- backend(X0 (B, 2, 3), theta (B, 3), init_jac (B, 2, 3, 3) or None) -> (value (B,), {"theta": (B, 3),
# "ode_init": (B, 2, 3)}) -- so that the host test (tests/fenrir_grad_oracle.py) and the GPU test (``fenrir_grad`` /
# ``dalton_grad``) run the same chain rule through ``pull_back``.

def fhn_case(N, t_max, n_obs, seed=1):
    import rodeo_amd as ra
    from oracle import scan, odes, interrogations as oi
    p, theta, x0 = 3, np.array([0.2, 0.2, 3.0]), np.array([-1.0, 1.0])
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    prior = ra.ibm_init(t_max / N, p, np.array([0.1, 0.1]))
    assert N % (n_obs - 1) == 0
    t = np.linspace(0.0, t_max, N + 1)
    nodes = np.arange(n_obs) * (N // (n_obs - 1))
    X, _ = scan.solve_mv(None, odes.fitzhugh_nagumo, W, init(x0, 0.0, theta=theta), 0.0, t_max, N, oi.interrogate_kramer, prior,
                         theta=theta)
    noise_sd = np.sqrt(0.005)
    y = (X[nodes, :, 0] + noise_sd * np.random.default_rng(seed).standard_normal((n_obs, 2)))[:, :, None]
    ow = np.zeros((n_obs, 2, 1, p)); ow[..., 0] = 1.0
    ov = np.full((n_obs, 2, 1, 1), noise_sd ** 2)
    return dict(N=N, t_max=t_max, p=p, W=W, init=init, prior=prior, t=t, nodes=nodes, obs_times=t[nodes], y=y, ow=ow, ov=ov,
                theta=theta, x0=x0, start=np.concatenate([np.log(theta), x0]) + 0.05)


def fhn_oracle_backend(case):
    """``fenrir_grad``'s contract on tests/fenrir_grad_oracle.py: nine directions (theta, then ode_init row-major) a trajectory."""
    import fenrir_grad_oracle as fgr
    from oracle import odes
    c = case

    def backend(X0, th, init_jac):
        B = len(th)
        dth = np.concatenate([np.eye(3), np.zeros((6, 3))])
        dx = np.zeros((B, 9, 2, 3))
        dx[:, 3:] = np.eye(6).reshape(6, 2, 3)
        if init_jac is not None:
            dx[:, :3] = np.moveaxis(init_jac, -1, 1)
        value, dvalue = fgr.fenrir_grid_jvp(odes.fitzhugh_nagumo, c["W"], X0, c["t"], "kramer", lambda dt: c["prior"], c["y"],
                                            c["nodes"], c["ow"], c["ov"], th, dtheta=dth, dx0=dx)
        return value, dict(theta=dvalue[:, :3], ode_init=dvalue[:, 3:].reshape(B, 2, 3))
    return backend


def fhn_value_and_grad(case, backend, chain="exact"):
    """The log-posterior and its gradient in u.  ``chain``: "exact"; "no_theta_factor" leaves the factor theta of d / d log theta
    out; "no_init_jac" leaves out the dependence of init(v0, t, theta) on theta."""
    from rodeo_amd.inference.laplace import pull_back
    import fenrir_grad_oracle as fgr
    init, p = case["init"], case["p"]

    def value_and_grad(u):
        B = len(u)
        th, v0 = np.exp(u[:, :3]), u[:, 3:5]
        X0 = np.stack([init(v0[b], 0.0, theta=th[b]) for b in range(B)])
        J = np.stack([fgr.fhn_init_jac(v0[b], th[b], p) for b in range(B)])                     # d x0 / d theta (B, 2, p, 3)
        value, grad = backend(X0, th, None if chain == "no_init_jac" else J)
        d_theta = np.zeros((B, 3, 5))                                                            # d theta / d u
        d_theta[:, np.arange(3), np.arange(3)] = 1.0 if chain == "no_theta_factor" else th
        d_x0 = np.zeros((B, 2, p, 5))                                                            # d x0 / d v0 at fixed theta
        V, (a, b_, c) = v0[:, 0], th.T
        d_x0[:, 0, 0, 3], d_x0[:, 0, 1, 3], d_x0[:, 1, 1, 3] = 1.0, c * (1 - V * V), -1.0 / c
        d_x0[:, 1, 0, 4], d_x0[:, 0, 1, 4], d_x0[:, 1, 1, 4] = 1.0, c, -b_ / c
        g = pull_back(grad, dict(theta=d_theta, ode_init=d_x0)) - u / 100.0
        return value + np.sum(-0.5 * (u / 10.0) ** 2 - np.log(10.0) - 0.5 * np.log(2 * np.pi), axis=1), g
    return value_and_grad
