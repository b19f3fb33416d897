"""
Test helper (not collected): NumPy restatement of the MAGI log-density (src/rodeo/inference/magi.py:6-99) for ONE item:
``ode_expand`` is called once, ``prior_pars`` are ((d, p, p), (d, p, p)), params unbatched.  Built on oracle.kalman_ops
(``"standard"``) and oracle.sqrt_ops (``"square-root"``, prior_pars[1] a lower factor) with
scipy.stats.multivariate_normal.logpdf as the density, block by block as the reference's vmap.
"""
import numpy as np
from scipy.stats import multivariate_normal
from oracle import kalman_ops, sqrt_ops


def magi_logdens(ode_data_subset, ode_expand, n_active, prior_pars, kalman_type, **params):
    if kalman_type == "standard":
        ops = kalman_ops
    elif kalman_type == "square-root":
        ops = sqrt_ops
    else:
        raise NotImplementedError
    n_vars = np.shape(ode_data_subset)[1]
    ode_state = np.asarray(ode_expand(ode_data_subset, **params), dtype=np.float64)
    n_deriv = ode_state.shape[2]
    wgt_meas = np.stack([np.eye(n_active, n_deriv)] * n_vars)
    mean_meas = np.zeros((n_vars, n_active))
    var_meas = np.zeros((n_vars, n_active, n_active))
    mean_state = np.zeros((n_vars, n_deriv))
    wgt_state, var_state = (np.asarray(a, dtype=np.float64) for a in prior_pars)
    mean, var = ode_state[0], np.zeros((n_vars, n_deriv, n_deriv))
    total = 0.0
    for x_meas in ode_state[1:, :, :n_active]:
        mp, vp = ops.predict(mean_state_past=mean, var_state_past=var, mean_state=mean_state, wgt_state=wgt_state,
                             var_state=var_state)
        mf, vf = ops.forecast(mean_state_pred=mp, var_state_pred=vp, mean_meas=mean_meas, wgt_meas=wgt_meas,
                              var_meas=var_meas)
        total += sum(multivariate_normal.logpdf(x_meas[k], mean=mf[k], cov=vf[k]) for k in range(n_vars))
        mean, var = ops.update(mean_state_pred=mp, var_state_pred=vp, x_meas=x_meas, mean_meas=mean_meas,
                               wgt_meas=wgt_meas, var_meas=var_meas)
    return float(total)


def exact_logdens(x_state, n_active, Q, R):
    """The same value from the joint Gaussian: log p(x_{1:N}[:, :, :n_active] | x_0) under X_n = Q X_{n-1} + N(0, R),
    built densely per block (x_state (N+1, d, p), Q / R (d, p, p) covariance form)."""
    N1, d, p = x_state.shape
    N = N1 - 1
    total = 0.0
    for k in range(d):
        # X_n = Q^n x_0 + sum_{m <= n} Q^{n-m} eps_m: mean and covariance of the stacked X_{1:N}
        powers = [np.eye(p)]
        for _ in range(N):
            powers.append(Q[k] @ powers[-1])
        mean = np.concatenate([powers[n] @ x_state[0, k] for n in range(1, N + 1)])
        cov = np.zeros((N * p, N * p))
        for i in range(1, N + 1):
            for j in range(1, N + 1):
                s = np.zeros((p, p))
                for m in range(1, min(i, j) + 1):
                    s += powers[i - m] @ R[k] @ powers[j - m].T
                cov[(i - 1) * p:i * p, (j - 1) * p:j * p] = s
        sel = np.concatenate([np.arange(n * p, n * p + n_active) for n in range(N)])
        y = x_state[1:, k, :n_active].reshape(-1)
        total += _chol_logpdf(y, mean[sel], cov[np.ix_(sel, sel)])
    return float(total)


def _chol_logpdf(x, mean, cov):
    """Gaussian log-density through a Cholesky factor (scipy's eigenvalue cut-off refuses the stacked IBM covariances)."""
    L = np.linalg.cholesky(cov)
    z = np.linalg.solve(L, x - mean)
    return -0.5 * z @ z - np.sum(np.log(np.diag(L))) - 0.5 * len(x) * np.log(2 * np.pi)


def random_prior(rng, d, p):
    """A random well-conditioned prior: Q near the identity, R = A A^T + p I scaled."""
    Q = np.stack([np.eye(p) + 0.1 * rng.standard_normal((p, p)) for _ in range(d)])
    R = []
    for _ in range(d):
        A = rng.standard_normal((p, p))
        R.append(0.1 * (A @ A.T + p * np.eye(p)))
    return Q, np.stack(R)


def stable_prior(rng, d, p):
    """Q diagonal (0.5 .. 0.95), R as in random_prior.  With a coupled Q and 1 < n_active < p, the standard form's filtered
    covariance (Sp - K W Sp, standard.py:93-102) loses its symmetry from step to step, by rounding that it amplifies: over
    hundreds of steps two correct restatements then part; a diagonal Q keeps it symmetric to rounding."""
    Q = np.stack([np.diag(rng.uniform(0.5, 0.95, p)) for _ in range(d)])
    return Q, random_prior(rng, d, p)[1]


def headline(B=1024, N=4000, d=2, p=3, seed=0):
    """The headline shape: B parameter sets over one path of a stable, well-conditioned prior whose first p - 1
    components are the data; ode_expand appends omega times the last data component (stable_prior)."""
    rng = np.random.default_rng(seed)
    Q, R = stable_prior(rng, d, p)
    x = np.zeros((N + 1, d, p))
    x[0] = rng.standard_normal((d, p))
    L = np.linalg.cholesky(R)
    for n in range(1, N + 1):
        x[n] = np.einsum("kij,kj->ki", Q, x[n - 1]) + np.einsum("kij,kj->ki", L, rng.standard_normal((d, p)))
    omega = np.linspace(0.8, 1.2, B)[:, None]

    def expand(u, omega):
        u = np.asarray(u)
        return np.concatenate([u, omega[0] * u[..., -1:]], axis=-1)

    return x[..., :p - 1], expand, omega, (Q, R)
