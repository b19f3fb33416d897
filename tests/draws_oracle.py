"""
``solve_sim_draws`` restated with the NumPy oracle (a helper, not collected): its law taken literally -- draw ``s`` is
``oracle.scan.solve_sim`` under the integer seed (seed + s) mod 2**64, restricted to the kept nodes.
"""
import numpy as np
from oracle import scan, odes, interrogations as oi

MASK = 0xFFFFFFFFFFFFFFFF

# ---- the statistical pin of the law (tests/test_oracle_draws.py on the oracle, tests/test_gpu_draws.py on the device) ----
# FitzHugh-Nagumo, n_bstate 3, N = 8, t_max = 0.2, kramer, key 7, 2048 draws: against solve_mv's posterior, every entry of
# every node >= 1 has its sample mean within PIN_Z sd / sqrt(S) and its sample variance over the smoothed variance within
# 1 +- PIN_Z sqrt(2 / (S - 1)) (the standard error of a normal sample's mean and variance).
PIN_KEY, PIN_DRAWS, PIN_Z = 7, 2048, 5.0
PIN_N, PIN_T_MAX, PIN_P = 8, 0.2, 3


def pin_problem(ra):
    """The pin's problem from the package's own helpers (``ra`` = rodeo_amd): arguments for the device and for the oracle."""
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, PIN_P)
    theta = np.array([0.2, 0.2, 3.0])
    x0 = init(np.array([-1.0, 1.0]), 0.0, theta=theta)
    prior = ra.ibm_init(PIN_T_MAX / PIN_N, PIN_P, np.array([0.5, 0.3]))
    return dict(W=W, x0=x0, prior=prior, theta=theta)


def pin_posterior(c):
    """solve_mv's mean (N+1, d, p) and marginal variances (N+1, d, p) of the pin's problem, from the oracle."""
    m, v = scan.solve_mv(None, odes.fitzhugh_nagumo, c["W"], c["x0"], 0.0, PIN_T_MAX, PIN_N, oi.interrogate_kramer, c["prior"],
                         theta=c["theta"])
    return m, np.einsum("...ii->...i", v)


def pin_statistics(x, mean, var):
    """(largest |z| of the sample means, smallest and largest variance ratio) over the nodes >= 1 of draws x (S, N+1, d, p)."""
    S = x.shape[0]
    z = (x[:, 1:].mean(axis=0) - mean[1:]) / np.sqrt(var[1:] / S)
    ratio = x[:, 1:].var(axis=0, ddof=1) / var[1:]
    return float(np.max(np.abs(z))), float(ratio.min()), float(ratio.max())


def pin_bounds(S=PIN_DRAWS):
    half = PIN_Z * np.sqrt(2.0 / (S - 1))
    return PIN_Z, 1.0 - half, 1.0 + half


def solve_sim_draws(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, n_draws=1, keep=None,
                    **params):
    """(n_draws, K, d, p), or (B, n_draws, K, d, p) for batched inputs; ``key`` an integer seed (None: 0)."""
    seed = 0 if key is None else int(key)
    rows = slice(None) if keep is None else np.asarray(keep, dtype=np.int64)
    paths = []
    for s in range(n_draws):
        x = scan.solve_sim((seed + s) & MASK, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                           **params)
        paths.append(x[..., rows, :, :])                             # (K, d, p) or (B, K, d, p)
    return np.stack(paths, axis=-4)
