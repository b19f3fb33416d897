"""
TEST INFRASTRUCTURE.  NumPy restatement of ``rodeo_amd.solve_mv_at`` (the solver's posterior at arbitrary times), built from
the oracle's own scans and Kalman operators: ``oracle.scan.solve_filter`` / ``solve_mv`` for the moments on the grid,
``oracle.kalman_ops.predict`` / ``smooth_mv`` for the two steps between nodes.  Same signature as the product's function.

By the prior's Markov property the posterior at t in (t_n, t_n+1) is
    (mu_t, Sigma_t) = predict(filt[n]; prior_at(t - t_n))
    (mu', Sigma')   = predict((mu_t, Sigma_t); prior_at(t_n+1 - t))
    (mu, Sigma)     = smooth_mv(next = smooth[n+1], filt = (mu_t, Sigma_t), pred = (mu', Sigma'), wgt = Q(t_n+1 - t))
tests/test_oracle_eval_at.py pins this against dense joint-Gaussian conditioning over nodes and queries.
"""
import numpy as np
from oracle import kalman_ops, scan

NODE_TOL = 1e-10       # a time within this many steps of a node is that node
PRIOR_TOL = 1e-10      # Chapman-Kolmogorov residual, relative to the matrix's largest entry


def check_prior_at(prior_at, prior_pars, h1, h2):
    """Q(h2) Q(h1) = Q and Q(h2) R(h1) Q(h2)^T + R(h2) = R, each to PRIOR_TOL of the block matrix's largest entry; returns
    the two relative residuals, raises ValueError beyond the bar."""
    Q, R = (np.asarray(a, dtype=np.float64) for a in prior_pars)
    (Q1, R1), (Q2, R2) = prior_at(h1), prior_at(h2)
    res = []
    for got, want in ((Q2 @ Q1, Q), (Q2 @ R1 @ np.swapaxes(Q2, -1, -2) + R2, R)):
        rel = np.max(np.max(np.abs(got - want), axis=(-1, -2)) / np.max(np.abs(want), axis=(-1, -2)))
        if not rel <= PRIOR_TOL:
            raise ValueError(f"prior_at is inconsistent with prior_pars ({rel:.3e} of the largest entry)")
        res.append(float(rel))
    return tuple(res)


def solve_mv_at(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, t_eval, prior_at,
                kalman_type="standard", **params):
    if kalman_type != "standard":
        raise NotImplementedError
    t_eval = np.asarray(t_eval, dtype=np.float64)
    if t_eval.ndim != 1 or t_eval.size == 0 or not np.all(np.isfinite(t_eval)) or t_eval.min() < t_min or t_eval.max() > t_max:
        raise ValueError("t_eval: a non-empty vector of finite times in [t_min, t_max]")
    Q, R = prior_pars
    mf, vf = scan.solve_filter(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, Q, R,
                               **params)["state_filt"]
    ms, vs = scan.solve_mv(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, **params)
    squeeze = ms.ndim == 3
    if squeeze:
        mf, vf, ms, vs = mf[None], vf[None], ms[None], vs[None]
    N = int(n_steps)
    mean = np.empty((ms.shape[0], len(t_eval)) + ms.shape[2:])
    var = np.empty((vs.shape[0], len(t_eval)) + vs.shape[2:])
    for k, t in enumerate(t_eval):
        x = (t - t_min) / ((t_max - t_min) / N)
        if abs(x - round(x)) <= NODE_TOL:
            n = min(max(int(round(x)), 0), N)
            mean[:, k], var[:, k] = ms[:, n], vs[:, n]
            continue
        n = min(max(int(np.floor(x)), 0), N - 1)
        h1 = t - (t_min + (t_max - t_min) * n / N)
        h2 = (t_min + (t_max - t_min) * (n + 1) / N) - t
        check_prior_at(prior_at, prior_pars, h1, h2)
        (Q1, R1), (Q2, R2) = prior_at(h1), prior_at(h2)
        zero = np.zeros(mf.shape[2:])
        m_t, v_t = kalman_ops.predict(mean_state_past=mf[:, n], var_state_past=vf[:, n], mean_state=zero, wgt_state=Q1,
                                      var_state=R1)
        m_p, v_p = kalman_ops.predict(mean_state_past=m_t, var_state_past=v_t, mean_state=zero, wgt_state=Q2, var_state=R2)
        mean[:, k], var[:, k] = kalman_ops.smooth_mv(mean_state_next=ms[:, n + 1], var_state_next=vs[:, n + 1],
                                                     mean_state_filt=m_t, var_state_filt=v_t, mean_state_pred=m_p,
                                                     var_state_pred=v_p, wgt_state=Q2)
    return (mean[0], var[0]) if squeeze else (mean, var)
