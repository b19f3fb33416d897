"""
Test helper (not collected): NumPy restatement of DALTON for non-Gaussian observations (src/rodeo/inference/dalton.py:550-1039)
for ONE trajectory, on oracle.kalman_ops and oracle.fenrir.multivariate_normal_logpdf.

The log-likelihood comes with hand-written derivatives: ``loglik(y_i, X, i, **params)`` -> float, ``grad(...)`` -> (d, p) and
``hess(...)`` -> (d, p, p), the diagonal blocks of the Hessian (dalton.py:618 keeps nothing else).

Two forms:
  * the repaired one (default, what the device builds): with ``active[b]`` the state components of block b
    that the log-likelihood reads, yhat_b = mu-[A_b] + V g_A, V = (-H_AA)^{-1}, weight = the selector of A_b, in the stacked
    update [W~; D_b] of dalton.py:630-643; -H_AA that is not positive definite gives NaN;
  * ``literal=True``: the reference's text as written -- the (p x p) 0/1 pattern of -pinv(H_b) as weight, ``obs_weight[i]`` with
    the OBSERVATION index (clamped like a JAX out-of-range read) in yhat, the stacked update through numpy.linalg.solve.  It may
    return non-finite values or raise numpy.linalg.LinAlgError.
"""
import numpy as np
from oracle import kalman_ops as ko
from oracle.fenrir import multivariate_normal_logpdf
from dalton_oracle import _grid_index, _step


def _pseudo_obs(mp, y_i, i, grad, hess, active, literal, params):
    """Per block: (weight (m, p), datum (m,), variance (m, m)) of the pseudo-observation at the predicted mean mp (d, p)."""
    d, p = mp.shape
    g, H = np.asarray(grad(y_i, mp, i, **params), dtype=np.float64), np.asarray(hess(y_i, mp, i, **params), dtype=np.float64)
    out = []
    if literal:
        var = np.stack([-np.linalg.pinv(H[b]) for b in range(d)])                   # dalton.py:618
        wgt = np.where(var != 0, 1.0, 0.0)                                          # :619
        for b in range(d):
            yhat = wgt[min(i, d - 1)] @ mp[b] + var[b] @ g[b]                        # :621 (obs_weight[i], clamped)
            out.append((wgt[b], yhat, var[b]))
        return out
    for b in range(d):
        A = list(active[b])
        if not A:
            out.append(None)
            continue
        nH = -H[b][np.ix_(A, A)]
        ok = np.all(np.isfinite(nH)) and np.all(np.linalg.eigvalsh(0.5 * (nH + nH.T)) > 0)
        V = np.linalg.inv(nH) if ok else np.full((len(A), len(A)), np.nan)
        D = np.zeros((len(A), p))
        D[np.arange(len(A)), A] = 1.0
        out.append((D, mp[b][A] + V @ g[b][A], V))
    return out


def solve_filter_nn(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, obs_data, obs_times,
                    loglik, grad, hess, active=None, literal=False, **params):
    """dalton.py:550-698: (predicted (mean, var), filtered (mean, var)), each (N+1, d, p[, p]), index 0 = (ode_init, 0)."""
    W = np.asarray(ode_weight, dtype=np.float64)
    x0 = np.asarray(ode_init, dtype=np.float64)
    Q, R = (np.asarray(a, dtype=np.float64) for a in prior_pars)
    obs_data = np.asarray(obs_data, dtype=np.float64)
    d, nm, p = W.shape
    ind = _grid_index(t_min, t_max, n_steps, obs_times)
    n_obs = len(ind)
    i = 1 if n_obs and ind[0] == 0 else 0
    mp_, vp_ = np.zeros((n_steps + 1, d, p)), np.zeros((n_steps + 1, d, p, p))
    mf_, vf_ = np.zeros((n_steps + 1, d, p)), np.zeros((n_steps + 1, d, p, p))
    mp_[0] = mf_[0] = x0
    m, v = x0.copy(), np.zeros((d, p, p))
    for n in range(n_steps):
        t = t_min + (t_max - t_min) * (n + 1) / n_steps
        mp, vp, Wm, mm, vm = _step(ode_fun, W, interrogate, t, m, v, Q, R, params)
        if i < n_obs and n + 1 == ind[i]:
            po = _pseudo_obs(mp, obs_data[i], i, grad, hess, active, literal, params)
            m, v = np.empty_like(mp), np.empty_like(vp)
            for b in range(d):
                if po[b] is None:                                                   # (no active component: z alone)
                    wgt, mean, var, x = Wm[b], mm[b], vm[b], np.zeros(nm)
                else:
                    Db, yb, Vb = po[b]
                    k = len(yb)
                    wgt = np.concatenate([Wm[b], Db], axis=0)                        # :630-633
                    mean = np.concatenate([mm[b], np.zeros(k)])
                    var = np.zeros((nm + k, nm + k))
                    var[:nm, :nm], var[nm:, nm:] = vm[b], Vb
                    x = np.concatenate([np.zeros(nm), yb])
                m[b], v[b] = ko.update(mean_state_pred=mp[b], var_state_pred=vp[b], x_meas=x, mean_meas=mean, wgt_meas=wgt,
                                       var_meas=var)
            i += 1
        else:
            m, v = ko.update(mean_state_pred=mp, var_state_pred=vp, x_meas=np.zeros((d, nm)), mean_meas=mm, wgt_meas=Wm,
                             var_meas=vm)
        mp_[n + 1], vp_[n + 1], mf_[n + 1], vf_[n + 1] = mp, vp, m, v
    return (mp_, vp_), (mf_, vf_)


def _filter_ode(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, **params):
    """_solve_filter_ode: the same filter without observations."""
    return solve_filter_nn(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                           np.zeros((0, np.shape(ode_weight)[0], 1)), np.zeros(0), None, None, None, **params)


def _logx_yhat(mp, vp, mf, vf, Q, R):
    """dalton.py:701-784: (smoothed means (N+1, d, p), logx_yhat)."""
    N, d = mf.shape[0] - 1, mf.shape[1]
    ms = mf.copy()
    m, v = mf[N], vf[N]
    lp = sum(multivariate_normal_logpdf(mf[N, b], mf[N, b], vf[N, b]) for b in range(d))
    for n in range(N - 1, 0, -1):
        kw = dict(wgt_state=Q, mean_state_filt=mf[n], var_state_filt=vf[n], mean_state_pred=mp[n + 1], var_state_pred=vp[n + 1],
                  var_state=R)
        mc, vc = ko.smooth_mv(mean_state_next=m, var_state_next=v, **kw)
        msim, vsim = ko.smooth_sim(x_state_next=m, **kw)
        lp += sum(multivariate_normal_logpdf(mc[b], msim[b], vsim[b]) for b in range(d))
        m, v = mc, vc
        ms[n] = m
    return ms, lp


def _logx_z(ms, mp, vp, mf, vf, Q, R):
    """dalton.py:787-849."""
    N, d = mf.shape[0] - 1, mf.shape[1]
    lp = sum(multivariate_normal_logpdf(ms[N, b], mf[N, b], vf[N, b]) for b in range(d))
    for n in range(N - 1, 0, -1):
        msim, vsim = ko.smooth_sim(x_state_next=ms[n + 1], wgt_state=Q, mean_state_filt=mf[n], var_state_filt=vf[n],
                                   mean_state_pred=mp[n + 1], var_state_pred=vp[n + 1], var_state=R)
        lp += sum(multivariate_normal_logpdf(ms[n, b], msim[b], vsim[b]) for b in range(d))
    return lp


def daltonng(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, obs_data, obs_times,
             loglik, grad, hess, active=None, literal=False, parts=False, **params):
    """dalton.py:851-949: logy_x + logx_z - logx_yhat (``parts=True``: the three terms)."""
    Q, R = (np.asarray(a, dtype=np.float64) for a in prior_pars)
    obs_data = np.asarray(obs_data, dtype=np.float64)
    (mp, vp), (mf, vf) = solve_filter_nn(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                                         obs_data, obs_times, loglik, grad, hess, active, literal, **params)
    if not (np.all(np.isfinite(mf)) and np.all(np.isfinite(vf))):                   # (LAPACK's eigh raises on NaN)
        return (np.nan, np.nan, np.nan) if parts else np.nan
    ms, logx_yhat = _logx_yhat(mp, vp, mf, vf, Q, R)
    ind = _grid_index(t_min, t_max, n_steps, obs_times)
    logy_x = sum(loglik(obs_data[i], ms[ind[i]], i, **params) for i in range(len(ind)))
    (mp, vp), (mf, vf) = _filter_ode(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, **params)
    logx_z = _logx_z(ms, mp, vp, mf, vf, Q, R)
    return (logy_x, logx_z, logx_yhat) if parts else logy_x + logx_z - logx_yhat


def solve_mv_nn(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, obs_data, obs_times,
                loglik, grad, hess, active=None, literal=False, **params):
    """dalton.py:955-1039: the filter above, then smooth_mv; row 0 = (ode_init, 0)."""
    Q, R = (np.asarray(a, dtype=np.float64) for a in prior_pars)
    (mp, vp), (mf, vf) = solve_filter_nn(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                                         obs_data, obs_times, loglik, grad, hess, active, literal, **params)
    ms, vs = mf.copy(), vf.copy()
    m, v = mf[n_steps], vf[n_steps]
    for n in range(n_steps - 1, 0, -1):
        m, v = ko.smooth_mv(mean_state_next=m, var_state_next=v, wgt_state=Q, mean_state_filt=mf[n], var_state_filt=vf[n],
                            mean_state_pred=mp[n + 1], var_state_pred=vp[n + 1], var_state=R)
        ms[n], vs[n] = m, v
    ms[0], vs[0] = mf[0], 0.0
    return ms, vs


# ---- test log-likelihoods with hand-written derivatives: (loglik, grad, hess, active per block) --------------------------

def poisson(b0=0.1, b1=0.5):
    """parameter.md:545-559: y_b ~ Poisson(exp(b0 + b1 X[b, 0])), summed over the blocks."""
    from math import lgamma

    def ll(y, X, i, **params):
        eta = b0 + b1 * X[:, 0]
        return np.sum(y[:, 0] * eta - np.exp(eta)) - sum(lgamma(v + 1.0) for v in y[:, 0])

    def grad(y, X, i, **params):
        g = np.zeros_like(X)
        g[:, 0] = b1 * (y[:, 0] - np.exp(b0 + b1 * X[:, 0]))
        return g

    def hess(y, X, i, **params):
        H = np.zeros(X.shape + X.shape[-1:])
        H[:, 0, 0] = -b1 * b1 * np.exp(b0 + b1 * X[:, 0])
        return H
    return ll, grad, hess


def gaussian_first(s2):
    """y_b ~ N(X[b, 0], s2): the expansion is exact and yhat = y."""
    def ll(y, X, i, **params):
        r = y[:, 0] - X[:, 0]
        return np.sum(-0.5 * r * r / s2 - 0.5 * np.log(2 * np.pi * s2))

    def grad(y, X, i, **params):
        g = np.zeros_like(X)
        g[:, 0] = (y[:, 0] - X[:, 0]) / s2
        return g

    def hess(y, X, i, **params):
        H = np.zeros(X.shape + X.shape[-1:])
        H[:, 0, 0] = -1.0 / s2
        return H
    return ll, grad, hess


def gaussian_all(s2):
    """y[b, j] ~ N(X[b, j], s2[j]) for EVERY state component: a diagonal Hessian without zero rows."""
    s2 = np.asarray(s2, dtype=np.float64)

    def ll(y, X, i, **params):
        r = y - X
        return np.sum(-0.5 * r * r / s2 - 0.5 * np.log(2 * np.pi * s2))

    def grad(y, X, i, **params):
        return (y - X) / s2

    def hess(y, X, i, **params):
        H = np.zeros(X.shape + X.shape[-1:])
        for j in range(X.shape[-1]):
            H[:, j, j] = -1.0 / s2[j]
        return H
    return ll, grad, hess


def coupled():
    """tests/test_gpu_daltonng.py's coupled_loglik: the blocks are coupled through X[0, 0] X[1, 0], block 0 has two active
    components, theta[0] enters; hand-written gradient and diagonal Hessian blocks."""
    def ll(y, X, i, theta=(0.2, 0.2, 3.0)):
        r0, r1 = y[0, 0] - X[0, 0] * X[1, 0], y[1, 0] - theta[0] * X[0, 1]
        return -0.5 * r0 * r0 / 0.04 - 0.5 * r1 * r1 / 0.25 - 0.5 * (X[0, 0] - 0.3 * X[0, 1]) ** 2 - 0.5 * X[1, 0] ** 2

    def grad(y, X, i, theta=(0.2, 0.2, 3.0)):
        r0, r1, u = y[0, 0] - X[0, 0] * X[1, 0], y[1, 0] - theta[0] * X[0, 1], X[0, 0] - 0.3 * X[0, 1]
        g = np.zeros(X.shape)
        g[0, 0] = r0 * X[1, 0] / 0.04 - u
        g[0, 1] = r1 * theta[0] / 0.25 + 0.3 * u
        g[1, 0] = r0 * X[0, 0] / 0.04 - X[1, 0]
        return g

    def hess(y, X, i, theta=(0.2, 0.2, 3.0)):
        H = np.zeros(X.shape + X.shape[-1:])
        H[0, 0, 0] = -X[1, 0] ** 2 / 0.04 - 1.0
        H[0, 0, 1] = H[0, 1, 0] = 0.3
        H[0, 1, 1] = -theta[0] ** 2 / 0.25 - 0.09
        H[1, 0, 0] = -X[0, 0] ** 2 / 0.04 - 1.0
        return H
    return ll, grad, hess
