"""
Test helper (not collected): NumPy restatement of DALTON for Gaussian observations (src/rodeo/inference/dalton.py:39-545) in
its literal form -- the stacked measurement [W~; D_i] with the joint eigendecomposition log-density (utils.py:60-78) and the
joint LU update (standard.py:93-102) -- for ONE trajectory: ode_init (d, p), prior_pars ((d, p, p), (d, p, p)), unbatched
params.  Built on oracle.kalman_ops, oracle.interrogations and oracle.fenrir.multivariate_normal_logpdf.  ``solve_sim`` draws
from the Philox stream of oracle/scan.solve_sim (trajectory index ``traj``).
"""
import numpy as np
from oracle import kalman_ops as ko, counter_rng
from oracle.fenrir import multivariate_normal_logpdf
from oracle.interrogations import psd_factor


def _grid_index(t_min, t_max, n_steps, obs_times):
    return np.searchsorted(np.linspace(t_min, t_max, n_steps + 1), np.asarray(obs_times, dtype=np.float64))


def _forecast_update(mean, var, x, mean_meas, wgt, var_meas):
    """fenrir.py:40-81 per block: (sum of block log-densities, updated mean, updated var)."""
    mf, vf = ko.forecast(mean_state_pred=mean, var_state_pred=var, mean_meas=mean_meas, wgt_meas=wgt, var_meas=var_meas)
    logp = sum(multivariate_normal_logpdf(x[b], mf[b], vf[b]) for b in range(len(x)))
    m, v = ko.update(mean_state_pred=mean, var_state_pred=var, x_meas=x, mean_meas=mean_meas, wgt_meas=wgt, var_meas=var_meas)
    return logp, m, v


def _step(ode_fun, ode_weight, interrogate, t, mean, var, Q, R, params):
    """predict + interrogation on this filter's own predicted moments (dalton.py:112-134)."""
    mp, vp = ko.predict(mean_state_past=mean, var_state_past=var, mean_state=np.zeros_like(mean), wgt_state=Q, var_state=R)
    wgt, mm, vm = interrogate(key=None, ode_fun=ode_fun, ode_weight=ode_weight, t=t, mean_state_pred=mp[None],
                              var_state_pred=vp[None], **params)
    return mp, vp, ode_weight + wgt[0], mm[0], vm[0]


def _joint(mp, vp, Wm, mm, vm, obs_data, obs_weight, obs_var, i):
    """The stacked measurement of dalton.py:136-143: ([W~; D_i], [mean_meas; 0], blockdiag(var_meas, Omega_i), [0; y_i])."""
    d, nm, _ = Wm.shape
    nb = obs_weight.shape[2]
    wgt = np.concatenate([Wm, obs_weight[i]], axis=1)
    mean = np.concatenate([mm, np.zeros((d, nb))], axis=1)
    var = np.zeros((d, nm + nb, nm + nb))
    var[:, :nm, :nm] = vm
    var[:, nm:, nm:] = obs_var[i]
    x = np.concatenate([np.zeros((d, nm)), obs_data[i]], axis=1)
    return x, mean, wgt, var


def dalton(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
           obs_data, obs_times, obs_weight, obs_var, **params):
    """dalton.py:39-235: logdens_joint - logdens_marg."""
    W = np.asarray(ode_weight, dtype=np.float64)
    x0 = np.asarray(ode_init, dtype=np.float64)
    Q, R = (np.asarray(a, dtype=np.float64) for a in prior_pars)
    obs_data, obs_weight, obs_var = (np.asarray(a, dtype=np.float64) for a in (obs_data, obs_weight, obs_var))
    d, nm, p = W.shape
    ind = _grid_index(t_min, t_max, n_steps, obs_times)
    n_obs = len(ind)
    lj, lm, i = 0.0, 0.0, 0
    if n_obs and ind[0] == 0:                                       # dalton.py:206-215
        lj = sum(multivariate_normal_logpdf(obs_data[0, b], obs_weight[0, b] @ x0[b], obs_var[0, b]) for b in range(d))
        i = 1
    mj, vj = x0.copy(), np.zeros((d, p, p))
    mz, vz = x0.copy(), np.zeros((d, p, p))
    zx = np.zeros((d, nm))
    for n in range(n_steps):
        t = t_min + (t_max - t_min) * (n + 1) / n_steps
        mp, vp, Wm, mm, vm = _step(ode_fun, W, interrogate, t, mj, vj, Q, R, params)
        if i < n_obs and n + 1 == ind[i]:                          # dalton.py:136-149
            lp, mj, vj = _forecast_update(mp, vp, *_joint(mp, vp, Wm, mm, vm, obs_data, obs_weight, obs_var, i))
            i += 1
        else:
            lp, mj, vj = _forecast_update(mp, vp, zx, mm, Wm, vm)
        lj += lp
        mp, vp, Wm, mm, vm = _step(ode_fun, W, interrogate, t, mz, vz, Q, R, params)
        lp, mz, vz = _forecast_update(mp, vp, zx, mm, Wm, vm)
        lm += lp
    return lj - lm


def solve_filter(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                 obs_data, obs_times, obs_weight, obs_var, **params):
    """dalton.py:242-371: (predicted (mean, var), filtered (mean, var)), each (N+1, d, p[, p]), index 0 = (ode_init, 0)."""
    W = np.asarray(ode_weight, dtype=np.float64)
    x0 = np.asarray(ode_init, dtype=np.float64)
    Q, R = (np.asarray(a, dtype=np.float64) for a in prior_pars)
    obs_data, obs_weight, obs_var = (np.asarray(a, dtype=np.float64) for a in (obs_data, obs_weight, obs_var))
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
            x, mean, wgt, var = _joint(mp, vp, Wm, mm, vm, obs_data, obs_weight, obs_var, i)
            i += 1
        else:
            x, mean, wgt, var = np.zeros((d, nm)), mm, Wm, vm
        m, v = ko.update(mean_state_pred=mp, var_state_pred=vp, x_meas=x, mean_meas=mean, wgt_meas=wgt, var_meas=var)
        mp_[n + 1], vp_[n + 1], mf_[n + 1], vf_[n + 1] = mp, vp, m, v
    return (mp_, vp_), (mf_, vf_)


def solve_mv(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
             obs_data, obs_times, obs_weight, obs_var, **params):
    """dalton.py:374-460: the filter above, then smooth_mv with the indices of solve.py:257-302."""
    Q, R = (np.asarray(a, dtype=np.float64) for a in prior_pars)
    (mp, vp), (mf, vf) = solve_filter(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                                      obs_data, obs_times, obs_weight, obs_var, **params)
    ms, vs = mf.copy(), vf.copy()
    m, v = mf[n_steps], vf[n_steps]
    for n in range(n_steps - 1, 0, -1):
        m, v = ko.smooth_mv(mean_state_next=m, var_state_next=v, wgt_state=Q, mean_state_filt=mf[n], var_state_filt=vf[n],
                            mean_state_pred=mp[n + 1], var_state_pred=vp[n + 1], var_state=R)
        ms[n], vs[n] = m, v
    ms[0], vs[0] = mf[0], 0.0
    return ms, vs


def solve_sim(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
              obs_data, obs_times, obs_weight, obs_var, seed=0, traj=0, **params):
    """dalton.py:463-545: the filter above, then the smooth_sim sampler of solve.py:162-204 with oracle/scan.solve_sim's
    normals (Philox, PURPOSE_SMOOTH, time index n) and factor (psd_factor)."""
    Q, R = (np.asarray(a, dtype=np.float64) for a in prior_pars)
    (mp, vp), (mf, vf) = solve_filter(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                                      obs_data, obs_times, obs_weight, obs_var, **params)
    d, p = mf.shape[1:]

    def draw(n, mean, var):
        z = counter_rng.normals(seed, np.array([traj]), n, d, p, counter_rng.PURPOSE_SMOOTH)[0]
        return mean + np.matmul(psd_factor(var), z[..., None])[..., 0]

    xs = np.empty_like(mf)
    x = draw(n_steps, mf[n_steps], vf[n_steps])
    xs[n_steps] = x
    for n in range(n_steps - 1, 0, -1):
        ms, vs = ko.smooth_sim(x_state_next=x, wgt_state=Q, mean_state_filt=mf[n], var_state_filt=vf[n],
                               mean_state_pred=mp[n + 1], var_state_pred=vp[n + 1], var_state=R)
        x = draw(n, ms, vs)
        xs[n] = x
    xs[0] = mf[0]
    return xs
