"""
Test helper (not collected): NumPy restatement of ``dalton_grid`` / ``dalton.solve_mv_grid`` / ``dalton.solve_sim_grid``
(``rodeo_amd.inference.dalton``), on tests/grid_oracle.py's ``grid_filter`` pattern: oracle.kalman_ops,
oracle.interrogations, oracle.fenrir's ``multivariate_normal_logpdf`` (utils.py:60-78, the 1e-8 rule) and the product's own slot
rule ``rodeo_amd.grid.grid_slots`` (host arithmetic on the grid; nothing of the device).

Step n -> n + 1 of the joint filter: predict with (Q_n, R_n) = prior_at(h_rep[slot[n]]), interrogate at t_grid[n+1], forecast
log-density of z = 0 and update, then -- if node n + 1 is observed -- forecast log-density of y and update: z first, y second.
The marginal filter is the same without y.  An observation on node 0 adds log N(y_0; D_0 x_0, Omega_0) to the joint density and
updates nothing.  ``nodes`` holds the NODE of every observation, strictly increasing.  The backward passes are grid_oracle's own
code, run on this filter's moments.  One trajectory gives the reference's shapes; a leading batch axis on ode_init, on what
prior_at returns or on the params adds a leading B, like grid_oracle.
"""
import contextlib
import numpy as np
from oracle import kalman_ops as ko, scan
from oracle.fenrir import multivariate_normal_logpdf
from oracle.interrogations import StepKey
from rodeo_amd.grid import grid_slots
import grid_oracle as go


def _logpdf(x, mean, var, seen):
    """Sum over blocks of one trajectory's forecast log-densities; the forecast variances' eigenvalues go to ``seen``."""
    if seen is not None:
        seen.extend(np.abs(np.linalg.eigvalsh(v)) for v in var)
    return sum(multivariate_normal_logpdf(x[b], mean[b], var[b]) for b in range(len(x)))


def filters(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, nodes, obs_weight, obs_var,
            with_obs=True, traj_offset=0, forecast_vars=None, **params):
    """One forward filter (joint, or marginal with ``with_obs=False``): ``(logdens (B,), (mp, vp, mf, vf), pairs, squeeze)`` with
    grid_oracle.grid_filter's records.  ``forecast_vars``: a list that receives |eigenvalues| of every forecast variance."""
    t = np.asarray(t_grid, dtype=np.float64)
    h_rep, slot = grid_slots(t)
    slots = [tuple(np.asarray(a, dtype=np.float64) for a in prior_at(float(h))) for h in h_rep]
    pairs = [slots[s] for s in slot]
    N = len(slot)
    W = np.asarray(ode_weight, dtype=np.float64)
    d, m, p = W.shape[-3:]
    B = scan._batch_size(W, ode_init, slots[0][0], slots[0][1], params, scan._default_batched_params(params))
    for Q, R in slots[1:]:
        for a in (Q, R):
            if a.ndim == 4:
                B = a.shape[0] if B in (None, 1) else B
    squeeze = B is None
    B = 1 if squeeze else B
    y, D, Om = (np.asarray(a, dtype=np.float64) for a in (obs_data, obs_weight, obs_var))
    nodes = np.asarray(nodes, dtype=np.int64)
    assert np.all(np.diff(nodes) > 0) and (len(nodes) == 0 or (nodes[0] >= 0 and nodes[-1] <= N))
    nb = D.shape[2] if D.ndim == 4 else 1
    mean = np.broadcast_to(np.asarray(ode_init, dtype=np.float64), (B, d, p)).copy()
    var = np.zeros((B, d, p, p))
    mp, vp = np.empty((B, N + 1, d, p)), np.empty((B, N + 1, d, p, p))
    mf, vf = np.empty_like(mp), np.empty_like(vp)
    mp[:, 0] = mf[:, 0] = mean
    vp[:, 0] = vf[:, 0] = 0.0
    logdens = np.zeros(B)
    i = 0
    if len(nodes) and nodes[0] == 0:                                # dalton.py:206-215
        if with_obs:
            for b in range(B):
                logdens[b] += _logpdf(y[0], ko._mv(D[0], mean[b]), Om[0], forecast_vars)
        i = 1
    traj = traj_offset + np.arange(B)
    zeros_z, zeros_y = np.zeros((B, d, m)), np.zeros((B, d, nb))
    for n in range(N):
        Q, R = pairs[n]
        mean_pred, var_pred = ko.predict(mean_state_past=mean, var_state_past=var, mean_state=np.zeros((B, d, p)), wgt_state=Q,
                                         var_state=R)
        step_key = None if key is None else StepKey(key, traj, n)
        wgt_meas, mean_meas, var_meas = interrogate(key=step_key, ode_fun=ode_fun, ode_weight=W, t=t[n + 1],
                                                    mean_state_pred=mean_pred, var_state_pred=var_pred, **params)
        Wm = np.broadcast_to(W + wgt_meas, (B, d, m, p))
        zm, zv = ko.forecast(mean_state_pred=mean_pred, var_state_pred=var_pred, mean_meas=mean_meas, wgt_meas=Wm, var_meas=var_meas)
        for b in range(B):
            logdens[b] += _logpdf(zeros_z[b], zm[b], zv[b], forecast_vars)
        mean, var = ko.update(mean_state_pred=mean_pred, var_state_pred=var_pred, x_meas=zeros_z, mean_meas=mean_meas, wgt_meas=Wm,
                              var_meas=var_meas)
        if i < len(nodes) and nodes[i] == n + 1:
            if with_obs:
                Di, Omi = np.broadcast_to(D[i], (B, d, nb, p)), np.broadcast_to(Om[i], (B, d, nb, nb))
                yi = np.broadcast_to(y[i], (B, d, nb))
                ym, yv = ko.forecast(mean_state_pred=mean, var_state_pred=var, mean_meas=zeros_y, wgt_meas=Di, var_meas=Omi)
                for b in range(B):
                    logdens[b] += _logpdf(yi[b], ym[b], yv[b], forecast_vars)
                mean, var = ko.update(mean_state_pred=mean, var_state_pred=var, x_meas=yi, mean_meas=zeros_y, wgt_meas=Di, var_meas=Omi)
            i += 1
        mp[:, n + 1], vp[:, n + 1], mf[:, n + 1], vf[:, n + 1] = mean_pred, var_pred, mean, var
    return logdens, (mp, vp, mf, vf), pairs, squeeze


def dalton_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, nodes, obs_weight, obs_var,
                forecast_vars=None, **params):
    """joint - marginal: a float, or (B,)."""
    args = (key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, nodes, obs_weight, obs_var)
    lj, _, _, squeeze = filters(*args, forecast_vars=forecast_vars, **params)
    lm = filters(*args, with_obs=False, forecast_vars=forecast_vars, **params)[0]
    return float(lj[0] - lm[0]) if squeeze else lj - lm


@contextlib.contextmanager
def _filter_of(obs_data, nodes, obs_weight, obs_var):
    """grid_oracle's backward passes read ``go.grid_filter``: for the length of a call it is the joint filter above."""
    def joint(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, traj_offset=0, **params):
        return filters(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, nodes, obs_weight, obs_var,
                       traj_offset=traj_offset, **params)[1:]
    plain, go.grid_filter = go.grid_filter, joint
    try:
        yield
    finally:
        go.grid_filter = plain


def solve_mv_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, nodes, obs_weight, obs_var, **params):
    with _filter_of(obs_data, nodes, obs_weight, obs_var):
        return go.solve_mv_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, **params)


def solve_sim_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, nodes, obs_weight, obs_var, **params):
    with _filter_of(obs_data, nodes, obs_weight, obs_var):
        return go.solve_sim_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, **params)
