"""
Test helper (not collected): NumPy restatement of ``rodeo_amd.solve_evidence_grid`` / ``solve_mv_dynamic_grid`` /
``solve_sim_dynamic_grid``, built on oracle.kalman_ops, oracle.interrogations and the product's own
slot rule ``rodeo_amd.grid.grid_slots`` (host arithmetic on the grid; nothing of the device).

    * ``evidence``: tests/evidence_oracle.py's filter with step n's pair (Q_n, R_n) = prior_at(h_rep[slot[n]]) and the
      interrogation at t_grid[n+1];
    * ``dynamic_filter``: tests/dynamic_oracle.py's with the same two changes -- mu- = Q_n mu, P = Q_n Sigma Q_n^T,
      c = max(z^2 / (W~ R_n W~^T), scale_min), Sigma- = P + c R_n, var_meas from this Sigma-;
    * the backward passes of tests/grid_oracle.py (the gain of step n formed with Q_n) on these predictions,
      var_state_pred = P + c R_n.

``prior_at`` is called once per slot.  One trajectory gives the reference's shapes; a leading batch axis on ode_init, on what
prior_at returns or on the params adds a leading B to every output.
"""
import numpy as np
from oracle import kalman_ops, counter_rng
from oracle.interrogations import psd_factor
from rodeo_amd.grid import grid_slots
from dynamic_oracle import Filtered, LOG_2PI, _T, _out


def _setup(ode_weight, ode_init, t_grid, prior_at, params):
    t = np.asarray(t_grid, dtype=np.float64)
    h_rep, slot = grid_slots(t)
    slots = [tuple(np.asarray(a, dtype=np.float64) for a in prior_at(float(h))) for h in h_rep]
    W = np.asarray(ode_weight, dtype=np.float64)
    x0 = np.asarray(ode_init, dtype=np.float64)
    d, m, p = W.shape
    assert m == 1
    sizes = [x0.shape[0]] if x0.ndim == 3 else []
    sizes += [a.shape[0] for pair in slots for a in pair if a.ndim == 4]
    sizes += [np.shape(v)[0] for v in params.values() if np.ndim(v) >= 2]
    B = sizes[0] if sizes else 1
    return t, [slots[s] for s in slot], W, x0, d, p, B, bool(sizes)


def evidence(ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, **params):
    """(logdens, quad, logdet): a float and (d,), or (B,) and (B, d) for batched inputs."""
    t, pairs, W, x0, d, p, B, batched = _setup(ode_weight, ode_init, t_grid, prior_at, params)
    N = len(pairs)
    mean, var = np.broadcast_to(x0, (B, d, p)).copy(), np.zeros((B, d, p, p))
    quad, logdet = np.zeros((B, d)), np.zeros((B, d))
    for n in range(N):
        Q, R = pairs[n]
        mp, vp = kalman_ops.predict(mean_state_past=mean, var_state_past=var, mean_state=np.zeros_like(mean), wgt_state=Q,
                                    var_state=R)
        wgt, mm, vm = interrogate(key=None, ode_fun=ode_fun, ode_weight=W, t=t[n + 1], mean_state_pred=mp, var_state_pred=vp,
                                  **params)
        Wm = W + wgt
        mf, vf = kalman_ops.forecast(mean_state_pred=mp, var_state_pred=vp, mean_meas=mm, wgt_meas=Wm, var_meas=vm)
        z, s = -mf[..., 0], vf[..., 0, 0]
        quad += z * z / s
        logdet += np.log(s)
        mean, var = kalman_ops.update(mean_state_pred=mp, var_state_pred=vp, x_meas=np.zeros((B, d, 1)), mean_meas=mm,
                                      wgt_meas=Wm, var_meas=vm)
    tot = np.zeros(B)
    for b in range(d):                                              # block order
        tot = tot + (quad[:, b] + logdet[:, b])
    logdens = -0.5 * tot - d * N * LOG_2PI / 2.0
    if batched:
        return logdens, quad, logdet
    return float(logdens[0]), quad[0], logdet[0]


def dynamic_filter(ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, scale_min=0.0, **params):
    """The forward pass: ``dynamic_oracle.Filtered`` (every array with a leading B) and the per-step pairs."""
    t, pairs, W, x0, d, p, B, batched = _setup(ode_weight, ode_init, t_grid, prior_at, params)
    N = len(pairs)
    mean, var = np.broadcast_to(x0, (B, d, p)).copy(), np.zeros((B, d, p, p))
    mp, vp = np.empty((B, N + 1, d, p)), np.empty((B, N + 1, d, p, p))
    mf, vf = np.empty_like(mp), np.empty_like(vp)
    mp[:, 0] = mf[:, 0] = mean
    vp[:, 0] = vf[:, 0] = 0.0
    scale, quad, logdet = np.empty((B, N, d)), np.zeros((B, d)), np.zeros((B, d))
    for n in range(N):
        Q, R = pairs[n]
        Rb = np.broadcast_to(R, (B, d, p, p))
        mpr, P = kalman_ops.predict(mean_state_past=mean, var_state_past=var, mean_state=np.zeros_like(mean), wgt_state=Q,
                                    var_state=np.zeros((d, p, p)))
        wgt, mm, _ = interrogate(key=None, ode_fun=ode_fun, ode_weight=W, t=t[n + 1], mean_state_pred=mpr, var_state_pred=P,
                                 **params)
        Wm = W + wgt
        z = -(np.matmul(Wm, mpr[..., None])[..., 0] + mm)[..., 0]                      # (B, d)
        r = np.matmul(np.matmul(Wm, Rb), _T(Wm))[..., 0, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.maximum(z * z / r, scale_min)
        Sp = P + c[..., None, None] * Rb
        _, _, vm = interrogate(key=None, ode_fun=ode_fun, ode_weight=W, t=t[n + 1], mean_state_pred=mpr, var_state_pred=Sp,
                               **params)
        _, vfore = kalman_ops.forecast(mean_state_pred=mpr, var_state_pred=Sp, mean_meas=mm, wgt_meas=Wm, var_meas=vm)
        s = vfore[..., 0, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            quad += z * z / s
            logdet += np.log(s)
        mean, var = kalman_ops.update(mean_state_pred=mpr, var_state_pred=Sp, x_meas=np.zeros((B, d, 1)), mean_meas=mm,
                                      wgt_meas=Wm, var_meas=vm)
        scale[:, n] = c
        mp[:, n + 1], vp[:, n + 1], mf[:, n + 1], vf[:, n + 1] = mpr, Sp, mean, var
    tot = np.zeros(B)
    for b in range(d):                                              # block order
        tot = tot + (quad[:, b] + logdet[:, b])
    logdens = -0.5 * tot - d * N * LOG_2PI / 2.0
    return Filtered(mp, vp, mf, vf, scale, quad, logdet, logdens, batched), pairs


def solve_mv_dynamic_grid(ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, scale_min=0.0, **params):
    """(mean, var, scale, logdens): tests/grid_oracle.py's smoothing pass on the calibrated predictions."""
    f, pairs = dynamic_filter(ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, scale_min, **params)
    N = len(pairs)
    ms, vs = np.empty_like(f.mean_filt), np.empty_like(f.var_filt)
    ms[:, N], vs[:, N] = f.mean_filt[:, N], f.var_filt[:, N]
    mean_next, var_next = f.mean_filt[:, N], f.var_filt[:, N]
    for n in range(N - 1, 0, -1):
        mean_next, var_next = kalman_ops.smooth_mv(
            mean_state_next=mean_next, var_state_next=var_next, wgt_state=pairs[n][0], mean_state_filt=f.mean_filt[:, n],
            var_state_filt=f.var_filt[:, n], mean_state_pred=f.mean_pred[:, n + 1], var_state_pred=f.var_pred[:, n + 1])
        ms[:, n], vs[:, n] = mean_next, var_next
    ms[:, 0], vs[:, 0] = f.mean_filt[:, 0], 0.0
    return _out(f, ms, vs, f.scale)


def solve_sim_dynamic_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, scale_min=0.0, traj_offset=0,
                           **params):
    """(x, scale, logdens): tests/grid_oracle.py's sampling pass (PURPOSE_SMOOTH draws keyed by trajectory, step, block)."""
    f, pairs = dynamic_filter(ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, scale_min, **params)
    N = len(pairs)
    B, _, d, p = f.mean_filt.shape
    traj = traj_offset + np.arange(B)
    seed = 0 if key is None else key

    def draw(n, mean, var):
        z = counter_rng.normals(seed, traj, n, d, p, counter_rng.PURPOSE_SMOOTH)
        return mean + np.matmul(psd_factor(var), z[..., None])[..., 0]

    xs = np.empty_like(f.mean_filt)
    x_next = draw(N, f.mean_filt[:, N], f.var_filt[:, N])
    xs[:, N] = x_next
    for n in range(N - 1, 0, -1):
        mean_sim, var_sim = kalman_ops.smooth_sim(
            x_state_next=x_next, wgt_state=pairs[n][0], mean_state_filt=f.mean_filt[:, n], var_state_filt=f.var_filt[:, n],
            mean_state_pred=f.mean_pred[:, n + 1], var_state_pred=f.var_pred[:, n + 1])
        x_next = draw(n, mean_sim, var_sim)
        xs[:, n] = x_next
    xs[:, 0] = f.mean_filt[:, 0]
    return _out(f, xs, f.scale)
