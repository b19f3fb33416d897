"""
Test helper (not collected): NumPy restatement of ``rodeo_amd.solve_mv_grid`` / ``solve_sim_grid``,
built on oracle.kalman_ops, oracle.interrogations' StepKey and oracle.counter_rng the way oracle/scan.py uses them, and on the
product's own slot rule ``rodeo_amd.grid.grid_slots`` (host arithmetic on the grid; nothing of the device).  The solver's scans
(src/rodeo/solve.py:47-122, 162-204, 257-301) with

    * step n -> n + 1 of length t[n+1] - t[n] under its own prior pair (Q_n, R_n) = prior_at(h_rep[slot[n]]), in ``predict`` and
      in ``smooth_mv`` / ``smooth_sim`` (the gain of step n is formed with Q_n);
    * the interrogation at t = t_grid[n+1].

``prior_at`` is called once per slot.  One trajectory gives the reference's shapes; a leading batch axis on ode_init, on what
prior_at returns or on the params adds a leading B to every output, like oracle/scan.py.
"""
import numpy as np
from oracle import kalman_ops, counter_rng, scan
from oracle.interrogations import StepKey, psd_factor
from rodeo_amd.grid import grid_slots


def grid_filter(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, traj_offset=0, **params):
    """Forward pass: (mp, vp, mf, vf) with a leading B, the per-step pairs [(Q_n, R_n)] and whether to squeeze B away."""
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
    mean = np.broadcast_to(np.asarray(ode_init, dtype=np.float64), (B, d, p)).copy()
    var = np.zeros((B, d, p, p))
    mp, vp = np.empty((B, N + 1, d, p)), np.empty((B, N + 1, d, p, p))
    mf, vf = np.empty_like(mp), np.empty_like(vp)
    mp[:, 0] = mf[:, 0] = mean
    vp[:, 0] = vf[:, 0] = 0.0
    traj = traj_offset + np.arange(B)
    for n in range(N):
        Q, R = pairs[n]
        mean_pred, var_pred = kalman_ops.predict(mean_state_past=mean, var_state_past=var, mean_state=np.zeros((B, d, p)),
                                                 wgt_state=Q, var_state=R)
        step_key = None if key is None else StepKey(key, traj, n)
        wgt_meas, mean_meas, var_meas = interrogate(key=step_key, ode_fun=ode_fun, ode_weight=W, t=t[n + 1],
                                                    mean_state_pred=mean_pred, var_state_pred=var_pred, **params)
        mean, var = kalman_ops.update(mean_state_pred=mean_pred, var_state_pred=var_pred, x_meas=np.zeros((B, d, m)),
                                      mean_meas=mean_meas, wgt_meas=W + wgt_meas, var_meas=var_meas)
        mp[:, n + 1], vp[:, n + 1], mf[:, n + 1], vf[:, n + 1] = mean_pred, var_pred, mean, var
    return (mp, vp, mf, vf), pairs, squeeze


def solve_mv_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, traj_offset=0, **params):
    """(mean, var): oracle/scan.py's solve_mv backward pass with every step's own pair."""
    (mp, vp, mf, vf), pairs, squeeze = grid_filter(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                                                   traj_offset, **params)
    N = len(pairs)
    ms, vs = np.empty_like(mf), np.empty_like(vf)
    ms[:, N], vs[:, N] = mf[:, N], vf[:, N]
    mean_next, var_next = mf[:, N], vf[:, N]
    for n in range(N - 1, 0, -1):
        Q, R = pairs[n]
        mean_next, var_next = kalman_ops.smooth_mv(
            mean_state_next=mean_next, var_state_next=var_next, wgt_state=Q, mean_state_filt=mf[:, n], var_state_filt=vf[:, n],
            mean_state_pred=mp[:, n + 1], var_state_pred=vp[:, n + 1], var_state=R)
        ms[:, n], vs[:, n] = mean_next, var_next
    ms[:, 0], vs[:, 0] = mf[:, 0], 0.0
    return (ms[0], vs[0]) if squeeze else (ms, vs)


def solve_sim_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, traj_offset=0, **params):
    """x: oracle/scan.py's solve_sim backward pass (PURPOSE_SMOOTH draws keyed by trajectory, step, block)."""
    (mp, vp, mf, vf), pairs, squeeze = grid_filter(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                                                   traj_offset, **params)
    N = len(pairs)
    B, _, d, p = mf.shape
    traj = traj_offset + np.arange(B)
    seed = 0 if key is None else key

    def draw(n, mean, var):
        z = counter_rng.normals(seed, traj, n, d, p, counter_rng.PURPOSE_SMOOTH)
        return mean + np.matmul(psd_factor(var), z[..., None])[..., 0]

    xs = np.empty_like(mf)
    x_next = draw(N, mf[:, N], vf[:, N])
    xs[:, N] = x_next
    for n in range(N - 1, 0, -1):
        Q, R = pairs[n]
        mean_sim, var_sim = kalman_ops.smooth_sim(
            x_state_next=x_next, wgt_state=Q, mean_state_filt=mf[:, n], var_state_filt=vf[:, n],
            mean_state_pred=mp[:, n + 1], var_state_pred=vp[:, n + 1], var_state=R)
        x_next = draw(n, mean_sim, var_sim)
        xs[:, n] = x_next
    xs[:, 0] = mf[:, 0]
    return xs[0] if squeeze else xs
