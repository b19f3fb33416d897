"""
Test helper (not collected): NumPy restatement of ``rodeo_amd.solve_mv_dynamic`` / ``solve_sim_dynamic`` (DESIGN.md section 7
(13)), built on oracle.kalman_ops and oracle.interrogations, plus oracle.counter_rng for the draws the way oracle/scan.py
draws them.  The solver's forward filter (src/rodeo/solve.py:47-122) with the prior variance of step n -> n + 1 scaled, per
block, by the estimate made at that step before its update:

    mu- = Q mu,  P = Q Sigma Q^T                       (no R yet)
    W~ = W + wgt_meas, a = mean_meas at mu-            (var_meas is not needed for these)
    z = 0 - (W~ mu- + a),  r = W~ R W~^T,  c = max(z^2 / r, scale_min)
    Sigma- = P + c R;  var_meas from THIS Sigma- (rodeo: W Sigma- W^T; schober, kramer: 0)
    s = W~ Sigma- W~^T + var_meas, the usual update;  quad += z^2 / s, logdet += log s

and the two backward passes of oracle/scan.py on the predicted moments (mu-, Sigma-) this filter made.

One trajectory -- ode_init (d, p), prior_pars ((d, p, p), (d, p, p)), unbatched params -- gives the reference's shapes; a
leading batch axis on ode_init, either prior matrix or the params runs the trajectories side by side through the same lines
and adds a leading B to every output, like tests/evidence_oracle.py.
"""
import collections
import numpy as np
from oracle import kalman_ops, counter_rng
from oracle.interrogations import psd_factor

LOG_2PI = np.log(2.0 * np.pi)

Filtered = collections.namedtuple("Filtered", ["mean_pred", "var_pred", "mean_filt", "var_filt", "scale", "quad", "logdet",
                                               "logdens", "batched"])


def _T(A):
    return np.swapaxes(A, -1, -2)


def dynamic_filter(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, scale_min=0.0, **params):
    """The forward pass; every array with a leading B (1 for one trajectory), ``batched`` says which."""
    W = np.asarray(ode_weight, dtype=np.float64)
    Q, R = (np.asarray(a, dtype=np.float64) for a in prior_pars)
    x0 = np.asarray(ode_init, dtype=np.float64)
    d, m, p = W.shape
    assert m == 1
    sizes = [a.shape[0] for a, nd in ((x0, 3), (Q, 4), (R, 4)) if a.ndim == nd]
    sizes += [np.shape(v)[0] for v in params.values() if np.ndim(v) >= 2]
    B = sizes[0] if sizes else 1
    N = int(n_steps)
    mean, var = np.broadcast_to(x0, (B, d, p)).copy(), np.zeros((B, d, p, p))
    mp, vp = np.empty((B, N + 1, d, p)), np.empty((B, N + 1, d, p, p))
    mf, vf = np.empty_like(mp), np.empty_like(vp)
    mp[:, 0] = mf[:, 0] = mean
    vp[:, 0] = vf[:, 0] = 0.0
    scale, quad, logdet = np.empty((B, N, d)), np.zeros((B, d)), np.zeros((B, d))
    Rb = np.broadcast_to(R, (B, d, p, p))
    for n in range(N):
        t = t_min + (t_max - t_min) * (n + 1) / N
        mpr, P = kalman_ops.predict(mean_state_past=mean, var_state_past=var, mean_state=np.zeros_like(mean), wgt_state=Q,
                                    var_state=np.zeros((d, p, p)))
        wgt, mm, _ = interrogate(key=None, ode_fun=ode_fun, ode_weight=W, t=t, mean_state_pred=mpr, var_state_pred=P, **params)
        Wm = W + wgt
        z = -(np.matmul(Wm, mpr[..., None])[..., 0] + mm)[..., 0]                      # (B, d)
        r = np.matmul(np.matmul(Wm, Rb), _T(Wm))[..., 0, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.maximum(z * z / r, scale_min)
        Sp = P + c[..., None, None] * Rb
        _, _, vm = interrogate(key=None, ode_fun=ode_fun, ode_weight=W, t=t, mean_state_pred=mpr, var_state_pred=Sp, **params)
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
    return Filtered(mp, vp, mf, vf, scale, quad, logdet, logdens, bool(sizes))


def _out(f, *arrays):
    res = tuple(a if f.batched else a[0] for a in arrays)
    ld = f.logdens if f.batched else float(f.logdens[0])
    return res + (ld,)


def solve_mv_dynamic(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, scale_min=0.0, **params):
    """(mean, var, scale, logdens): oracle/scan.py's solve_mv backward pass on the calibrated predictions."""
    f = dynamic_filter(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, scale_min, **params)
    Q = np.asarray(prior_pars[0], dtype=np.float64)
    N = int(n_steps)
    ms, vs = np.empty_like(f.mean_filt), np.empty_like(f.var_filt)
    ms[:, N], vs[:, N] = f.mean_filt[:, N], f.var_filt[:, N]
    mean_next, var_next = f.mean_filt[:, N], f.var_filt[:, N]
    for n in range(N - 1, 0, -1):
        mean_next, var_next = kalman_ops.smooth_mv(
            mean_state_next=mean_next, var_state_next=var_next, wgt_state=Q, mean_state_filt=f.mean_filt[:, n],
            var_state_filt=f.var_filt[:, n], mean_state_pred=f.mean_pred[:, n + 1], var_state_pred=f.var_pred[:, n + 1])
        ms[:, n], vs[:, n] = mean_next, var_next
    ms[:, 0], vs[:, 0] = f.mean_filt[:, 0], 0.0
    return _out(f, ms, vs, f.scale)


def solve_sim_dynamic(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, scale_min=0.0,
                      traj_offset=0, **params):
    """(x, scale, logdens): oracle/scan.py's solve_sim backward pass (PURPOSE_SMOOTH draws keyed by trajectory, step, block)."""
    f = dynamic_filter(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, scale_min, **params)
    Q = np.asarray(prior_pars[0], dtype=np.float64)
    N = int(n_steps)
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
            x_state_next=x_next, wgt_state=Q, mean_state_filt=f.mean_filt[:, n], var_state_filt=f.var_filt[:, n],
            mean_state_pred=f.mean_pred[:, n + 1], var_state_pred=f.var_pred[:, n + 1])
        x_next = draw(n, mean_sim, var_sim)
        xs[:, n] = x_next
    xs[:, 0] = f.mean_filt[:, 0]
    return _out(f, xs, f.scale)
