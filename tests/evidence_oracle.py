"""
Test helper (not collected): NumPy restatement of ``rodeo_amd.solve_evidence`` in either Kalman form, built on
oracle.kalman_ops / oracle.sqrt_ops and oracle.interrogations.  The solver's forward filter (src/rodeo/solve.py:47-122) with,
at every step, the forecast of the interrogation's measurement (standard.py / square_root.py ``forecast``): z the innovation
0 - mean_fore, s its variance.  The density is the plain Gaussian one, with no threshold on s.

One trajectory -- ode_init (d, p), prior_pars ((d, p, p), (d, p, p)), unbatched params -- gives (logdens, quad (d,),
logdet (d,)).  A leading batch axis on ode_init, either prior matrix or the params (the oracle's ops and interrogations take
leading axes) runs the trajectories side by side through the same lines and gives (B,), (B, d), (B, d).
"""
import numpy as np
from oracle import kalman_ops, sqrt_ops

LOG_2PI = np.log(2.0 * np.pi)


def evidence(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type="standard", **params):
    funs = {"standard": kalman_ops, "square-root": sqrt_ops}[kalman_type]
    W = np.asarray(ode_weight, dtype=np.float64)
    Q, R = (np.asarray(a, dtype=np.float64) for a in prior_pars)
    x0 = np.asarray(ode_init, dtype=np.float64)
    d, m, p = W.shape
    assert m == 1
    sizes = [a.shape[0] for a, nd in ((x0, 3), (Q, 4), (R, 4)) if a.ndim == nd]
    sizes += [np.shape(v)[0] for v in params.values() if np.ndim(v) >= 2]
    B = sizes[0] if sizes else 1
    mean, var = np.broadcast_to(x0, (B, d, p)).copy(), np.zeros((B, d, p, p))
    quad, logdet = np.zeros((B, d)), np.zeros((B, d))
    for n in range(n_steps):
        t = t_min + (t_max - t_min) * (n + 1) / n_steps
        mp, vp = funs.predict(mean_state_past=mean, var_state_past=var, mean_state=np.zeros_like(mean), wgt_state=Q,
                              var_state=R)
        wgt, mm, vm = interrogate(key=None, ode_fun=ode_fun, ode_weight=W, t=t, mean_state_pred=mp, var_state_pred=vp, **params)
        Wm = W + wgt
        mf, vf = funs.forecast(mean_state_pred=mp, var_state_pred=vp, mean_meas=mm, wgt_meas=Wm, var_meas=vm)
        z, s = -mf[..., 0], vf[..., 0, 0]
        quad += z * z / s
        logdet += np.log(s)
        mean, var = funs.update(mean_state_pred=mp, var_state_pred=vp, x_meas=np.zeros((B, d, 1)), mean_meas=mm, wgt_meas=Wm,
                                var_meas=vm)
    tot = np.zeros(B)
    for b in range(d):                                              # block order
        tot = tot + (quad[:, b] + logdet[:, b])
    logdens = -0.5 * tot - d * n_steps * LOG_2PI / 2.0
    if sizes:
        return logdens, quad, logdet
    return float(logdens[0]), quad[0], logdet[0]
