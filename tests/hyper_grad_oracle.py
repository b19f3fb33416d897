"""
Test helper (not collected): a literal NumPy restatement of the tangent recursions of ``dalton_grid_jvp`` and ``fenrir_grid_jvp``
with the two reserved directions ``"log_sigma"`` and ``"log_obs_var"``, one trajectory and one direction
at a time.  It is tests/dalton_grad_oracle.py's / tests/fenrir_grad_oracle.py's recursion with two more terms; per block b, with
l. = the rate of log sigma_b and w. = the rate of the common log-scale of block b's observation variances:

  predict   Sigma.- = Q Sigma. Q^T + 2 l. R     wherever a prediction is formed: DALTON's joint and marginal filter, Fenrir's forward
            filter, and Fenrir's backward pass where it re-evaluates pred[n + 1]; mu.- = Q mu. as before; the initial variance
            and Q carry no tangent
  observe   the y update's variance Omega has the tangent w. Omega (``_update``'s dV), node 0 and node N like any other

``_update`` and the analytic f., J, J. of the two systems are tests/dalton_grad_oracle.py's, imported.  Nothing of the device and
nothing of the value restatements is used: the finite-difference test compares this file with differences of those.
"""
import numpy as np
from rodeo_amd.grid import grid_slots
from dalton_grad_oracle import _update, TANGENTS


def _predict(Q, R, mu, S, dmu, dS, dls):
    """All blocks: (mu-, Sigma-, mu.-, Sigma.-) with Sigma.- = Q Sigma. Q^T + 2 l. R."""
    Qt = np.swapaxes(Q, -1, -2)
    return (np.einsum("bij,bj->bi", Q, mu), Q @ S @ Qt + R, np.einsum("bij,bj->bi", Q, dmu),
            Q @ dS @ Qt + 2.0 * dls[:, None, None] * R)


def _step(tangent_fun, W, itg, theta, dtheta, mp, Sp, dmp, dSp, mu, S, dmu, dS, seen=None):
    """The interrogation and the z update of every block, in place on (mu, S, dmu, dS): (logdens term, its derivative)."""
    zero = np.zeros(W.shape[-1])
    val = dval = 0.0
    f, fd, J, Jd = tangent_fun(mp, theta, dmp, dtheta)
    for b in range(W.shape[0]):
        w = W[b, 0]
        if itg == "kramer":
            Wm, dWm = w - J[b], -Jd[b]
            a, da, V, dV = -f[b] + J[b] @ mp[b], -fd[b] + Jd[b] @ mp[b] + J[b] @ dmp[b], 0.0, 0.0
        else:
            Wm, dWm, a, da = w, zero, -f[b], -fd[b]
            V, dV = (w @ Sp[b] @ w, w @ dSp[b] @ w) if itg == "rodeo" else (0.0, 0.0)
        (mu[b], S[b]), (dmu[b], dS[b]), v, dv, s = _update(Wm, dWm, a, da, V, dV, mp[b], Sp[b], dmp[b], dSp[b])
        val, dval = val + v, dval + dv
        if seen is not None:
            seen.append(abs(s))
    return val, dval


def dalton_filter_jvp(tangent_fun, W, x0, t, itg, pairs, y, nodes, D, Om, theta, dx0, dtheta, dls, dlo, with_obs=True,
                      forecast_vars=None):
    """One trajectory, one direction: (logdens, its derivative) of DALTON's joint filter, or of the marginal one."""
    d, _, p = W.shape
    mu, S = np.array(x0, dtype=np.float64), np.zeros((d, p, p))
    dmu, dS = np.array(dx0, dtype=np.float64), np.zeros((d, p, p))
    zero = np.zeros(p)
    val = dval = 0.0
    seen = forecast_vars if forecast_vars is not None else []

    def observe(i, update):
        nonlocal val, dval
        for b in range(d):
            om = Om[i, b, 0, 0]
            new, dnew, v, dv, s = _update(D[i, b, 0], zero, -y[i, b, 0], 0.0, om, dlo[b] * om, mu[b], S[b], dmu[b], dS[b])
            if update:
                (mu[b], S[b]), (dmu[b], dS[b]) = new, dnew
            val, dval = val + v, dval + dv
            seen.append(abs(s))

    i = 0
    if len(nodes) and nodes[0] == 0:
        if with_obs:
            observe(0, False)                                        # the density alone: x_0 is not updated
        i = 1
    for n in range(len(t) - 1):
        Q, R = pairs[n]
        mp, Sp, dmp, dSp = _predict(Q, R, mu, S, dmu, dS, dls)
        v, dv = _step(tangent_fun, W, itg, theta, dtheta, mp, Sp, dmp, dSp, mu, S, dmu, dS, seen)
        val, dval = val + v, dval + dv
        if i < len(nodes) and nodes[i] == n + 1:
            if with_obs:
                observe(i, True)
            i += 1
    return val, dval


def fenrir_forward_jvp(tangent_fun, W, x0, t, itg, pairs, theta, dx0, dtheta, dls):
    """One trajectory, one direction: the filtered records and their tangents (mf (N+1, d, p), Sf (N+1, d, p, p), dmf, dSf)."""
    d, _, p = W.shape
    N = len(t) - 1
    mf, Sf, dmf, dSf = np.zeros((N + 1, d, p)), np.zeros((N + 1, d, p, p)), np.zeros((N + 1, d, p)), np.zeros((N + 1, d, p, p))
    mu, S = np.array(x0, dtype=np.float64), np.zeros((d, p, p))
    dmu, dS = np.array(dx0, dtype=np.float64), np.zeros((d, p, p))
    mf[0], dmf[0] = mu, dmu
    for n in range(N):
        Q, R = pairs[n]
        mp, Sp, dmp, dSp = _predict(Q, R, mu, S, dmu, dS, dls)
        _step(tangent_fun, W, itg, theta, dtheta, mp, Sp, dmp, dSp, mu, S, dmu, dS)
        mf[n + 1], Sf[n + 1], dmf[n + 1], dSf[n + 1] = mu, S, dmu, dS
    return mf, Sf, dmf, dSf


def fenrir_backward_jvp(mf, Sf, dmf, dSf, pairs, y, nodes, D, Om, dls, dlo, forecast_vars=None):
    """One block of one trajectory (dls, dlo: that block's two rates): (logdens, its derivative)."""
    N = len(pairs)
    zero = np.zeros(mf.shape[-1])
    val = dval = 0.0
    i = len(nodes) - 1
    bm, bS, dbm, dbS = mf[N].copy(), Sf[N].copy(), dmf[N].copy(), dSf[N].copy()

    def observe(bm, bS, dbm, dbS):
        (m, S), (dm, dS), v, dv, w = _update(D[i], zero, -y[i], 0.0, Om[i], dlo * Om[i], bm, bS, dbm, dbS)
        if forecast_vars is not None:
            forecast_vars.append(abs(w))
        return m, S, dm, dS, v, dv

    if i >= 0 and nodes[i] == N:
        bm, bS, dbm, dbS, v, dv = observe(bm, bS, dbm, dbS)
        val, dval, i = val + v, dval + dv, i - 1
    for n in range(N - 1, -1, -1):
        Q, R = pairs[n]
        mp, Sp = Q @ mf[n], Q @ Sf[n] @ Q.T + R
        dmp, dSp = Q @ dmf[n], Q @ dSf[n] @ Q.T + 2.0 * dls * R
        T, dT = Sf[n] @ Q.T, dSf[n] @ Q.T
        G = np.linalg.solve(Sp, T.T).T
        dG = np.linalg.solve(Sp, (dT - G @ dSp).T).T
        b, db = mf[n] - G @ mp, dmf[n] - dG @ mp - G @ dmp
        Cm, dC = Sf[n] - G @ T.T, dSf[n] - dG @ T.T - G @ dT.T
        dbm, dbS = dG @ bm + G @ dbm + db, dG @ bS @ G.T + G @ dbS @ G.T + G @ bS @ dG.T + dC      # (the carry before its own step)
        bm, bS = G @ bm + b, G @ bS @ G.T + Cm
        if i >= 0 and nodes[i] == n:
            bm, bS, dbm, dbS, v, dv = observe(bm, bS, dbm, dbS)
            val, dval, i = val + v, dval + dv, i - 1
    assert i == -1
    return val, dval


def _grid_jvp(which, oracle_ode, W, x0, t_grid, itg, prior_at, y, nodes, D, Om, theta, dtheta, dx0, dls, dlo, forecast_vars):
    t = np.asarray(t_grid, dtype=np.float64)
    h_rep, slot = grid_slots(t)
    slots = [tuple(np.asarray(a, dtype=np.float64) for a in prior_at(float(h))) for h in h_rep]
    W, x0, theta, y, D, Om = (np.asarray(a, dtype=np.float64) for a in (W, x0, theta, y, D, Om))
    d, _, p = W.shape[-3:]
    lead = [a.shape[0] for a, nd in ((x0, 3), (theta, 2)) if a.ndim == nd] + [a.shape[0] for pair in slots for a in pair if a.ndim == 4]
    B = lead[0] if lead else 1
    given = [(a, nd) for a, nd in ((dtheta, 2), (dx0, 3), (dls, 2), (dlo, 2)) if a is not None]
    K = given[0][0].shape[-given[0][1]]
    dtheta = np.zeros((K, theta.shape[-1])) if dtheta is None else np.asarray(dtheta, dtype=np.float64)
    dx0 = np.zeros((K, d, p)) if dx0 is None else np.asarray(dx0, dtype=np.float64)
    dls = np.zeros((K, d)) if dls is None else np.asarray(dls, dtype=np.float64)
    dlo = np.zeros((K, d)) if dlo is None else np.asarray(dlo, dtype=np.float64)
    value, dvalue = np.zeros(B), np.zeros((B, K))
    nodes = [int(k) for k in nodes]
    tf = TANGENTS[oracle_ode]
    for b in range(B):
        pick = lambda a, nd: a[b] if a.ndim == nd + 1 else a                                         # noqa: E731
        pairs = [(pick(slots[s][0], 3), pick(slots[s][1], 3)) for s in slot]
        for k in range(K):
            th, x, dth, dx, ls, lo = pick(theta, 1), pick(x0, 2), pick(dtheta, 2)[k], pick(dx0, 3)[k], pick(dls, 2)[k], pick(dlo, 2)[k]
            if which == "dalton":
                args = (tf, W, x, t, itg, pairs, y, nodes, D, Om, th, dx, dth, ls, lo)
                vj, dj = dalton_filter_jvp(*args, forecast_vars=forecast_vars)
                vm, dm = dalton_filter_jvp(*args, with_obs=False, forecast_vars=forecast_vars)
                value[b], dvalue[b, k] = vj - vm, dj - dm
            else:
                mf, Sf, dmf, dSf = fenrir_forward_jvp(tf, W, x, t, itg, pairs, th, dx, dth, ls)
                val = dval = 0.0
                for blk in range(d):                                 # (block order: the device's ordered sum)
                    mine = [(Q[blk], R[blk]) for Q, R in pairs]
                    v, dv = fenrir_backward_jvp(mf[:, blk], Sf[:, blk], dmf[:, blk], dSf[:, blk], mine, y[:, blk, 0], nodes,
                                                D[:, blk, 0], Om[:, blk, 0, 0], ls[blk], lo[blk], forecast_vars=forecast_vars)
                    val, dval = val + v, dval + dv
                value[b], dvalue[b, k] = val, dval
    return value, dvalue


def dalton_grid_jvp(oracle_ode, W, x0, t_grid, itg, prior_at, y, nodes, D, Om, theta, dtheta=None, dx0=None, dlog_sigma=None,
                    dlog_obs_var=None, forecast_vars=None):
    """``(value (B,), dvalue (B, K))`` of the DALTON restatement.  The arguments of tests/dalton_grad_oracle.py's function, and the
    two hyper directions (K, d) or (B, K, d); None is a zero direction."""
    return _grid_jvp("dalton", oracle_ode, W, x0, t_grid, itg, prior_at, y, nodes, D, Om, theta, dtheta, dx0, dlog_sigma,
                     dlog_obs_var, forecast_vars)


def fenrir_grid_jvp(oracle_ode, W, x0, t_grid, itg, prior_at, y, nodes, D, Om, theta, dtheta=None, dx0=None, dlog_sigma=None,
                    dlog_obs_var=None, forecast_vars=None):
    """The same for the Fenrir restatement."""
    return _grid_jvp("fenrir", oracle_ode, W, x0, t_grid, itg, prior_at, y, nodes, D, Om, theta, dtheta, dx0, dlog_sigma,
                     dlog_obs_var, forecast_vars)
