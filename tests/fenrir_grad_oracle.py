"""
Test helper (not collected): a literal NumPy restatement of the tangent recursion of ``fenrir_grid_jvp``
(``rodeo_amd.inference.fenrir``), one trajectory and one direction at a time, next to every primal
quantity its derivative along the direction (a trailing d marks it below):

  forward   the data-free filter of tests/dalton_grad_oracle.py's step -- predict, interrogate (rodeo / schober / kramer), update
            by ``_update`` -- whose log-density terms are discarded; (mu_f, Sigma_f) and (mu_f d, Sigma_f d) of every node are
            kept; node 0: (ode_init, 0) with tangent (the ode_init direction, 0)
  backward  the carry starts at node N's filtered record and its tangent; for n = N-1 .. 0 with the pair (Q, R) of step n:
            mu- = Q mu_f, Sigma- = Q Sigma_f Q^T + R             mu- d = Q mu_f d, Sigma- d = Q Sigma_f d Q^T
            T = Sigma_f Q^T, G = T (Sigma-)^-1                   Td = Sigma_f d Q^T, Gd = (Td - G Sigma- d) (Sigma-)^-1
            b = mu_f - G mu-                                     bd = mu_f d - Gd mu- - G mu- d
            C = Sigma_f - G T^T                                  Cd = Sigma_f d - Gd T^T - G Td^T
            m <- G m + b,  S <- G S G^T + C                      md <- Gd m + G md + bd,  Sd <- Gd S G^T + G Sd G^T + G S Gd^T + Cd
            (both solves are LU solves on Sigma- with the transposed right-hand side, as the kernels do them), and where node n is
            observed -- node 0 and node N like any other -- the scalar measurement y = D x + N(0, Omega) by ``_update`` with the
            row D, a = -y, V = Omega: its log-density term and that term's derivative are added, nothing where |w| <= 1e-8.

``_update`` and the analytic f., J, J. of the two systems are tests/dalton_grad_oracle.py's.  Nothing of the device and nothing of
tests/fenrir_grid_oracle.py is used: the finite-difference test compares this file with differences of that one.
"""
import numpy as np
from rodeo_amd.grid import grid_slots
from dalton_grad_oracle import _update, TANGENTS, fhn_tangent, lorenz_tangent, fhn_init_jac   # noqa: F401  (re-exported for the tests)


def forward_jvp(tangent_fun, W, x0, t, itg, pairs, theta, dx0, dtheta):
    """One trajectory, one direction: the filtered records and their tangents, (mf (N+1, d, p), Sf (N+1, d, p, p), dmf, dSf)."""
    d, _, p = W.shape
    N = len(t) - 1
    mf, Sf, dmf, dSf = np.zeros((N + 1, d, p)), np.zeros((N + 1, d, p, p)), np.zeros((N + 1, d, p)), np.zeros((N + 1, d, p, p))
    mu, S = np.array(x0, dtype=np.float64), np.zeros((d, p, p))
    dmu, dS = np.array(dx0, dtype=np.float64), np.zeros((d, p, p))
    mf[0], dmf[0] = mu, dmu
    zero = np.zeros(p)
    for n in range(N):
        Q, R = pairs[n]
        mp, Sp = np.einsum("bij,bj->bi", Q, mu), Q @ S @ np.swapaxes(Q, -1, -2) + R
        dmp, dSp = np.einsum("bij,bj->bi", Q, dmu), Q @ dS @ np.swapaxes(Q, -1, -2)
        f, fd, J, Jd = tangent_fun(mp, theta, dmp, dtheta)
        for b in range(d):
            w = W[b, 0]
            if itg == "kramer":
                Wm, dWm = w - J[b], -Jd[b]
                a, da, V, dV = -f[b] + J[b] @ mp[b], -fd[b] + Jd[b] @ mp[b] + J[b] @ dmp[b], 0.0, 0.0
            else:
                Wm, dWm, a, da = w, zero, -f[b], -fd[b]
                V, dV = (w @ Sp[b] @ w, w @ dSp[b] @ w) if itg == "rodeo" else (0.0, 0.0)
            (mu[b], S[b]), (dmu[b], dS[b]), _, _, _ = _update(Wm, dWm, a, da, V, dV, mp[b], Sp[b], dmp[b], dSp[b])
        mf[n + 1], Sf[n + 1], dmf[n + 1], dSf[n + 1] = mu, S, dmu, dS
    return mf, Sf, dmf, dSf


def backward_jvp(mf, Sf, dmf, dSf, pairs, y, nodes, D, Om, forecast_vars=None):
    """One block of one trajectory: records (N+1, p[, p]), pairs[n] = (Q, R) (p, p), y (n_obs,), D (n_obs, p), Om (n_obs,).  Returns
    (logdens, its derivative)."""
    N = len(pairs)
    p = mf.shape[-1]
    zero = np.zeros(p)
    val = dval = 0.0
    i = len(nodes) - 1
    bm, bS, dbm, dbS = mf[N].copy(), Sf[N].copy(), dmf[N].copy(), dSf[N].copy()

    def observe(bm, bS, dbm, dbS):
        (m, S), (dm, dS), v, dv, w = _update(D[i], zero, -y[i], 0.0, Om[i], 0.0, bm, bS, dbm, dbS)
        if forecast_vars is not None:
            forecast_vars.append(abs(w))
        return m, S, dm, dS, v, dv

    if i >= 0 and nodes[i] == N:
        bm, bS, dbm, dbS, v, dv = observe(bm, bS, dbm, dbS)
        val, dval, i = val + v, dval + dv, i - 1
    for n in range(N - 1, -1, -1):
        Q, R = pairs[n]
        mp, Sp = Q @ mf[n], Q @ Sf[n] @ Q.T + R
        dmp, dSp = Q @ dmf[n], Q @ dSf[n] @ Q.T
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


def fenrir_grid_jvp(oracle_ode, W, x0, t_grid, itg, prior_at, y, nodes, D, Om, theta, dtheta=None, dx0=None, forecast_vars=None):
    """``(value (B,), dvalue (B, K))`` of the restatement.  x0 (d, p) or (B, d, p), theta (n,) or (B, n), what ``prior_at`` returns
    (d, p, p) or (B, d, p, p); dtheta (K, n) or (B, K, n), dx0 (K, d, p) or (B, K, d, p), None for zero; y (n_obs, d, 1), D (n_obs, d,
    1, p), Om (n_obs, d, 1, 1) on the strictly increasing ``nodes``.  ``itg`` is "rodeo", "schober" or "kramer".  ``forecast_vars``: a
    list that receives every y forecast variance."""
    t = np.asarray(t_grid, dtype=np.float64)
    h_rep, slot = grid_slots(t)
    slots = [tuple(np.asarray(a, dtype=np.float64) for a in prior_at(float(h))) for h in h_rep]
    W, x0, theta, y, D, Om = (np.asarray(a, dtype=np.float64) for a in (W, x0, theta, y, D, Om))
    d, _, p = W.shape[-3:]
    lead = [a.shape[0] for a, nd in ((x0, 3), (theta, 2)) if a.ndim == nd] + [a.shape[0] for pair in slots for a in pair if a.ndim == 4]
    B = lead[0] if lead else 1
    K = (dtheta if dtheta is not None else dx0).shape[-2 if dtheta is not None else -3]
    dtheta = np.zeros((K, theta.shape[-1])) if dtheta is None else np.asarray(dtheta, dtype=np.float64)
    dx0 = np.zeros((K, d, p)) if dx0 is None else np.asarray(dx0, dtype=np.float64)
    value, dvalue = np.zeros(B), np.zeros((B, K))
    nodes = [int(k) for k in nodes]
    for b in range(B):
        pick = lambda a, nd: a[b] if a.ndim == nd + 1 else a                                         # noqa: E731
        pairs = [(pick(slots[s][0], 3), pick(slots[s][1], 3)) for s in slot]
        for k in range(K):
            mf, Sf, dmf, dSf = forward_jvp(TANGENTS[oracle_ode], W, pick(x0, 2), t, itg, pairs, pick(theta, 1), pick(dx0, 3)[k],
                                           pick(dtheta, 2)[k])
            val = dval = 0.0
            for blk in range(d):                                     # (block order: the device's ordered sum)
                mine = [(Q[blk], R[blk]) for Q, R in pairs]
                v, dv = backward_jvp(mf[:, blk], Sf[:, blk], dmf[:, blk], dSf[:, blk], mine, y[:, blk, 0], nodes, D[:, blk, 0],
                                     Om[:, blk, 0, 0], forecast_vars=forecast_vars)
                val, dval = val + v, dval + dv
            value[b], dvalue[b, k] = val, dval
    return value, dvalue
