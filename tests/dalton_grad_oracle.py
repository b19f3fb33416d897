"""
Test helper (not collected): a literal NumPy restatement of the tangent recursion of ``dalton_grid_jvp``
(``rodeo_amd.inference.dalton``), on tests/dalton_grid_oracle.py's ``filters`` pattern -- the same steps
in the same order, one trajectory and one direction at a time, next to (mu, Sigma) the pair (mu., Sigma.):

  predict        mu.- = Q mu. ;  Sigma.- = Q Sigma. Q^T
  interrogation  rodeo / schober: a. = -f. ;  V. = W Sigma.- W^T (rodeo), 0 (schober);
                 kramer: wgt. = -J. ;  a. = -f. + J. mu- + J mu.-
  update         WS = W~ Sigma-, SW = Sigma- W~^T, s = WS W~ + V, innov = -(W~ mu- + a), K = SW / s; the product rule through all
                 of them (one-sided, not symmetrised); d(-1/2 (innov^2 / s + log s)) = -innov innov. / s + 1/2 innov^2 s. / s^2 - 1/2 s. / s,
                 and nothing where |s| <= 1e-8
  y update       the same with the constant row D and variance Omega; node 0: the density alone, differentiated in x_0.

f., J and J. of ``oracle.odes``' FitzHugh-Nagumo and Lorenz63 are written out analytically below (f. is the derivative of f
along (x., theta.) through all blocks, J. that of the block-diagonal Jacobian entries d f_b / d X[b][0]).  Nothing of the device
and nothing of tests/dalton_grid_oracle.py is used: the finite-difference test compares this file with differences of that one.
"""
import numpy as np
from oracle import odes
from rodeo_amd.grid import grid_slots

LOG_2PI = float(np.log(2.0 * np.pi))


def fhn_tangent(x, th, dx, dth):
    """(f, f., J, J.) of FitzHugh-Nagumo at x (d, p), theta = (a, b, c), along (dx, dth); J, J. (d, p) hold column 0 only."""
    (a, b, c), (da, db, dc) = th, dth
    V, R, dV, dR = x[0, 0], x[1, 0], dx[0, 0], dx[1, 0]
    f = np.array([c * (V - V ** 3 / 3 + R), -(V - a + b * R) / c])
    fd = np.array([dc * (V - V ** 3 / 3 + R) + c * ((1 - V * V) * dV + dR),
                   -(dV - da + db * R + b * dR) / c + (V - a + b * R) * dc / c ** 2])
    J, Jd = np.zeros_like(x), np.zeros_like(x)
    J[0, 0], J[1, 0] = c * (1 - V * V), -b / c
    Jd[0, 0], Jd[1, 0] = dc * (1 - V * V) - 2 * c * V * dV, -db / c + b * dc / c ** 2
    return f, fd, J, Jd


def lorenz_tangent(x, th, dx, dth):
    """(f, f., J, J.) of Lorenz63 at x (3, p), theta = (rho, sigma, beta)."""
    (rho, sig, beta), (drho, dsig, dbeta) = th, dth
    (X, Y, Z), (dX, dY, dZ) = x[:, 0], dx[:, 0]
    f = np.array([-sig * X + sig * Y, rho * X - Y - X * Z, -beta * Z + X * Y])
    fd = np.array([dsig * (Y - X) + sig * (dY - dX), drho * X + rho * dX - dY - dX * Z - X * dZ, -dbeta * Z - beta * dZ + dX * Y + X * dY])
    J, Jd = np.zeros_like(x), np.zeros_like(x)
    J[:, 0] = [-sig, -1.0, -beta]
    Jd[:, 0] = [-dsig, 0.0, -dbeta]
    return f, fd, J, Jd


def fhn_init_jac(v0, theta, p):
    """d x0 / d theta (d, p, 3) of the quick start's initial state x0 = [v0, f(v0, theta), 0, ...] (``first_order_pad``)."""
    (a, b, c), (V, R) = theta, v0
    J = np.zeros((2, p, 3))
    J[0, 1, 2] = V - V ** 3 / 3 + R
    J[1, 1] = [1.0 / c, -R / c, (V - a + b * R) / c ** 2]
    return J


TANGENTS = {odes.fitzhugh_nagumo: fhn_tangent, odes.lorenz63: lorenz_tangent}


def _update(W, dW, a, da, V, dV, mp, Sp, dmp, dSp):
    """One scalar measurement 0 = W x + a + N(0, V): ((mu, Sigma), (mu., Sigma.), logdens term, its derivative)."""
    WS, SW = W @ Sp, Sp @ W
    s = WS @ W + V
    innov = -(W @ mp + a)
    K = SW / s
    dWS, dSW = dW @ Sp + W @ dSp, dSp @ W + Sp @ dW
    ds = dWS @ W + WS @ dW + dV
    dinnov = -(dW @ mp + W @ dmp + da)
    dK = (dSW - K * ds) / s
    mu, S = mp + K * innov, Sp - np.outer(K, WS)
    dmu, dS = dmp + dK * innov + K * dinnov, dSp - np.outer(dK, WS) - np.outer(K, dWS)
    if abs(s) > 1e-8:
        val = -0.5 * (innov * innov / s + np.log(s)) - 0.5 * LOG_2PI
        dval = -innov * dinnov / s + 0.5 * innov * innov * ds / s ** 2 - 0.5 * ds / s
    else:
        val = dval = 0.0
    return (mu, S), (dmu, dS), val, dval, s


def filter_jvp(tangent_fun, W, x0, t, itg, pairs, y, nodes, D, Om, theta, dx0, dtheta, with_obs=True, forecast_vars=None):
    """One trajectory, one direction: (logdens, its derivative) of the joint filter, or of the marginal one (``with_obs=False``).
    W (d, 1, p); pairs[n] = (Q, R) (d, p, p) of step n; y (n_obs, d, 1), D (n_obs, d, 1, p), Om (n_obs, d, 1, 1); nodes increasing."""
    d, _, p = W.shape
    mu, S = np.array(x0, dtype=np.float64), np.zeros((d, p, p))
    dmu, dS = np.array(dx0, dtype=np.float64), np.zeros((d, p, p))
    zero = np.zeros(p)
    val = dval = 0.0
    seen = forecast_vars if forecast_vars is not None else []
    i = 0
    if len(nodes) and nodes[0] == 0:
        if with_obs:
            for b in range(d):
                _, _, v, dv, s = _update(D[0, b, 0], zero, -y[0, b, 0], 0.0, Om[0, b, 0, 0], 0.0, mu[b], S[b], dmu[b], dS[b])
                val, dval = val + v, dval + dv
                seen.append(abs(s))
        i = 1
    for n in range(len(t) - 1):
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
            (mu[b], S[b]), (dmu[b], dS[b]), v, dv, s = _update(Wm, dWm, a, da, V, dV, mp[b], Sp[b], dmp[b], dSp[b])
            val, dval = val + v, dval + dv
            seen.append(abs(s))
        if i < len(nodes) and nodes[i] == n + 1:
            if with_obs:
                for b in range(d):
                    (mu[b], S[b]), (dmu[b], dS[b]), v, dv, s = _update(D[i, b, 0], zero, -y[i, b, 0], 0.0, Om[i, b, 0, 0], 0.0, mu[b],
                                                                     S[b], dmu[b], dS[b])
                    val, dval = val + v, dval + dv
                    seen.append(abs(s))
            i += 1
    return val, dval


def dalton_grid_jvp(oracle_ode, W, x0, t_grid, itg, prior_at, y, nodes, D, Om, theta, dtheta=None, dx0=None, forecast_vars=None):
    """``(value (B,), dvalue (B, K))`` of the restatement: joint - marginal and its derivative along every direction.  x0 (d, p) or
    (B, d, p), theta (n,) or (B, n), what ``prior_at`` returns (d, p, p) or (B, d, p, p); dtheta (K, n) or (B, K, n), dx0 (K, d, p)
    or (B, K, d, p), None for zero.  ``itg`` is "rodeo", "schober" or "kramer"."""
    t = np.asarray(t_grid, dtype=np.float64)
    h_rep, slot = grid_slots(t)
    slots = [tuple(np.asarray(a, dtype=np.float64) for a in prior_at(float(h))) for h in h_rep]
    W, x0, theta = (np.asarray(a, dtype=np.float64) for a in (W, x0, theta))
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
            args = (TANGENTS[oracle_ode], W, pick(x0, 2), t, itg, pairs, y, nodes, D, Om, pick(theta, 1), pick(dx0, 3)[k],
                    pick(dtheta, 2)[k])
            vj, dj = filter_jvp(*args, forecast_vars=forecast_vars)
            vm, dm = filter_jvp(*args, with_obs=False, forecast_vars=forecast_vars)
            value[b], dvalue[b, k] = vj - vm, dj - dm
    return value, dvalue
