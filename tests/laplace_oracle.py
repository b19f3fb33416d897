"""
TEST INFRASTRUCTURE: NumPy restatement of the device pieces of rodeo_amd.inference.laplace (csrc/laplace_kernels.hpp): the
order of the S = 2 k^2 + 1 stencil points, the difference formulas with their order of operations, and the damped Newton
step.  float64 throughout; nothing here is imported by the product.
"""
import numpy as np


def n_stencil(k):
    return 2 * k * k + 1


def pairs(k):
    """The pairs i < j in row-major order."""
    return [(i, j) for i in range(k) for j in range(i + 1, k)]


def stencil(u, step):
    """u (C, k), step (k,) -> (C, S, k): u;  u +- h_i e_i (i ascending, + first);  u +- h_i e_i +- h_j e_j for the pairs
    i < j in row-major order, signs (+,+), (+,-), (-,+), (-,-)."""
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    n_c, k = u.shape
    out = np.repeat(u[:, None, :], n_stencil(k), axis=1)
    s = 1
    for i in range(k):
        out[:, s, i] += step[i]
        out[:, s + 1, i] -= step[i]
        s += 2
    for i, j in pairs(k):
        for si in (1.0, -1.0):
            for sj in (1.0, -1.0):
                out[:, s, i] += si * step[i]
                out[:, s, j] += sj * step[j]
                s += 1
    assert s == n_stencil(k)
    return out


def grad_hess(vals, step):
    """vals (C, S), step (k,) -> grad (C, k), hess (C, k, k), n_bad (C,), with the device's order of operations."""
    vals = np.atleast_2d(np.asarray(vals, dtype=np.float64))
    n_c, S = vals.shape
    k = len(step)
    assert S == n_stencil(k)
    grad, hess = np.empty((n_c, k)), np.empty((n_c, k, k))
    f0 = vals[:, 0]
    with np.errstate(invalid="ignore"):
        for i in range(k):
            fp, fm = vals[:, 1 + 2 * i], vals[:, 2 + 2 * i]
            grad[:, i] = (fp - fm) / (2.0 * step[i])
            hess[:, i, i] = ((fp - f0) + (fm - f0)) / (step[i] * step[i])
        for q, (i, j) in enumerate(pairs(k)):
            g = vals[:, 1 + 2 * k + 4 * q:1 + 2 * k + 4 * q + 4]
            hess[:, i, j] = ((g[:, 0] - g[:, 1]) - (g[:, 2] - g[:, 3])) / ((4.0 * step[i]) * step[j])
            hess[:, j, i] = hess[:, i, j]
    n_bad = np.sum(~np.isfinite(vals), axis=1)
    grad[n_bad > 0] = np.nan
    hess[n_bad > 0] = np.nan
    return grad, hess, n_bad


def newton_step(grad, hess, damping):
    """delta = (-hess + damping I)^-1 grad, logdet = log det(-hess + damping I), ok; NaN and ok = False where the Cholesky
    factor does not exist."""
    n_c, k = grad.shape
    delta, logdet, ok = np.full((n_c, k), np.nan), np.full(n_c, np.nan), np.zeros(n_c, bool)
    for c in range(n_c):
        A = -hess[c] + damping[c] * np.eye(k)
        if not np.all(np.isfinite(A)):
            continue
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            continue
        ok[c] = True
        delta[c] = np.linalg.solve(L.T, np.linalg.solve(L, grad[c]))
        logdet[c] = 2.0 * np.sum(np.log(np.diag(L)))
    return delta, logdet, ok


def quadratic(k, n_c, seed):
    """A random concave quadratic logpost(u) = c0 - 1/2 (u - m)^T A (u - m) (A SPD, eigenvalues in [0.5, 4]) and starts."""
    rng = np.random.default_rng(seed)
    Qm, _ = np.linalg.qr(rng.standard_normal((k, k)))
    A = (Qm * rng.uniform(0.5, 4.0, k)) @ Qm.T
    A = 0.5 * (A + A.T)
    m = rng.standard_normal(k)
    c0 = float(rng.standard_normal())
    starts = m + rng.standard_normal((n_c, k))

    def logpost(u):
        d = np.asarray(u) - m
        return c0 - 0.5 * np.einsum("bi,ij,bj->b", d, A, d)
    return A, m, c0, starts, logpost
