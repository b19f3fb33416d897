"""
``rodeo.inference.magi`` (src/rodeo/inference/magi.py:6-99): ``magi_logdens``, the log-density of the MAGI approximation
p(X_{0:N}, Z = 0 | params, prior_pars).  ``ode_expand(ode_data_subset, **params)`` builds the full solution process
X_{0:N} (N+1, d, p) on the host; the device (``rk_magi_logdens``, ``csrc/magi.hip``) runs, per block, the Kalman filter of
the prior that starts from the known X_0 and measures the first ``n_active`` components of X_{1:N} exactly (W =
eye(n_active, p), no noise), and adds up the forecast log-densities.  The density is the plain Gaussian one of
``jax.scipy.stats.multivariate_normal.logpdf`` (Cholesky of the forecast variance), not the eigenvalue rule with its 1e-8
cut-off that ``fenrir`` and ``dalton`` use (utils.py:60-78).  Only X_0 and the measured components go to the device.

Same signature as the reference (``kalman_type`` has no default).  ``"standard"``: the LU gain of standard.py:93-102;
``"square-root"``: square_root.py, ``prior_pars[1]`` is a lower factor.  Served: n_deriv p in 2..6 (standard) or 2..7
(square-root), n_active in 1..p, any number of blocks d; a larger p spills the lane kernel's registers.  Refused
before any device work: an unknown ``kalman_type`` (NotImplementedError), p outside the served range
(NotImplementedError), n_active outside 1..p, ``prior_pars`` not of shape (d, p, p), an ``ode_expand`` result not of shape
(N+1, d, p), inconsistent batch sizes (ValueError).

Which form to trust: with n_active >= 2 and a coupled Q (any prior whose Q is not diagonal, IBM priors included), the
reference's standard form loses the symmetry of its covariance from step to step (its update Sigma- - K W Sigma- acts on
one side only) and amplifies the rounding: over tens to hundreds of steps the value leaves the true log-density, by
percents, also at n_active = p.  This build computes the reference's formula as it is, so it does the same.  Use
``"square-root"`` there; n_active = 1 or a diagonal Q is safe in both forms (tests/test_oracle_magi.py).

Batched extension, in the style of ``fenrir`` / ``dalton``: ``ode_data_subset`` (B, N+1, d, k), ``prior_pars`` (B, d, p, p)
and any ``**params`` entry of shape (B, n) may carry one leading batch axis; the result is then an array (B,), else a
float.  ``ode_expand`` is host code: it is called once per batch item with that item's data and params, and once only
when nothing but the prior is batched (that state then serves every prior).  The rule for ``**params`` is the solver's for
ODE parameters: a scalar or 1-D entry is shared, a 2-D entry is (B, n) and batched, more dimensions are refused.  A
parameter that is itself a matrix (shared by every item) does not go through ``**params``: bind it into ``ode_expand``
(``functools.partial(expand, A=A)``), so that only batched and vector parameters are passed by keyword.
"""
import ctypes as C
import numpy as np
from .. import _lib
from ..device import default_device, batch_minor

_KALMAN = {"standard": _lib.KALMAN_STANDARD, "square-root": _lib.KALMAN_SQRT}
P_MIN = 2
P_MAX = {"standard": 6, "square-root": 7}    # beyond, the lane kernel spills to scratch (csrc/magi.hip)


def _batch_axes(data, Q, R, params):
    """The batch size B (None if nothing is batched), whether the data / params need one ode_expand call per item."""
    sizes = {}
    if data.ndim == 4:
        sizes["ode_data_subset"] = data.shape[0]
    elif data.ndim != 3:
        raise ValueError(f"magi: ode_data_subset must have shape (N+1, d, k) or (B, N+1, d, k), got {data.shape}")
    for name, a in (("prior_pars[0]", Q), ("prior_pars[1]", R)):
        if a.ndim == 4:
            sizes[name] = a.shape[0]
    per_item = data.ndim == 4
    for k, v in params.items():
        nd = np.ndim(v)
        if nd > 2:
            raise ValueError(f"magi: params entry '{k}' must have shape (n,) or (B, n), got {np.shape(v)}; bind a shared "
                             f"matrix parameter into ode_expand (functools.partial) instead")
        if nd == 2:
            sizes[k] = np.shape(v)[0]
            per_item = True
    if len(set(sizes.values())) > 1:
        raise ValueError(f"magi: inconsistent batch sizes {sizes}")
    return (next(iter(sizes.values())) if sizes else None), per_item


def magi_logdens(ode_data_subset, ode_expand, n_active, prior_pars, kalman_type, **params):
    """log p(ode_data_subset, Z = 0 | params, prior_pars) (magi.py:6-99): a float, or an array (B,) for batched inputs."""
    if kalman_type not in _KALMAN:
        raise NotImplementedError                                   # magi.py:29-34
    data = np.asarray(ode_data_subset)
    Q = np.asarray(prior_pars[0], dtype=np.float64)
    R = np.asarray(prior_pars[1], dtype=np.float64)
    B, per_item = _batch_axes(data, Q, R, params)
    n1, d = data.shape[-3], data.shape[-2]
    p = Q.shape[-1] if Q.ndim >= 1 else 0
    for name, a in (("prior_pars[0]", Q), ("prior_pars[1]", R)):
        if a.ndim not in (3, 4) or a.shape[-3:] != (d, p, p):
            raise ValueError(f"magi: {name} must have shape (d, p, p) = ({d}, p, p) [+ a leading batch axis], got {a.shape}")
    if not P_MIN <= p <= P_MAX[kalman_type]:
        raise NotImplementedError(f"magi on the device: n_deriv in {P_MIN}..{P_MAX[kalman_type]} for kalman_type "
                                  f"'{kalman_type}' (beyond, the lane kernel spills its registers), got {p}")
    n_active = int(n_active)
    if not 1 <= n_active <= p:
        raise ValueError(f"magi: n_active must be in 1..{p}, got {n_active}")
    N = n1 - 1

    def expand(i):
        di = data[i] if data.ndim == 4 else data
        pi = {k: (v[i] if np.ndim(v) == 2 else v) for k, v in params.items()} if i is not None else params
        st = np.asarray(ode_expand(di, **pi), dtype=np.float64)
        if st.shape != (n1, d, p):
            raise ValueError(f"magi: ode_expand must return shape (N+1, d, p) = ({n1}, {d}, {p}), got {st.shape}")
        return st

    if per_item:
        states = np.stack([expand(i) for i in range(B)])            # (B, N+1, d, p)
        x0, xm = states[:, 0], states[:, 1:, :, :n_active]
    else:
        st = expand(None)
        x0, xm = st[0], st[1:, :, :n_active]
    dev = default_device()
    d_x0 = dev.to_device(batch_minor(x0, per_item))
    d_xm = dev.to_device(batch_minor(xm, per_item))
    d_Q = dev.to_device(batch_minor(Q, Q.ndim == 4))
    d_R = dev.to_device(batch_minor(R, R.ndim == 4))
    nb = B if B is not None else 1
    cfg = _lib.MagiCfg(n_traj=nb, n_steps=N, n_block=d, n_bstate=p, n_active=n_active, kalman_type=_KALMAN[kalman_type])
    inp = _lib.MagiIn(x0=d_x0.ptr, x0_batched=int(per_item), x_meas=d_xm.ptr, x_meas_batched=int(per_item),
                      prior_weight=d_Q.ptr, prior_weight_batched=int(Q.ndim == 4),
                      prior_var=d_R.ptr, prior_var_batched=int(R.ndim == 4))
    out = dev.empty((nb,))
    _lib.check(dev.lib.rk_magi_logdens(dev.h, C.byref(cfg), C.byref(inp), out.ptr))
    ll = out.to_host()
    return ll if B is not None else float(ll[0])
