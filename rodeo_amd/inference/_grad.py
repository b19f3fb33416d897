"""
What the device gradients of ``dalton.py`` and ``fenrir.py`` share: what is served and
refused, the staging of the directions -- the ODE parameters', ``ode_init``'s and the two reserved log-scales' -- in the library's
batch-minor convention, and ``*_grid_grad``'s unit directions and gradient dict.  Nothing here touches a device.  ``dalton.py``
re-imports the names that were reached through it, and keeps ``_stage_all``, which tests observe through that module.
"""
import numpy as np
from .. import _lib
from ..solve import _interrogate_id

_GRAD_BSTATE = (2, 3)                                               # (dalton_grad.hip: dalton_grad_pmax)
_GRAD_STATE_MAX = 27                                                # n_block n_bstate^2 of the largest instance that ships
# arguments of the call that are no parameter of the ODE: a derivative with respect to one of them is not built
_GRAD_NOT_WRT = ("sigma", "prior", "prior_pars", "prior_at", "ode_weight", "obs_data", "obs_weight", "obs_var", "obs_times",
                 "t_grid")
# The two reserved direction names, shape (K, d) / (B, K, d): the rate of log sigma_b, the prior scale
# of block b (every step's R_b gets 2 rate R_b, Q nothing, the initial variance nothing), and the rate of a common log-scale of
# block b's observation variances.  A name in ``params`` wins over the reserved meaning.
_GRAD_HYPER = ("log_sigma", "log_obs_var")


def _grad_ode(who, ode_fun, W, params):
    """The right-hand side the gradient kernels run: a built-in one that has its scalar-generic form, or the gradient kind of a
    traced Python function (``rodeo_amd.trace.grad_from_python``: registered with the library, no device work)."""
    from ..trace import grad_from_python
    rid = getattr(ode_fun, "rhs_id", None)
    if rid in (_lib.RHS_FITZHUGH_NAGUMO, _lib.RHS_LORENZ63) or getattr(ode_fun, "grad_kind", False):
        return ode_fun
    if getattr(ode_fun, "traced_from", None) is not None:             # rodeo_amd.ode.from_python's
        fun, n_vars, n_used, spec = ode_fun.traced_from
        return grad_from_python(fun, n_vars, n_used, **dict(spec))
    if rid is None and callable(ode_fun):                           # a plain Python function: solve._device_ode's sizes
        sizes = {k: int(np.shape(v)[-1]) if np.ndim(v) >= 1 else 1 for k, v in params.items()}
        return grad_from_python(ode_fun, int(W[-3]), int(W[-1]), **sizes)
    raise NotImplementedError(f"{who}: not built: the right-hand side {getattr(ode_fun, 'name', ode_fun)!r} (fitzhugh_nagumo, "
                              "lorenz63, or a traced Python function)")


def _grad_config(who, ode_fun, ode_weight, interrogate, kalman_type, obs_weight, names, params, sibling="dalton_grid"):
    """What the gradient kernels do not serve (NotImplementedError, "not built") and the names a derivative is asked for
    (ValueError for an unknown one), before any device work.  Returns the right-hand side to run (``_grad_ode``).  ``sibling``
    names the value call whose kernel is the yardstick of the size limit (``fenrir.py`` passes its own)."""
    if kalman_type != "standard":
        raise NotImplementedError(f"{who}: not built: kalman_type {kalman_type!r} (the standard form only)")
    if _interrogate_id(interrogate)[0] == _lib.INTERROGATE_CHKREBTII:
        raise NotImplementedError(f"{who}: not built: interrogate_chkrebtii (rodeo, schober, kramer)")
    W = np.shape(ode_weight)
    if len(W) not in (3, 4):
        raise ValueError("ode_weight must have shape (n_block, n_bmeas, n_bstate) [+ a leading batch axis]")
    if W[-2] != 1:
        raise NotImplementedError(f"{who}: not built: n_bmeas = {W[-2]} (1 only)")
    if np.ndim(obs_weight) == 4 and np.shape(obs_weight)[2] != 1:
        raise NotImplementedError(f"{who}: not built: n_bobs = {np.shape(obs_weight)[2]} (1 only: the derivative of the "
                                  "eigendecomposition's cut-off density is out of scope)")
    if not _GRAD_BSTATE[0] <= W[-1] <= _GRAD_BSTATE[1]:
        raise NotImplementedError(f"{who}: not built: n_bstate = {W[-1]} ({_GRAD_BSTATE[0]} .. {_GRAD_BSTATE[1]}: beyond, the kernel "
                                  f"needs more scratch than {sibling}'s)")
    if W[-3] * W[-1] ** 2 > _GRAD_STATE_MAX:
        raise NotImplementedError(f"{who}: not built: {W[-3]} blocks at n_bstate = {W[-1]} (n_block n_bstate^2 <= {_GRAD_STATE_MAX})")
    ode = _grad_ode(who, ode_fun, W, params)
    for name in names:
        if name in _GRAD_NOT_WRT and name not in params:
            raise NotImplementedError(f"{who}: not built: a derivative with respect to {name!r} (the ODE parameters and "
                                      "'ode_init' only)")
        if name != "ode_init" and name not in params and name not in _GRAD_HYPER:
            raise ValueError(f"{who}: {name!r} is no parameter of this call (known: {sorted(params) + ['ode_init'] + list(_GRAD_HYPER)})")
    return ode


def _split_hyper(tangents, params):
    """``tangents`` as (the ODE parameters' and ode_init's, the reserved hyper names'): a name in ``params`` is a parameter."""
    hyper = {name: v for name, v in tangents.items() if name in _GRAD_HYPER and name not in params}
    return {name: v for name, v in tangents.items() if name not in hyper}, hyper


def _stage_hyper(who, hyper, B, batched, d, K):
    """The hyper directions checked and batch-minor: ``(K, dlog_sigma, its batched flag, dlog_obs_var, its batched flag)`` with an
    array (K, d) or (K, d, B), None for a missing name.  ``K``: the count of the other directions, None when there is none."""
    out = []
    for name in _GRAD_HYPER:
        if name not in hyper:
            out += [None, 0]
            continue
        a = _direction(who, name, hyper[name], B, batched, (d,))
        k = a.shape[a.ndim - 2]
        if K is not None and k != K:
            raise ValueError(f"{who}: the directions must agree in their count K, got {sorted({K, k})}")
        K = k
        if K == 0:
            raise ValueError(f"{who}: no direction given (K = 0)")
        out += [np.ascontiguousarray(a), 0] if a.ndim == 2 else [np.ascontiguousarray(np.moveaxis(a, 0, -1)), 1]
    return (K,) + tuple(out)


def _direction(who, name, v, B, batched, tail):
    """One entry of ``tangents`` as float64 ``(K, *tail)`` or ``(B, K, *tail)``, or the ValueError."""
    try:
        a = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: the direction {name!r} is no array of numbers") from None
    nt = len(tail)
    if a.ndim not in (nt + 1, nt + 2) or a.shape[a.ndim - nt:] != tail or (a.ndim == nt + 2 and (not batched or a.shape[0] != B)):
        raise ValueError(f"{who}: the direction {name!r} must have shape (K, {', '.join(map(str, tail))})" +
                         (f" or ({B}, K, {', '.join(map(str, tail))})" if batched else "") + f", got {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{who}: the direction {name!r} holds a non-finite value")
    return a


def _stage_directions(who, ode, tangents, B, batched, d, p):
    """``tangents`` checked and in the library's batch-minor convention: ``(K, dtheta, dtheta_batched, dinit, dinit_batched)`` with
    dtheta (K, n_theta) or (K, n_theta, B), dinit (K, d, p) or (K, d, p, B), and None for an argument without a direction."""
    dirs = {}
    for name, v in tangents.items():
        tail = (d, p) if name == "ode_init" else (dict(ode.param_spec)[name],)
        dirs[name] = _direction(who, name, v, B, batched, tail)
    counts = {a.shape[a.ndim - (3 if name == "ode_init" else 2)] for name, a in dirs.items()}
    if len(counts) != 1:
        raise ValueError(f"{who}: the directions must agree in their count K, got {sorted(counts)}" if counts else
                         f"{who}: no direction given (K = 0)")
    K = counts.pop()
    if K == 0:
        raise ValueError(f"{who}: no direction given (K = 0)")

    def minor(a, nt):                                               # (K, ...) as it is, (B, K, ...) -> (K, ..., B)
        return (np.ascontiguousarray(a), 0) if a.ndim == nt + 1 else (np.ascontiguousarray(np.moveaxis(a, 0, -1)), 1)

    dtheta = (None, 0)
    par = [name for name, _ in ode.param_spec if name in dirs]
    if par:
        any_b = any(dirs[name].ndim == 3 for name in par)
        parts = []
        for name, size in ode.param_spec:
            a = dirs.get(name)
            a = np.zeros((K, size)) if a is None else a
            parts.append(np.broadcast_to(a, (B, K, size)) if any_b else a)
        dtheta = minor(np.concatenate(parts, axis=-1), 1)
    dinit = minor(dirs["ode_init"], 2) if "ode_init" in dirs else (None, 0)
    return (K,) + dtheta + dinit


def _unit_directions(who, ode_fun, ode_weight, ode_init, wrt, init_jac, params):
    """``dalton_grid_grad``'s directions: the unit directions of every name in ``wrt``, with ``init_jac[name]`` (d, p, size) or
    (B, d, p, size) as that parameter's ``ode_init`` direction.  Returns (tangents, [(name, first direction, shape)])."""
    wrt = (wrt,) if isinstance(wrt, str) else tuple(wrt)
    if len(set(wrt)) != len(wrt):
        raise ValueError(f"{who}: a name occurs twice in wrt {wrt}")
    init_jac = dict(init_jac or {})
    d, p = (int(n) for n in np.shape(ode_init)[-2:]) if np.ndim(ode_init) >= 2 else (0, 0)
    shapes = []
    for name in wrt:
        if name == "ode_init":
            shapes.append((name, (d, p)))
        elif name in params:
            shapes.append((name, (int(np.shape(params[name])[-1]) if np.ndim(params[name]) else 1,)))
        elif name in _GRAD_HYPER:
            shapes.append((name, (d,)))
        else:
            shapes.append((name, (0,)))                             # (_grad_config raises for it)
    for name in init_jac:
        if name not in wrt or name == "ode_init" or name not in params:
            raise ValueError(f"{who}: init_jac[{name!r}] belongs to no parameter in wrt {wrt}")
    K = sum(int(np.prod(s)) for _, s in shapes)
    tangents, layout, k0 = {}, [], 0
    jacs = {}
    for name, shape in shapes:
        size = int(np.prod(shape))
        if name in init_jac:
            try:
                J = np.asarray(init_jac[name], dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: init_jac[{name!r}] is no array of numbers") from None
            if J.ndim not in (3, 4) or J.shape[-3:] != (d, p, size):
                raise ValueError(f"{who}: init_jac[{name!r}] must have shape ({d}, {p}, {size}) [+ a leading batch axis], got {J.shape}")
            jacs[name] = J
    lead = {J.shape[0] for J in jacs.values() if J.ndim == 4}
    if len(lead) > 1:
        raise ValueError(f"{who}: the init_jac entries disagree in their batch size {sorted(lead)}")
    x0_dir = None
    if "ode_init" in wrt or jacs:
        x0_dir = np.zeros(((lead.pop(),) if lead else ()) + (K, d, p))
    for name, shape in shapes:
        size = int(np.prod(shape))
        if name == "ode_init":
            x0_dir[..., k0:k0 + size, :, :] = np.eye(size).reshape(size, d, p)
        else:
            unit = np.zeros((K, size))
            unit[k0:k0 + size] = np.eye(size)
            tangents[name] = unit
            if name in jacs:                                        # direction j of this parameter moves ode_init by J[..., j]
                x0_dir[..., k0:k0 + size, :, :] += np.moveaxis(jacs[name], -1, -3)
        layout.append((name, k0, shape))
        k0 += size
    if x0_dir is not None:
        tangents["ode_init"] = x0_dir
    return tangents, layout


def _wrt_directions(who, sibling, ode_fun, ode_weight, ode_init, interrogate, kalman_type, obs_weight, wrt, init_jac, params):
    """What the two ``*_grid_grad`` do before their ``_jvp``: the refusals and the unit directions of ``wrt`` (tangents, layout)."""
    _grad_config(who, ode_fun, ode_weight, interrogate, kalman_type, obs_weight, (wrt,) if isinstance(wrt, str) else tuple(wrt), params,
                 sibling=sibling)
    tangents, layout = _unit_directions(who, ode_fun, ode_weight, ode_init, wrt, init_jac, params)
    if not tangents:
        raise ValueError(f"{who}: wrt is empty (K = 0)")
    return tangents, layout


def _grad_of(dvalue, layout, batched):
    """``dvalue`` (B, K) of the unit directions cut into the dict name -> gradient, (B, *shape) or, unbatched, shape."""
    grad = {}
    for name, k0, shape in layout:
        g = dvalue[:, k0:k0 + int(np.prod(shape))].reshape((-1,) + shape)
        grad[name] = g if batched else g[0]
    return grad
