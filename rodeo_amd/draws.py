"""
``solve_sim_draws`` (an addition): many sample paths per trajectory from ONE forward filter, stored
and downloaded only at the nodes the caller keeps.

    solve_sim_draws(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                    kalman_type="standard", n_draws=1, keep=None, **params)
        -> x  (n_draws, K, d, p)            one trajectory
              (B, n_draws, K, d, p)         batched inputs (solve_sim's batching rules)

THE LAW, which is also the contract: draw ``s`` is the path ``solve_sim`` returns for the integer seed
``(_seed(key) + s) mod 2**64`` -- the kernel keys Philox with (seed + s, trajectory, step, block, smoothing purpose) exactly as
``solve_sim``'s backward kernel does with seed -- so ``x[..., s, :, :, :]`` equals ``solve_sim(key + s, ...)[keep]`` up to
rounding, and node 0 is ``ode_init``.

Under interrogate_rodeo / _schober / _kramer the forward filter does not depend on the key, so it runs once
(``rk_solve_filter``'s lanes on batch-minor records).  The backward kernel (``bwd_sim_draws_kernel``, one lane per (chunk of
draws, block, trajectory)) does per step once what no draw changes -- the load of the filtered record, the prediction, the
smoothing gain, Sigma_f - G T^T and its factor -- and per draw a matrix-vector product, p normals and, at a kept node, a
store.  A chunk is 1, 2 or ``chunk()`` = 4 draws, the smallest whose waves fit the device side by side (the chain of n_steps
dependent steps bounds the time from below, so sharing pays only once the device is full); the draws do not depend on it.
All of it runs on the device (``rk_solve_sim_draws``).

Not built: the square-root form, interrogate_chkrebtii, the p = 3 tile route, the dense route (n_bmeas > 1), draws of
``dalton.solve_sim`` on the uniform grid (``rodeo_amd.inference.dalton.solve_sim_draws_grid`` gives draws from p(X | Z, Y) on any
grid, a uniform one included) and off-grid times (``solve_sim_draws_grid``, grid_draws.py, takes a grid that has them as nodes).
"""
import numpy as np
from . import _lib
from .solve import _KALMAN, _device_ode, _interrogate_id, _seed, _shape_rule, cached_plan

BSTATE = (2, 6)                                                     # n_bstate served
N_DRAWS_MAX = 65535                                                 # (the library's bound: one grid row per chunk of draws)


def chunk():
    """The most draws one lane of the backward kernel carries (the library's ``rk_sim_draws_chunk``)."""
    return int(_lib.load().rk_sim_draws_chunk())


def draw_seed(key, s):
    """The integer seed whose ``solve_sim`` path is draw ``s`` of ``solve_sim_draws(key, ...)``: (seed(key) + s) mod 2**64."""
    return (_seed(key) + int(s)) & 0xFFFFFFFFFFFFFFFF


def _keep_rule(keep, n_steps, name="solve_sim_draws"):
    """``keep`` as an int32 array of grid indices, or None for every node; ValueError for what the contract rules out (``name``:
    the function the message names)."""
    if keep is None:
        return None
    k = np.asarray(keep)
    if k.ndim != 1 or not np.issubdtype(k.dtype, np.integer):
        raise ValueError(f"{name}: keep must be a 1-D integer array of grid indices, got shape {k.shape}, dtype {k.dtype}")
    if k.size == 0:
        raise ValueError(f"{name}: keep is empty")
    if k.min() < 0 or k.max() > n_steps:
        raise ValueError(f"{name}: keep must lie in 0 .. n_steps = {n_steps}, got {int(k.min())} .. {int(k.max())}")
    if np.any(np.diff(k.astype(np.int64)) <= 0):
        raise ValueError(f"{name}: keep must be strictly increasing")
    return k.astype(np.int32)


def _draw_rules(name, interrogate, n_draws, keep, n_steps):
    """What is refused for the draws themselves, for ``solve_sim_draws`` and for ``solve_sim_draws_grid`` (grid_draws.py):
    interrogate_chkrebtii, ``n_draws`` and ``keep``; returns (n_draws, keep or None)."""
    if _interrogate_id(interrogate)[0] == _lib.INTERROGATE_CHKREBTII:
        raise NotImplementedError(f"{name}: interrogate_chkrebtii is not served: its forward pass depends on the key, "
                                  "so the draws cannot share one filter (rodeo, schober, kramer)")
    if isinstance(n_draws, bool) or not isinstance(n_draws, (int, np.integer)) or not 1 <= n_draws <= N_DRAWS_MAX:
        raise ValueError(f"{name}: n_draws must be an integer in 1 .. {N_DRAWS_MAX}, got {n_draws!r}")
    return int(n_draws), _keep_rule(keep, int(n_steps), name)


def _refusals(ode_fun, ode_weight, ode_init, n_steps, interrogate, prior_pars, kalman_type, n_draws, keep, params):
    """Everything this build does not serve, raised before any device work; returns (DeviceODE, n_draws, keep or None)."""
    if kalman_type not in _KALMAN:
        raise NotImplementedError(f"solve_sim_draws: unknown kalman_type {kalman_type!r}")
    if kalman_type != "standard":
        raise NotImplementedError("solve_sim_draws: kalman_type='square-root' is not built")
    n_draws, keep = _draw_rules("solve_sim_draws", interrogate, n_draws, keep, n_steps)
    W = np.shape(ode_weight)
    if len(W) not in (3, 4):
        raise ValueError("ode_weight must have shape (n_block, n_bmeas, n_bstate) [+ a leading batch axis]")
    d, m, p = W[-3:]
    if m != 1:
        raise NotImplementedError("solve_sim_draws on the device: n_bmeas = 1 only (the dense / indep_init form is not served)")
    if not BSTATE[0] <= p <= BSTATE[1]:
        raise NotImplementedError(f"solve_sim_draws on the device: n_bstate in {BSTATE[0]}..{BSTATE[1]}, got {p}")
    ode = _device_ode(ode_fun, ode_weight, params)
    if (ode.n_block, ode.n_bmeas) != (d, m):
        raise ValueError(f"ODE '{ode.name}' has (n_block, n_bmeas) = ({ode.n_block}, {ode.n_bmeas}) but ode_weight has ({d}, {m})")
    _shape_rule(ode, ode_weight, ode_init, prior_pars, params)      # ValueError: ranks, mismatched shapes, batch sizes
    return ode, n_draws, keep


def _launch_draws(name, plan, key, fn, n_draws, keep, *front):
    """One launch of a many-draws entry ``fn(handle, cfg, in, out, *front, n_draws, keep, K, x_draws)`` on the batch-minor
    ``plan`` and the download: ``x`` (n_draws, K, d, p) or (B, n_draws, K, d, p).  ``solve_sim_draws``'s, and with the grid (and
    the observations) in ``front`` that of the two ``solve_sim_draws_grid`` (grid_draws.py, inference/dalton.py)."""
    dev = plan.dev
    K = plan.N + 1 if keep is None else int(keep.size)
    keep_dev = plan.staged("sim_draws_keep", keep)[0] if keep is not None else None
    x = dev.empty((n_draws, K, plan.d, plan.p, plan.B))
    plan.launch(fn, key, _lib.MODE_FILTER, *front, n_draws, keep_dev.ptr if keep_dev is not None else None, K, x.ptr)
    if plan.layout != _lib.LAYOUT_BATCH_MINOR:                       # (batch_minor=True: the records the backward kernel reads)
        raise RuntimeError(f"{name}: the plan reports layout {plan.layout}, not the batch-minor records")
    xs = x.batch_first()                                             # (B, n_draws, K, d, p): a view of the download
    return xs if plan.batched else xs[0]


def solve_sim_draws(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                    kalman_type="standard", n_draws=1, keep=None, **params):
    """
    ``n_draws`` sample solutions per trajectory from one forward filter: ``x`` (n_draws, K, d, p), or (B, n_draws, K, d, p) for
    batched inputs.  The first nine arguments and the batching rules are ``solve_sim``'s (a leading batch axis on ``ode_init``,
    ``prior_pars``, ``**params``).

    ``keep``: ``None`` keeps every node (K = n_steps + 1); otherwise a 1-D integer array of grid indices in 0 .. n_steps,
    strictly increasing, K = len(keep) -- only those nodes are stored and downloaded.  ``n_draws`` and ``keep`` are keywords of
    this function, so an ODE parameter named ``n_draws`` or ``keep`` is not possible.

    The law: draw ``s`` is ``solve_sim``'s path for the integer seed ``(seed(key) + s) mod 2**64`` (None -> 0, an int as it is,
    a 2-word uint32 key packed) -- ``x[..., s, :, :, :]`` equals ``solve_sim(key + s, ...)[keep]`` up to rounding; node 0 is
    ``ode_init``.

    Refused before any device work: NotImplementedError for an unknown ``kalman_type``, for ``"square-root"`` (not built), for
    ``interrogate_chkrebtii`` (its forward pass depends on the key, so the draws cannot share one filter), n_bmeas > 1 and
    n_bstate outside 2 .. 6; ValueError for an ``n_draws`` that is not an integer in 1 .. 65535, a ``keep`` that is not 1-D
    integer, is empty, leaves 0 .. n_steps or is not strictly increasing, and for the shapes ``solve_sim`` refuses.
    """
    ode, n_draws, keep = _refusals(ode_fun, ode_weight, ode_init, n_steps, interrogate, prior_pars, kalman_type, n_draws, keep,
                                   params)
    plan = cached_plan(ode, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type,
                       batch_minor=True, **params)
    return _launch_draws("solve_sim_draws", plan, key, plan.dev.lib.rk_solve_sim_draws, n_draws, keep)
