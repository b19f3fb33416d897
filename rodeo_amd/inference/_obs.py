"""
What ``dalton`` and ``fenrir`` share on the host (private): the check of Gaussian observations, the configurations the device
kernels do not serve, and the front end of the two off-grid likelihoods ``dalton_at`` / ``fenrir_at`` -- where the observation
times sit on the grid, the sub-step priors they need, and the ``rk_dalton_at_in`` both entries read.
"""
import numpy as np
from .. import _lib
from ..solve import cached_plan, check_prior_at, eval_at_nodes, _device_ode, _interrogate_id, _prior_at_pair, _shape_rule


def _check_obs(obs_data, obs_weight, obs_var):
    """(obs (n_obs, d, n_bobs), D (n_obs, d, n_bobs, p), Omega (n_obs, d, n_bobs, n_bobs), n_bobs) as contiguous float64."""
    obs = np.ascontiguousarray(obs_data, dtype=np.float64)
    D = np.ascontiguousarray(obs_weight, dtype=np.float64)
    Om = np.ascontiguousarray(obs_var, dtype=np.float64)
    if D.ndim != 4:
        raise ValueError("fenrir: obs_weight must have shape (n_obs, n_block, n_bobs, n_bstate)")
    n_bobs = D.shape[2]
    if not 1 <= n_bobs <= 3:
        raise NotImplementedError("fenrir on the device: n_bobs (observations per block) in 1..3")
    if Om.shape != D.shape[:2] + (n_bobs, n_bobs) or obs.shape != D.shape[:2] + (n_bobs,):
        raise ValueError("fenrir: obs_data (n_obs, n_block, n_bobs), obs_weight (n_obs, n_block, n_bobs, n_bstate), obs_var "
                         "(n_obs, n_block, n_bobs, n_bobs)")
    return obs, D, Om, n_bobs


def _refuse_config(who, ode_weight, kalman_type, interrogate=None, bmeas=None, bstate=(2, 6), got=False):
    """
    The configurations the lane / tile kernels behind ``who`` do not serve: the square-root form, an ``ode_weight`` of the wrong
    rank, n_bstate outside ``bstate`` (``got``: the message names the value) and, where the caller has them, interrogate_chkrebtii
    (``interrogate`` given) and n_bmeas > 1 (``bmeas`` given: what its message says after "n_bmeas = 1 only").
    """
    if kalman_type == "square-root":
        raise NotImplementedError(f"{who}: the square-root form is not built on the device (kalman_type='standard' only)")
    if kalman_type != "standard":
        raise NotImplementedError                                   # dalton.py:83-88, 884-889; fenrir.py:293-298
    if interrogate is not None and _interrogate_id(interrogate)[0] == _lib.INTERROGATE_CHKREBTII:
        raise NotImplementedError(f"{who}: interrogate_chkrebtii is not supported (rodeo, schober, kramer)")
    W = np.shape(ode_weight)
    if len(W) not in (3, 4):
        raise ValueError("ode_weight must have shape (n_block, n_bmeas, n_bstate) [+ a leading batch axis]")
    if bmeas is not None and W[-2] != 1:
        raise NotImplementedError(f"{who} on the device: n_bmeas = 1 only{bmeas}")
    if not bstate[0] <= W[-1] <= bstate[1]:
        raise NotImplementedError(f"{who} on the device: n_bstate in {bstate[0]}..{bstate[1]}" + (f", got {W[-1]}" if got else ""))


def _served(who, ode_weight, kalman_type, obs_data, obs_weight, obs_var, **config):
    """``_refuse_config(who, ..., **config)``, then the observations against ``ode_weight``; returns (obs, D, Omega, n_bobs)."""
    _refuse_config(who, ode_weight, kalman_type, **config)
    W = np.shape(ode_weight)
    obs, D, Om, n_bobs = _check_obs(obs_data, obs_weight, obs_var)
    if D.shape[1:] != (W[-3], n_bobs, W[-1]):
        raise ValueError(f"obs_weight must have shape (n_obs, {W[-3]}, n_bobs, {W[-1]})")
    return obs, D, Om, n_bobs


# --- observations between grid nodes -------------------------------------------------------

def _compose(chain):
    """(Q, R) of the sub-steps `chain` applied in order: Q = Q_k .. Q_1, R = Q_k R' Q_k^T + R_k."""
    Qc, Rc = chain[0]
    for Qk, Rk in chain[1:]:
        Rc = np.matmul(np.matmul(Qk, Rc), np.swapaxes(Qk, -1, -2)) + Rk
        Qc = np.matmul(Qk, Qc)
    return Qc, Rc


def _at_layout(times, t_min, t_max, n_steps, prior_at, prior_pars, d, p, B, who="dalton_at"):
    """
    Where the observation times sit on the grid and the sub-step priors they need, checked on the host: returns
    ``(table (n_obs, 4) int32, pre, post)`` with table rows (node, off-grid flag, pre slot, post slot or -1) and ``pre`` /
    ``post`` lists of (Q, R) pairs (empty when every time is a node: ``prior_at`` is then never called).  Each interval's
    chain of sub-steps must compose to ``prior_pars`` (Chapman-Kolmogorov, ``check_prior_at``'s bar).  ``who`` names the caller
    in the messages.
    """
    t = np.asarray(times, dtype=np.float64)
    if t.ndim != 1 or t.size == 0:
        raise ValueError(f"{who}: obs_times must be a non-empty 1-D array, got shape {t.shape}")
    if not np.all(np.isfinite(t)):
        raise ValueError(f"{who}: obs_times holds a non-finite time")
    if np.any(np.diff(t) <= 0):
        raise ValueError(f"{who}: obs_times must be strictly increasing")
    if t[0] < t_min or t[-1] > t_max:
        raise ValueError(f"{who}: obs_times must lie in [t_min, t_max] = [{t_min}, {t_max}], got [{t[0]}, {t[-1]}]")
    node, on, _, _ = eval_at_nodes(t, t_min, t_max, n_steps)
    if np.any(np.diff(node[on]) == 0):
        raise ValueError(f"{who}: two observation times are the same grid node (within EVAL_AT_NODE_TOL of a step)")
    N = int(n_steps)
    table = np.zeros((len(t), 4), dtype=np.int32)
    table[:, 0], table[:, 1], table[:, 3] = node, ~on, -1
    pre, post = [], []
    for n in np.unique(node[~on]):
        members = np.nonzero(~on & (node == n))[0]
        left, right = t_min + (t_max - t_min) * n / N, t_min + (t_max - t_min) * (n + 1) / N
        events = np.concatenate([[left], t[members], [right]])
        gaps = np.diff(events)
        chain = [_prior_at_pair(prior_at, h, d, p, B) for h in gaps]
        check_prior_at(_compose(chain[:-1]), chain[-1], prior_pars, float(events[-2] - left), float(gaps[-1]))
        table[members, 2] = len(pre) + np.arange(len(members))
        table[members[-1], 3] = len(post)
        pre.extend(chain[:-1])
        post.append(chain[-1])
    return table, pre, post


def _stack_pairs(pairs, B, force=0):
    """[(Q, R)] each (d, p, p) or (B, d, p, p) -> ((Qs, Rs), batched): (n, d, p, p), or (n, d, p, p, B) batch-minor when any
    matrix is batched (``_stack_prior``'s rule: a batched sigma gives a batched R and a shared Q; both are then broadcast)."""
    batched = int(bool(force) or any(m.ndim == 4 for pair in pairs for m in pair))
    out = []
    for k in (0, 1):
        mats = [pair[k] for pair in pairs]
        if batched:
            full = np.array([np.broadcast_to(m, (B,) + m.shape[-3:]) for m in mats])              # (n, B, d, p, p)
            out.append(np.ascontiguousarray(np.moveaxis(full, 1, -1)))
        else:
            out.append(np.ascontiguousarray(np.array(mats)))
    return tuple(out), batched


def _obs_nodes(who, t, obs_times, n_obs):
    """The node of every observation time on the checked grid ``t`` (int32, strictly increasing), or the ValueError."""
    from ..grid import _times, nodes_of_times
    if np.shape(obs_times) != (n_obs,):
        raise ValueError(f"{who}: obs_times must have shape ({n_obs},), got {np.shape(obs_times)}")
    x = _times(obs_times, t, who)
    if np.any(np.diff(x) <= 0):
        raise ValueError(f"{who}: obs_times must be strictly increasing")
    node, on = nodes_of_times(t, x)
    if not np.all(on):
        raise ValueError(f"{who}: the observation time {float(x[~on][0])!r} is no node of t_grid (within EVAL_AT_NODE_TOL of the shorter "
                         "adjacent step); rodeo_amd.grid_with_times(t_grid, obs_times) returns a grid that has every time as a node")
    if np.any(np.diff(node) == 0):
        raise ValueError(f"{who}: two observation times are the same node of t_grid (within EVAL_AT_NODE_TOL of a step)")
    return node.astype(np.int32)


def _grid_plan(obs_slot, ode, ode_weight, ode_init, t, slot, pairs, interrogate, kalman_type, params, obs, D, Om, node, n_bobs):
    """
    What the likelihoods on a non-uniform grid (``dalton_grid``, ``fenrir_grid`` and their solvers) do once nothing is left to
    refuse: the cached batch-minor plan (its own prior pair is slot 0's) with the grid ``(t, slot, pairs)`` of ``grid._refusals``
    staged in ``rodeo_amd.solve_mv_grid``'s slot and the observations on the nodes ``node`` in ``obs_slot``.  Returns ``(plan, g,
    observation pointers and counts)``; the pointers are None for an empty observation set.
    """
    plan = cached_plan(ode, ode_weight, ode_init, t[0], t[-1], len(slot), interrogate, pairs[0], kalman_type, batch_minor=True,
                       **params)
    (q, r), batched = _stack_pairs(pairs, plan.B)
    d_t, d_slot, d_q, d_r = plan.staged("grid", t, slot, q, r)
    g = _lib.GridIn(t=d_t.ptr, slot=d_slot.ptr, q=d_q.ptr, r=d_r.ptr, q_batched=batched, r_batched=batched, n_slots=len(pairs))
    ptrs = (None,) * 4
    if len(node):
        ptrs = tuple(a.ptr for a in plan.staged(obs_slot, obs, D, Om, node))
    return plan, g, ptrs + (len(node), n_bobs)


def _at_inputs(who, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, prior_pars, n_obs, obs_times, prior_at, params):
    """
    What ``dalton_at`` and ``fenrir_at`` do between their refusals and their plan: the checks of ``prior_at`` and ``obs_times``,
    the solver's shape rule, ``_at_layout`` and the stacked sub-step priors.  Returns ``(table, stacked, batched)`` with
    ``stacked = (pre_trans, pre_noise, post_trans, post_noise)``, or ``None`` when every time is a node (the caller's on-grid
    entry then serves the nodes ``table[:, 0]``).
    """
    if not callable(prior_at):
        raise TypeError(f"{who}: prior_at must be a callable prior_at(dt) -> (wgt_state, var_state)")
    if np.shape(obs_times) != (n_obs,):
        raise ValueError(f"{who}: obs_times must have shape ({n_obs},), got {np.shape(obs_times)}")
    _, _, Q, R, _, _, sizes = _shape_rule(_device_ode(ode_fun, ode_weight, params), ode_weight, ode_init, prior_pars, params)
    B = sizes[0] if sizes else 1
    d, p = int(np.shape(ode_weight)[-3]), int(np.shape(ode_weight)[-1])
    table, pre, post = _at_layout(obs_times, t_min, t_max, n_steps, prior_at, (Q, R), d, p, B, who=who)
    if not pre:
        return table, None, 0
    (pre_q, pre_r), batched = _stack_pairs(pre, B)
    (post_q, post_r), _ = _stack_pairs(post, B, force=batched)
    return table, (pre_q, pre_r, post_q, post_r), batched


def _stage_at(plan, slot, obs, D, Om, table, stacked, batched):
    """The eight arrays of an off-grid likelihood on the device (``SolvePlan.staged``: uploaded again only when they change)
    and the ``rk_dalton_at_in`` that points at them; returns ``(d_obs, d_weight, d_var, at)``."""
    d_obs, d_w, d_v, d_tab, d_pq, d_pr, d_sq, d_sr = plan.staged(slot, obs, D, Om, table, *stacked)
    at = _lib.DaltonAtIn(table=d_tab.ptr, n_pre=stacked[0].shape[0], n_post=stacked[2].shape[0], pre_trans=d_pq.ptr,
                         pre_noise=d_pr.ptr, post_trans=d_sq.ptr, post_noise=d_sr.ptr, prior_batched=batched)
    return d_obs, d_w, d_v, at
