"""
``solve_sim_draws_grid`` (an addition): ``solve_sim_draws`` on the grid it is given -- many sample paths
per trajectory from ONE forward filter on a non-uniform ``t_grid``, stored and downloaded only at the nodes the caller keeps.
Uncertainty bands at the observation times: put the times in with ``grid_with_times`` and keep their nodes.

    solve_sim_draws_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at,
                         kalman_type="standard", n_draws=1, keep=None, **params)
        -> x  (n_draws, K, d, p)            one trajectory
              (B, n_draws, K, d, p)         batched inputs (solve_sim_grid's batching rules)

THE LAW, which is also the contract: draw ``s`` is the path ``solve_sim_grid`` returns for the integer seed
``draws.draw_seed(key, s)`` = (seed(key) + s) mod 2**64, restricted to ``keep`` -- the kernel keys Philox with (seed + s,
trajectory, step, block, smoothing purpose) exactly as ``solve_sim_grid``'s backward kernel does with seed; node 0 is
``ode_init``.

The forward pass is ``solve_sim_grid``'s (``grid_fwd_kernel``), run once.  The backward kernel (``grid_bwd_sim_draws_kernel``, one
lane per (chunk of draws, block, trajectory)) is ``solve_sim_draws``'s with every step's own prior pair in the prediction and in
the smoothing gain; the chunk rule is ``solve_sim_draws``'s (``draws.chunk()``), and the draws do not depend on it.  All of it
runs on the device (``rk_solve_sim_draws_grid``).  ``rodeo_amd.inference.dalton.solve_sim_draws_grid`` is the same from DALTON's
joint filter: draws from p(X | Z, Y).

Not built: the square-root form, interrogate_chkrebtii, the p = 3 tile route, draws from Fenrir's solver, and grids inside
``solve_mv_at`` and ``daltonng``.
"""
import ctypes as C
from . import grid
from .draws import _draw_rules, _launch_draws
from .inference._obs import _grid_plan


def solve_sim_draws_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, kalman_type="standard", n_draws=1,
                         keep=None, **params):
    """
    ``n_draws`` sample solutions per trajectory on the nodes ``t_grid`` from one forward filter: ``x`` (n_draws, K, d, p), or
    (B, n_draws, K, d, p) for batched inputs.  The first seven arguments, ``kalman_type``, the grid rules, the slot rule
    (``grid_slots``: ``prior_at`` is called once per slot) and the batching rules are ``solve_sim_grid``'s.

    ``keep``: ``None`` keeps every node (K = N + 1); otherwise a 1-D integer array of node indices of ``t_grid`` in 0 .. N,
    strictly increasing, K = len(keep) -- only those nodes are stored and downloaded (``grid_with_times`` returns the nodes of
    the times it puts in).  ``n_draws`` (1 .. 65535) and ``keep`` are keywords of this function, so an ODE parameter named
    ``n_draws`` or ``keep`` is not possible.

    The law: draw ``s`` is ``solve_sim_grid``'s path for the integer seed ``draws.draw_seed(key, s)`` --
    ``x[..., s, :, :, :]`` equals ``solve_sim_grid(key + s, ...)[keep]``; node 0 is ``ode_init``.

    Refused before any device work: everything ``solve_sim_grid`` refuses, and what ``solve_sim_draws`` refuses for ``n_draws``,
    ``keep`` and ``interrogate_chkrebtii`` (its forward pass depends on the key, so the draws cannot share one filter).
    """
    name = "solve_sim_draws_grid"
    n_draws, keep = _draw_rules(name, interrogate, n_draws, keep, len(grid._grid(t_grid)) - 1)
    ode, t, slot, pairs = grid._refusals(name, ode_fun, ode_weight, ode_init, t_grid, prior_at, kalman_type, params)
    plan, g, _ = _grid_plan("dalton_grid", ode, ode_weight, ode_init, t, slot, pairs, interrogate, kalman_type, params, None, None,
                            None, (), 0)                            # (the grid staged on the plan; no observations)
    return _launch_draws(name, plan, key, plan.dev.lib.rk_solve_sim_draws_grid, n_draws, keep, C.byref(g))
