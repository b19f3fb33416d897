"""
``solve_sim_draws_grid`` restated with the NumPy oracle (a helper, not collected): its law taken literally -- draw ``s`` is
tests/grid_oracle.py's ``solve_sim_grid`` (for DALTON tests/dalton_grid_oracle.py's) under the integer seed (seed + s) mod 2**64,
restricted to the kept nodes -- and the problems of the statistical pins (tests/test_oracle_draws_grid.py on the oracle,
tests/test_gpu_draws_grid.py on the device).
"""
import numpy as np
import grid_cases as gc
import dalton_grid_cases as dgc
import grid_oracle as go
import dalton_grid_oracle as dgo
import draws_oracle as dro

MASK = dro.MASK


def _loop(one, key, n_draws, keep):
    seed = 0 if key is None else int(key)
    rows = slice(None) if keep is None else np.asarray(keep, dtype=np.int64)
    return np.stack([one((seed + s) & MASK)[..., rows, :, :] for s in range(n_draws)], axis=-4)


def solve_sim_draws_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, n_draws=1, keep=None, **params):
    """(n_draws, K, d, p), or (B, n_draws, K, d, p) for batched inputs; ``key`` an integer seed (None: 0)."""
    return _loop(lambda seed: go.solve_sim_grid(seed, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, **params),
                 key, n_draws, keep)


def dalton_solve_sim_draws_grid(key, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data, obs_nodes,
                                obs_weight, obs_var, n_draws=1, keep=None, **params):
    """The same over ``dalton_grid_oracle.solve_sim_grid`` (observations on the nodes ``obs_nodes``): draws from p(X | Z, Y)."""
    return _loop(lambda seed: dgo.solve_sim_grid(seed, ode_fun, ode_weight, ode_init, t_grid, interrogate, prior_at, obs_data,
                                                 obs_nodes, obs_weight, obs_var, **params), key, n_draws, keep)


def restate(c, key, n_draws, keep=None, r_scale=1.0):
    """The law for a grid_cases.Case or a dalton_grid_cases.DCase: its own ``restate_sim`` under every seed."""
    return _loop(lambda seed: c.restate_sim(seed, r_scale), key, n_draws, keep)


# ---- the statistical pins: tests/draws_oracle.py's on a grid ------------------------------------------------------------------
# FitzHugh-Nagumo, n_bstate 3, kramer, the 8 distinct steps of grid_cases.grid("distinct", 8, 0.2), key 7, 2048 draws, bounds
# draws_oracle.pin_bounds().  (a) against grid_oracle.solve_mv_grid's posterior.  (b) the same problem with observations on the
# nodes PIN_NODES at 100 x the prior scale, against dalton_grid_oracle.solve_mv_grid's: at dalton_grid_cases' own scale the data
# move the mean by 1.6 standard errors only and the pin could not tell a sampler that ignores them, so (b) also sets its draws
# against p(X | Z) at that scale and asserts that THIS side fails.
PIN_NODES, PIN_SCALE = (0, 1, 4, 5, 8), 100.0


def pin_case():
    return gc.fhn(dro.PIN_P, "kramer", "distinct", N=dro.PIN_N, t_max=dro.PIN_T_MAX)


def pin_dalton_case():
    return dgc.make(pin_case(), PIN_NODES, scale=PIN_SCALE)


def pin_data_free(c):
    """`c` (a DCase) without its data: the plain problem at the same prior scale."""
    return gc.Case(c)


def pin_posterior(c):
    """The restated posterior mean (N+1, d, p) and marginal variances (N+1, d, p) of a pin case."""
    m, v = c.restate_mv()
    return m, np.einsum("...ii->...i", v)
