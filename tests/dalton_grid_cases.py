"""
Test helper (not collected): the device cases of tests/test_gpu_dalton_grid.py, in one place so that
tests/test_oracle_dalton_grid.py can check on the CPU, beforehand, that every one of them is a case the device bars can judge:
(e) no forecast variance of z or of y, in either filter, lies in (1e-9, 1e-7) -- ten times either side of utils.py:60-78's 1e-8
rule, where two correct evaluations could keep and drop the same term -- and (f) the restatement's own move under R (1 + 1e-15)
stays below the bar.

The problems and grids are tests/grid_cases.py's (imported, not edited).  Prior scale per n_bstate, chosen for (e): grid_cases'
SIGMA up to 3; 100 x SIGMA at 4 and 5 (s scales with sigma^2: with SIGMA the z forecast variances of p = 4 kramer "distinct" are
3.4e-10 .. 1.5e-4 and p = 5 rodeo "levels" reaches down to 2.8e-9); SIGMA / 10 at 6 on [0, 1], where every z term is then dropped
in both filters (s <= 5.1e-11) and the value is the y terms alone.  Observation noise Omega = 0.05^2 on the diagonal.
"""
import functools
import numpy as np
import grid_cases as gc
import dalton_grid_oracle as dgo
from oracle import priors

OMEGA = 0.05 ** 2
NODES = (1, 7, 8, 19, 33, 40)                           # of the N = 40 grids: node 1, two neighbours, node N
SCALE = {2: 1.0, 3: 1.0, 4: 100.0, 5: 100.0, 6: 0.1}     # of grid_cases.SIGMA (Lorenz63: of its own sigma)


def observations(d, p, n_obs, n_bobs=1, seed=0):
    """y (n_obs, d, n_bobs), D (n_obs, d, n_bobs, p) = rows e_0 .. e_{n_bobs-1}, Omega (n_obs, d, n_bobs, n_bobs) diagonal."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((n_obs, d, n_bobs)) * 0.3 - 0.5
    D = np.zeros((n_obs, d, n_bobs, p))
    for j in range(n_bobs):
        D[:, :, j, j] = 1.0
    Om = np.zeros((n_obs, d, n_bobs, n_bobs))
    for j in range(n_bobs):
        Om[:, :, j, j] = OMEGA * (1.0 + 0.5 * j)
    return y, D, Om


class DCase(gc.Case):
    """A grid_cases.Case with observations on nodes: keys nodes, y, D, Om, n_bobs besides Case's."""

    def device_call(self, fn, key=None, ode=None):
        return fn(key, *self.device_args(ode), self["y"], self["t"][list(self["nodes"])], self["D"], self["Om"], **self["params"])

    def _restate(self, fn, key, r_scale=1.0, **kw):
        return fn(key, self["oracle_ode"], self["W"], self["x0"], self["t"], gc.ITG[self["itg"]][1],
                  self.prior_at(priors.ibm_init, r_scale), self["y"], self["nodes"], self["D"], self["Om"], **kw, **self["params"])

    def restate_value(self, r_scale=1.0, forecast_vars=None):
        return self._restate(dgo.dalton_grid, None, r_scale, forecast_vars=forecast_vars)

    def restate_mv(self, r_scale=1.0):
        return self._restate(dgo.solve_mv_grid, None, r_scale)

    def restate_sim(self, key, r_scale=1.0):
        return self._restate(dgo.solve_sim_grid, key, r_scale)


@functools.lru_cache(maxsize=None)
def make(base, nodes=NODES, n_bobs=1, scale=None):
    """`base` (a grid_cases.Case) at this file's prior scale (or `scale`) with observations on `nodes`."""
    d, p = base["W"].shape[-3], base["p"]
    scale = SCALE[p] if scale is None else scale
    y, D, Om = observations(d, p, len(nodes), n_bobs)
    c = DCase(base)
    c.update(sigma=base["sigma"] * scale, nodes=tuple(nodes), y=y, D=D, Om=Om, n_bobs=n_bobs,
             label=f"{base['label']} sigma x{scale:g} obs@{','.join(map(str, nodes)) or 'none'} n_bobs={n_bobs}")
    return c


def _short(p, itg, N, B=None):
    return gc.fhn(p, itg, "distinct", N=N, t_max=0.1 * N, B=B)


SHORT_NODES = {1: (0, 1), 2: (1, 2), 3: (0, 2, 3)}       # N = 1, 2, 3: node 0, node 1, node N, two neighbours
SHORT_SCALE_5 = 1000.0                                   # steps of 0.035 .. 0.28: with 100 x SIGMA p = 5 reaches down to 2.3e-9


@functools.lru_cache(maxsize=None)
def times_case():
    """Off-node observation times put into a uniform grid by ``rodeo_amd.grid_with_times``: 42 steps in four slots (h, 0.37 h,
    0.63 h, twice 0.5 h).  The case carries the times it was made from under "times"."""
    import rodeo_amd as ra
    base = gc.fhn(3, "kramer", "uniform", B=3)
    t0 = base["t"]
    h = t0[1] - t0[0]
    times = np.array([t0[3] + 0.37 * h, t0[8], t0[20] + 0.5 * h])
    t, node = ra.grid_with_times(t0, times)
    moved = gc.Case(base)
    moved.update(t=t, label=base["label"] + " + grid_with_times")
    c = make(moved, tuple(int(k) for k in node))
    c["times"] = times
    return c


def value_cases():
    """Every dalton_grid case of tests/test_gpu_dalton_grid.py (the log-likelihood form: 32 trajectories per wave)."""
    out = [make(gc.fhn(3, "kramer", kind)) for kind in ("levels", "distinct")]                       # B absent, two register sets
    out += [make(gc.fhn(3, "kramer", "distinct", B=B)) for B in (1, 3, 33)]                           # 33: a second wave, one live pair
    out += [make(gc.fhn(4, "kramer", "distinct", B=3)), make(gc.fhn(4, "rodeo", "levels"))]
    out += [make(gc.fhn(5, "rodeo", "levels", B=B)) for B in (None, 3, 33)]                           # the LDS-staged shared pair
    out += [make(gc.fhn(5, "rodeo", "levels", B=33, batched_sigma=True))]                             # per-lane LDS rows
    out += [make(gc.fhn(3, "kramer", "levels", B=3, batched_sigma=True))]                             # batched pairs in registers
    out += [make(_short(3, "kramer", N), SHORT_NODES[N]) for N in (1, 2, 3)]
    out += [make(_short(5, "rodeo", N, B=3), SHORT_NODES[N], scale=SHORT_SCALE_5) for N in (1, 2, 3)]
    out += [make(gc.fhn(3, "kramer", "distinct"), (0, 1, 20, 21, 40)), make(gc.fhn(3, "kramer", "distinct"), ())]
    out += [make(gc.fhn(5, "rodeo", "levels", B=3), (0, 1, 20, 21, 40))]
    out += [make(gc.fhn(3, "kramer", "distinct", B=3), n_bobs=m) for m in (2, 3)]
    out += [make(gc.fhn(2, "rodeo", "levels", B=3)), make(gc.fhn(6, "rodeo", "distinct", t_max=1.0, B=3), n_bobs=3)]
    out += [make(gc.fhn(3, "rodeo", "distinct")), make(gc.fhn(3, "schober", "levels", t_max=2.0))]
    out += [make(gc.lorenz(3, "rodeo", "distinct", B=5)), make(gc.lorenz(4, "rodeo", "distinct", B=5)), times_case()]
    return out


def mv_cases():
    """Every dalton.solve_mv_grid case (the store form: one lane per trajectory; 65 is a second wave with one live lane)."""
    out = [make(gc.fhn(3, "kramer", "distinct", B=B)) for B in (None, 1, 65)]
    out += [make(gc.fhn(4, "kramer", "distinct", B=3)), make(gc.fhn(5, "rodeo", "levels", B=65))]
    out += [make(gc.fhn(5, "rodeo", "levels", B=65, batched_sigma=True))]
    out += [make(_short(3, "kramer", N, B=65), SHORT_NODES[N]) for N in (1, 2, 3)]
    out += [make(_short(5, "rodeo", N, B=3), SHORT_NODES[N], scale=SHORT_SCALE_5) for N in (1, 2, 3)]
    out += [make(gc.fhn(3, "kramer", "distinct", B=3), (0, 1, 20, 21, 40)), make(gc.fhn(3, "kramer", "distinct", B=3), n_bobs=2)]
    # (5, 3) where the value cases have (6, 3): at n_bstate = 6 the restated MEAN moves by more than its absolute bar under
    # R (1 + 1e-15) -- 2.6e-8 even on three steps, its highest derivatives being of order 1e5 (grid_cases.Case.yardstick)
    out += [make(gc.fhn(2, "rodeo", "levels", B=3)), make(gc.fhn(5, "rodeo", "levels", B=3), n_bobs=3)]
    out += [make(gc.fhn(3, "schober", "levels", t_max=2.0)), make(gc.lorenz(3, "rodeo", "distinct", B=5)),
            make(gc.lorenz(4, "rodeo", "distinct", B=5))]
    return out


def sim_cases():
    """Every dalton.solve_sim_grid case: (case, key).  n_bstate = 5 (the LDS-staged pair) on three steps: on the N = 40 grids the
    restated PATH moves by 2e-4 .. 0.13 of max|x| under R (1 + 1e-15), on three steps by 1.3e-12."""
    return [(make(gc.fhn(3, "rodeo", "distinct", B=65)), 42), (make(_short(5, "rodeo", 3, B=3), SHORT_NODES[3], scale=SHORT_SCALE_5), 7),
            (make(_short(3, "kramer", 2, B=3), SHORT_NODES[2]), 5)]


def all_cases():
    seen, out = set(), []
    for c in value_cases() + mv_cases() + [c for c, _ in sim_cases()]:
        if id(c) not in seen:
            seen.add(id(c))
            out.append(c)
    return out


def mv_moves(c):
    """grid_cases.mv_moves for a DCase: the restatement and its own move under a 1e-15 relative perturbation of R."""
    return gc.mv_moves(c)
