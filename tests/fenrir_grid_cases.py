"""
Test helper (not collected): the device cases of tests/test_gpu_fenrir_grid.py, in one place so that
tests/test_oracle_fenrir_grid.py can check on the CPU, beforehand, that every one of them is a case the device bars can judge:
(e) no y forecast variance lies in (1e-9, 1e-7) -- ten times either side of utils.py:60-78's 1e-8 rule -- and (f) the
restatement's own move under R (1 + 1e-15) is at most a tenth of the case's bar.

The problems, grids, observations (Omega = 0.05^2), nodes and prior scales are tests/grid_cases.py's and
tests/dalton_grid_cases.py's (imported, not edited).  Every ``solve_mv_grid`` case uses interrogate_rodeo and stops at
n_bstate = 5: with kramer or schober (an exact measurement) the backward predictions that Fenrir's smoothing sweep inverts are
singular on these problems -- the restated sweep raises LinAlgError or moves by 1e2 (mean) under R (1 + 1e-15) -- and at
n_bstate = 6 the restated mean moves by 1e-7 even on three steps.  kramer, schober, chkrebtii and n_bstate = 6 appear in value
cases only: the value needs no sweep.
"""
import functools
import numpy as np
import grid_cases as gc
import dalton_grid_cases as dgc
import fenrir_grid_oracle as fgo

VALUE_BAR = 1e-7                                         # of max(1, |ref|)        (tests/test_gpu_inference.py)
MEAN_BAR = 1e-8                                          # of max(1, max|ref|)
VAR_BAR = 1e-7                                           # of max|ref|             (test_fenrir_solve_mv_parity)
WIDE_NODES = (0, 1, 20, 21, 40)                          # node 0, node 1, two neighbours, node N


class FCase(dgc.DCase):
    """A dalton_grid_cases.DCase restated by fenrir_grid_oracle; the key (chkrebtii's) is the base case's."""

    def restate_value(self, r_scale=1.0, forecast_vars=None):
        return self._restate(fgo.fenrir_grid, self["key"], r_scale, forecast_vars=forecast_vars)

    def restate_mv(self, r_scale=1.0):
        return self._restate(fgo.solve_mv_grid, self["key"], r_scale)


@functools.lru_cache(maxsize=None)
def make(base, nodes=dgc.NODES, n_bobs=1, scale=None):
    """`base` (a grid_cases.Case) at dalton_grid_cases' prior scale (or `scale`) with its observations on `nodes`."""
    return FCase(dgc.make(base, nodes, n_bobs, scale))


@functools.lru_cache(maxsize=None)
def times_case(itg):
    """dalton_grid_cases.times_case's grid -- off-node observation times put into a uniform grid by ``grid_with_times``: 42 steps
    in four slots -- under interrogation `itg`.  The case carries the times it was made from under "times"."""
    import rodeo_amd as ra
    base = gc.fhn(3, itg, "uniform", B=3)
    t0 = base["t"]
    h = t0[1] - t0[0]
    times = np.array([t0[3] + 0.37 * h, t0[8], t0[20] + 0.5 * h])
    t, node = ra.grid_with_times(t0, times)
    moved = gc.Case(base)
    moved.update(t=t, label=base["label"] + " + grid_with_times")
    c = make(moved, tuple(int(k) for k in node))
    c["times"] = times
    return c


def _short(p, N, B):
    return gc.fhn(p, "rodeo", "distinct", N=N, t_max=0.1 * N, B=B)


def mv_cases():
    """Every fenrir.solve_mv_grid case; each is a value case too (65: a second wave with one live lane per block)."""
    out = [make(gc.fhn(3, "rodeo", kind)) for kind in gc.GRIDS]                                      # B absent
    out += [make(gc.fhn(2, "rodeo", "distinct")), make(gc.fhn(4, "rodeo", "distinct", B=3)), make(gc.fhn(5, "rodeo", "levels"))]
    out += [make(gc.fhn(3, "rodeo", "distinct", B=B)) for B in (1, 3, 65)]
    out += [make(gc.fhn(5, "rodeo", "levels", B=65))]
    out += [make(gc.fhn(3, "rodeo", "levels", B=3, batched_sigma=True)), make(gc.fhn(5, "rodeo", "levels", B=65, batched_sigma=True))]
    out += [make(_short(3, N, 65), dgc.SHORT_NODES[N]) for N in (1, 2, 3)]
    out += [make(_short(5, N, 3), dgc.SHORT_NODES[N], scale=dgc.SHORT_SCALE_5) for N in (1, 2, 3)]
    out += [make(gc.fhn(3, "rodeo", "distinct", B=3), WIDE_NODES), make(gc.fhn(3, "rodeo", "distinct", B=3), ())]
    out += [make(gc.fhn(3, "rodeo", "distinct", B=3), n_bobs=m) for m in (2, 3)]
    out += [make(gc.fhn(5, "rodeo", "levels", B=3), WIDE_NODES, n_bobs=3), make(gc.fhn(2, "rodeo", "levels", B=3), n_bobs=2)]
    out += [make(gc.lorenz(p, "rodeo", "distinct", B=5)) for p in (3, 4)]                             # three blocks: the ordered sum
    out += [times_case("rodeo")]
    return out


def value_only_cases():
    """The fenrir_grid cases whose smoothing sweep is not tested: n_bstate = 6, and the three other interrogations."""
    out = [make(gc.fhn(6, "rodeo", kind, t_max=gc.T_MAX[6], B=3), n_bobs=m) for kind, m in (("levels", 1), ("distinct", 3))]
    out += [make(gc.fhn(3, "kramer", "distinct", B=3)), make(gc.fhn(4, "kramer", "levels")), make(gc.fhn(3, "schober", "levels", t_max=2.0))]
    out += [make(gc.fhn(3, "chkrebtii", "levels", key=11)), make(gc.lorenz(3, "kramer", "distinct", B=5)), times_case("kramer")]
    return out


def value_cases():
    return mv_cases() + value_only_cases()


@functools.lru_cache(maxsize=None)
def value_ref(c):
    """The restated value of a case, computed once and shared (read-only)."""
    v = np.asarray(c.restate_value())
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def mv_ref(c):
    """The restated moments of a case, computed once and shared (read-only)."""
    m, v = c.restate_mv()
    m.setflags(write=False)
    v.setflags(write=False)
    return m, v
