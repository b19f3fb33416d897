"""
Test helper (not collected): the device cases of tests/test_gpu_daltonng_grid.py, in one place so that
tests/test_oracle_daltonng_grid.py can check on the CPU, beforehand, that every one of them is a case the device bars can judge:
the restatement is finite, its own move under R (1 + 1e-15) stays below the bar, and no eigenvalue of a conditional variance lies
within 1e-6 relative of utils.py:60-78's 1e-8 rule.

The problems and grids are tests/grid_cases.py's (imported, not edited) at their own prior scale; the model is
``daltonng_oracle.poisson()`` on counts with mean 2 (``default_rng(0)``), observed on nodes 1, 7, 8, 19, 33, 40 of the N = 40 grids.
"""
import functools
import numpy as np
import grid_cases as gc
import daltonng_oracle as ng
import daltonng_grid_oracle as ngo
from oracle import priors
from rodeo_amd.trace import gammaln

NODES = (1, 7, 8, 19, 33, 40)                           # of the N = 40 grids: node 1, two neighbours, node N
SHORT_NODES = {1: (0, 1), 2: (1, 2), 3: (0, 2, 3)}       # N = 1, 2, 3: node 0, node 1, node N, two neighbours
VALUE_BAR, MOMENT_BAR = 1e-7, 1e-8                       # tests/test_gpu_daltonng.py's


def poisson_loglik(obs_data_i, ode_data_i, ind, **params):
    """The device side of ``daltonng_oracle.poisson()`` (tests/test_gpu_daltonng.py's)."""
    eta = 0.1 + 0.5 * ode_data_i[:, 0]
    y = obs_data_i.flatten()
    return np.sum(y * eta - np.exp(eta) - gammaln(y + 1.0))


def coupled_loglik(y, X, ind, theta):
    """The device side of ``daltonng_oracle.coupled()`` (tests/test_gpu_daltonng.py's): two active components in block 0, a
    parameter of **params inside."""
    r0 = y[0, 0] - X[0, 0] * X[1, 0]
    r1 = y[1, 0] - theta[0] * X[0, 1]
    return -0.5 * r0 * r0 / 0.04 - 0.5 * r1 * r1 / 0.25 - 0.5 * (X[0, 0] - 0.3 * X[0, 1]) ** 2 - 0.5 * X[1, 0] ** 2


MODELS = {"poisson": (poisson_loglik, ng.poisson, None), "coupled": (coupled_loglik, ng.coupled, ((0, 1), (0,)))}


class NCase(gc.Case):
    """A grid_cases.Case with counts on nodes: keys nodes, y, model besides Case's."""

    def device_call(self, fn, ode=None):
        return fn(None, *self.device_args(ode), self["y"], self["t"][list(self["nodes"])], MODELS[self["model"]][0], **self["params"])

    def _one(self, fn, b, r_scale, **kw):
        """The restatement for trajectory b (None: the case has no batch axis)."""
        pick = (lambda a: a) if b is None else (lambda a: a[b])
        sigma = self["sigma"] if self["sigma"].ndim == 1 else self["sigma"][b]
        p, d = self["p"], self["W"].shape[-3]

        def prior_at(h):
            Q, R = priors.ibm_init(h, p, sigma)
            return Q, R * r_scale
        _, make, active = MODELS[self["model"]]
        return fn(self["oracle_ode"], self["W"], pick(self["x0"]), self["t"], gc.ITG[self["itg"]][1], prior_at, self["y"],
                  self["nodes"], *make(), active=active or ((0,),) * d, **kw, **{k: pick(v) for k, v in self["params"].items()})

    def picked(self):
        """The trajectories the device tests compare (None: no batch axis): all of a small batch; of 33 and 65 the ends of the
        first wave's halves and the last trajectory, which sits alone in the second wave."""
        B = self["B"]
        return None if B is None else (list(range(B)) if B <= 5 else sorted({0, 1, 30, 31, 32, B - 2, B - 1}))

    def _all(self, fn, r_scale, **kw):
        if self["B"] is None:
            return fn(None, r_scale, **kw)
        return [fn(b, r_scale, **kw) for b in self.picked()]

    def restate_value(self, r_scale=1.0, cond_eigs=None):
        """A float, or the values of the trajectories ``picked()``."""
        out = self._all(lambda b, r, **kw: self._one(ngo.daltonng_grid, b, r, **kw), r_scale, cond_eigs=cond_eigs)
        return out if self["B"] is None else np.array(out)

    def restate_mv(self, r_scale=1.0):
        """(mean, var), with a leading axis over the trajectories ``picked()`` for a batched case."""
        out = self._all(lambda b, r: self._one(ngo.solve_mv_nn_grid, b, r), r_scale)
        return out if self["B"] is None else (np.stack([m for m, _ in out]), np.stack([v for _, v in out]))


@functools.lru_cache(maxsize=None)
def make(base, nodes=NODES, model="poisson", seed=0):
    d = base["W"].shape[-3]
    if model == "poisson":
        y = np.random.default_rng(seed).poisson(2.0, size=(len(nodes), d, 1)).astype(np.float64)
    else:
        y = np.random.default_rng(4).standard_normal((len(nodes), d, 1)) * 0.3
    c = NCase(base)
    c.update(nodes=tuple(nodes), y=y, model=model, label=f"{base['label']} {model} obs@{','.join(map(str, nodes)) or 'none'}")
    return c


def _short(p, itg, N, B=None, batched_sigma=False):
    return gc.fhn(p, itg, "distinct", N=N, t_max=0.1 * N, B=B, batched_sigma=batched_sigma)


def single_cases():
    """The ten single-trajectory cases at the plain bars (both calls)."""
    out = [make(gc.fhn(3, "kramer", kind)) for kind in ("levels", "distinct")]
    out += [make(gc.fhn(3, "rodeo", "distinct")), make(gc.fhn(3, "schober", "distinct", t_max=2.0))]
    out += [make(gc.fhn(4, "kramer", kind)) for kind in ("levels", "distinct")] + [make(gc.fhn(4, "rodeo", "distinct"))]
    out += [make(gc.fhn(5, "rodeo", kind)) for kind in ("levels", "distinct")] + [make(gc.fhn(2, "rodeo", "levels"))]
    return out


def yardstick_case():
    """n_bstate = 6: mean and variance on the perturbation yardstick (grid_cases.Case.yardstick), the value at the plain bar."""
    return make(gc.fhn(6, "rodeo", "distinct", t_max=1.0))


def value_cases():
    """The batched daltonng_grid cases (BOTH: 32 trajectories per wave; 33 is a second wave with one live pair of lanes): two
    register sets (3), a shared pair staged in LDS with helper lanes (5), per-lane LDS rows (5, batched sigma); N = 1, 2, 3; the
    observation placements; the coupled model; Lorenz63."""
    out = [make(gc.fhn(3, "kramer", "distinct", B=B)) for B in (1, 3, 33, 65)]
    out += [make(gc.fhn(5, "rodeo", "levels", B=B)) for B in (1, 3, 33)]
    out += [make(gc.fhn(5, "rodeo", "levels", B=33, batched_sigma=True))]
    out += [make(_short(3, "kramer", N, B=33), SHORT_NODES[N]) for N in (1, 2, 3)]
    out += [make(_short(5, "rodeo", N, B=3), SHORT_NODES[N]) for N in (1, 2, 3)]
    out += [make(_short(5, "rodeo", 2, B=3, batched_sigma=True), SHORT_NODES[2])]
    out += [make(gc.fhn(3, "kramer", "distinct", B=3), (0, 1, 20, 21, 40)), make(gc.fhn(3, "kramer", "distinct"), ())]
    out += [make(gc.fhn(3, "kramer", "distinct", B=3), (0, 13, 27, 40), model="coupled")]
    out += [make(gc.lorenz(3, "rodeo", "distinct", B=5))]
    return out


def mv_cases():
    """The batched solve_mv_nn_grid cases (the store form: one lane per trajectory; 65 is a second wave with one live lane)."""
    out = [make(gc.fhn(3, "kramer", "distinct", B=B)) for B in (1, 33, 65)]
    out += [make(gc.fhn(5, "rodeo", "levels", B=1)), make(gc.fhn(5, "rodeo", "levels", B=65)), make(gc.fhn(5, "rodeo", "levels", B=65, batched_sigma=True))]
    out += [make(_short(3, "kramer", N, B=65), SHORT_NODES[N]) for N in (1, 2, 3)]
    out += [make(_short(5, "rodeo", N, B=3), SHORT_NODES[N]) for N in (1, 2, 3)]
    out += [make(gc.fhn(3, "kramer", "distinct", B=3), (0, 1, 20, 21, 40))]
    out += [make(gc.fhn(3, "kramer", "distinct", B=3), (0, 13, 27, 40), model="coupled")]
    out += [make(gc.lorenz(3, "rodeo", "distinct", B=5))]
    return out


def all_cases():
    seen, out = set(), []
    for c in single_cases() + [yardstick_case()] + value_cases() + mv_cases():
        if id(c) not in seen:
            seen.add(id(c))
            out.append(c)
    return out


def rel(a, b):
    """Largest |a - b| relative to max(1, max|b|): tests/test_gpu_daltonng.py's measure for the value and both moments."""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def value_rel(a, b):
    """Per trajectory: |a - b| / max(1, |b|), the largest."""
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@functools.lru_cache(maxsize=None)
def moves(c):
    """The restatement (value, (mean, var)) and its own moves under a 1e-15 relative perturbation of R: (value relative, mean,
    var in ``rel``'s measure)."""
    v, mv = c.restate_value(), c.restate_mv()
    v2, mv2 = c.restate_value(1.0 + 1e-15), c.restate_mv(1.0 + 1e-15)
    return v, mv, (value_rel(v2, v), rel(mv2[0], mv[0]), rel(mv2[1], mv[1]))
