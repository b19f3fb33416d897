"""
Test helper (not collected): the problems and grids of tests/test_gpu_grid.py, in one place so that tests/test_oracle_grid.py
can check on the CPU, beforehand, that every one of them is a case the device bars can judge: the restatement's own move under
a 1e-15 relative perturbation of R must stay below the bar.

Grids over N steps on [0, t_max], all with h_max / h_min <= 8:
  "levels"    runs of steps of relative length 1, 1/2, 1/4 (three slots);
  "distinct"  N distinct steps 2^U(-1.5, 1.5) (``default_rng(3)``), N slots;
  "uniform"   ``np.linspace``, one slot.
"""
import functools
import numpy as np
import rodeo_amd as ra
from rodeo_amd import interrogate as ri
from oracle import odes, interrogations as oi, priors
import grid_oracle as go

ITG = {"kramer": (ri.interrogate_kramer, oi.interrogate_kramer), "rodeo": (ri.interrogate_rodeo, oi.interrogate_rodeo),
       "schober": (ri.interrogate_schober, oi.interrogate_schober),
       "chkrebtii": (functools.partial(ri.interrogate_chkrebtii, kalman_type="standard"),
                     functools.partial(oi.interrogate_chkrebtii, kalman_type="standard"))}
THETA = np.array([0.2, 0.2, 3.0])
SIGMA = np.array([0.5, 0.3])
LORENZ = np.array([28.0, 10.0, 8.0 / 3.0])
GRIDS = ("levels", "distinct", "uniform")
T_MAX = {2: 4.0, 3: 4.0, 4: 4.0, 5: 4.0, 6: 1.0}      # horizon of the N = 40 cases: at 6 the restatement is not finite on [0, 4]


def grid(kind, N, t_max):
    if kind == "uniform":
        return np.linspace(0.0, t_max, N + 1)
    if kind == "levels":
        w = np.array([(1.0, 0.5, 0.25, 0.5)[(n // 3) % 4] for n in range(N)])
    else:
        w = 2.0 ** np.random.default_rng(3).uniform(-1.5, 1.5, N)
    return np.concatenate([[0.0], np.cumsum(w * (t_max / w.sum()))])    # (a level's steps differ in their last bits: one slot)


class Case(dict):
    """One problem: device and oracle right-hand sides, weight, initial value(s), grid, sigma, params, interrogation name."""
    __hash__ = object.__hash__

    def prior_at(self, lib=ra.ibm_init, r_scale=1.0):
        sigma = self["sigma"]

        def at(h):
            if sigma.ndim == 2 and lib is priors.ibm_init:              # (the oracle's takes one trajectory's sigma)
                pairs = [lib(h, self["p"], s) for s in sigma]
                Q, R = pairs[0][0], np.stack([pair[1] for pair in pairs])
            else:
                Q, R = lib(h, self["p"], sigma)
            return Q, R * r_scale
        return at

    @property
    def yardstick(self):
        """Does this case lean on the perturbation yardstick?  n_bstate = 6 only: the mean's highest
        derivatives are of order 1e5 there and the restatement itself moves by up to 9e-6 under R (1 + 1e-15)."""
        return self["p"] == 6

    def device_args(self, ode=None):
        return (ode or self["ode"], self["W"], self["x0"], self["t"], ITG[self["itg"]][0], self.prior_at())

    def restate_mv(self, r_scale=1.0):
        return go.solve_mv_grid(self["key"], self["oracle_ode"], self["W"], self["x0"], self["t"], ITG[self["itg"]][1],
                                self.prior_at(priors.ibm_init, r_scale), **self["params"])

    def restate_sim(self, key, r_scale=1.0):
        return go.solve_sim_grid(key, self["oracle_ode"], self["W"], self["x0"], self["t"], ITG[self["itg"]][1],
                                 self.prior_at(priors.ibm_init, r_scale), **self["params"])


@functools.lru_cache(maxsize=None)
def fhn(p, itg, kind, N=40, t_max=4.0, B=None, batched_sigma=False, key=None):
    """The quick start's FitzHugh-Nagumo problem; a batch varies theta, the initial value and (batched_sigma) sigma."""
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    if B is None:
        theta, v0, sigma = THETA, np.array([-1.0, 1.0]), SIGMA
    else:
        k = np.arange(B)[:, None]
        theta, v0 = THETA * (1 + 0.002 * k), np.array([-1.0, 1.0]) + 0.001 * k
        sigma = SIGMA * (1 + 0.01 * k) if batched_sigma else SIGMA
    return Case(ode=ra.ode.fitzhugh_nagumo, oracle_ode=odes.fitzhugh_nagumo, W=W, x0=init(v0, 0.0, theta=theta), t=grid(kind, N, t_max),
                sigma=sigma, params=dict(theta=theta), itg=itg, p=p, key=key, B=B,
                label=f"fhn {itg} p={p} {kind} N={N} t_max={t_max} B={B}{' sigma batched' if batched_sigma else ''}")


@functools.lru_cache(maxsize=None)
def lorenz(p, itg, kind, N=40, t_max=0.8, B=None):
    W, init = ra.utils.first_order_pad(ra.ode.lorenz63, 3, p)
    theta = LORENZ if B is None else LORENZ * (1 + 0.002 * np.arange(B)[:, None])
    v0 = np.array([-12.0, -5.0, 38.0])
    x0 = init(v0 if B is None else v0 + 0.01 * np.arange(B)[:, None], 0.0, theta=theta)
    return Case(ode=ra.ode.lorenz63, oracle_ode=odes.lorenz63, W=W, x0=x0, t=grid(kind, N, t_max), sigma=np.array([5.0, 4.0, 6.0]),
                params=dict(theta=theta), itg=itg, p=p, key=None, B=B, label=f"lorenz {itg} p={p} {kind} N={N} B={B}")


@functools.lru_cache(maxsize=None)
def higher(p, itg, kind, N=40, t_max=4.0):
    """x'' = sin 2t - x: the right-hand side reads the time."""
    W = np.zeros((1, 1, p))
    W[0, 0, 2] = 1.0
    x0 = np.zeros((1, p))
    x0[0, :3] = [-1.0, 0.0, 1.0]
    return Case(ode=ra.ode.higher_order, oracle_ode=odes.higher_order, W=W, x0=x0, t=grid(kind, N, t_max), sigma=np.array([0.01]),
                params={}, itg=itg, p=p, key=None, B=None, label=f"higher_order {itg} p={p} {kind} N={N}")


def mv_cases():
    """Every solve_mv_grid case of tests/test_gpu_grid.py."""
    out = [fhn(p, "rodeo", kind, t_max=T_MAX[p]) for p in (2, 3, 4, 5, 6) for kind in GRIDS]
    out += [fhn(p, "kramer", kind) for p in (3, 4) for kind in GRIDS]
    out += [fhn(3, "schober", kind, t_max=2.0) for kind in GRIDS]
    out += [fhn(3, "chkrebtii", kind, key=11) for kind in ("levels", "distinct")]
    out += [fhn(p, itg, kind, B=B) for p, itg, kind in ((3, "kramer", "distinct"), (5, "rodeo", "levels")) for B in (1, 3, 65)]
    out += [fhn(5, "rodeo", "distinct", B=3)]
    out += [fhn(p, itg, "levels", B=65, batched_sigma=True) for p, itg in ((3, "kramer"), (5, "rodeo"))]
    out += [fhn(3, "kramer", "distinct", N=N, t_max=0.1 * N, B=B) for N in (1, 2, 3) for B in (None, 65)]
    out += [fhn(5, "rodeo", "distinct", N=N, t_max=0.1 * N, B=3) for N in (1, 2, 3)]
    out += [lorenz(p, itg, "distinct", B=B) for p, itg, B in ((3, "rodeo", None), (3, "kramer", 5), (4, "rodeo", 5))]
    out += [higher(p, "kramer", "distinct") for p in (3, 4, 6)]
    return out


def sim_cases():
    """Every solve_sim_grid case: (case, key)."""
    return [(fhn(3, "rodeo", "distinct", B=65), 42), (fhn(2, "kramer", "levels", B=3), 42), (fhn(5, "rodeo", "distinct", t_max=1.0, B=3), 7),
            (fhn(3, "rodeo", "distinct", N=2, t_max=0.2, B=65), 5), (fhn(3, "rodeo", "distinct", N=1, t_max=0.1, B=3), 5),
            (fhn(3, "rodeo", "distinct", N=3, t_max=0.3), 5), (fhn(3, "chkrebtii", "levels", B=3, key=9), 9)]


def mv_bars(c):
    """tests/test_gpu_solver.py's: |mean - restatement| absolute -- 1e-9, Lorenz63 (chaotic) 1e-6 -- and var of max|var|."""
    return (1e-6 if c["ode"] is ra.ode.lorenz63 else 1e-9), 1e-9


def mv_moves(c):
    """The restatement, and its own move (mean absolute, var of max|var|) under a 1e-15 relative perturbation of R."""
    m, v = c.restate_mv()
    m2, v2 = c.restate_mv(1.0 + 1e-15)
    return (m, v), float(np.max(np.abs(m2 - m))), float(np.max(np.abs(v2 - v)) / np.max(np.abs(v)))


def sim_bar(p):
    return 1e-7 if p <= 4 else 1e-5                      # of max|x| (tests/test_gpu_draws.py: test_gpu_evidence._bar)
