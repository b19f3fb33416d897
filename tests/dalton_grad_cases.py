"""
Test helper (not collected): the cases of tests/test_gpu_dalton_grad.py, in one place so that tests/test_oracle_dalton_grad.py can
check on the CPU, beforehand, that every one of them is a case the device bar can judge.  The problems, grids and observations
are tests/dalton_grid_cases.py's ``make`` on tests/grid_cases.py's problems (imported, not edited); a case here adds K directions.

Directions (``standard``): the unit theta directions, the unit ``ode_init`` directions, one mixed random direction and a zero
direction (K = n_theta + d p + 2).  ``small``: unit theta, one mixed, one zero (K = 5).  ``per_traj``: the mixed direction differs
per trajectory, shape (B, K, .).  Item counts that exercise the lane map, as (B, K): (1, 1); (3, 5); (11, 3), 33 items -- a second
wave with one live pair; (33, 1).
"""
import functools
import numpy as np
import grid_cases as gc
import dalton_grid_cases as dc
import dalton_grad_oracle as dgr
from oracle import priors


class GCase(dict):
    """A dalton_grid_cases.DCase under "case" with directions "dtheta" (K, n) / (B, K, n) and "dx0" (K, d, p) / (B, K, d, p), either
    may be None; "K", "B" (None: unbatched) and "label"."""
    __hash__ = object.__hash__

    @property
    def theta(self):
        return np.asarray(self["case"]["params"]["theta"], dtype=np.float64)

    def tangents(self):
        out = {}
        if self["dtheta"] is not None:
            out["theta"] = self["dtheta"]
        if self["dx0"] is not None:
            out["ode_init"] = self["dx0"]
        return out

    def restate(self, r_scale=1.0, forecast_vars=None):
        """(value (B,), dvalue (B, K)) of tests/dalton_grad_oracle.py."""
        c = self["case"]
        return dgr.dalton_grid_jvp(c["oracle_ode"], c["W"], c["x0"], c["t"], c["itg"], c.prior_at(priors.ibm_init, r_scale), c["y"],
                                   c["nodes"], c["D"], c["Om"], self.theta, self["dtheta"], self["dx0"], forecast_vars=forecast_vars)

    def moved(self, k, eps):
        """The DCase at (theta, ode_init) + eps * direction k: what the finite differences evaluate."""
        c = dc.DCase(self["case"])
        theta, x0 = self.theta, np.asarray(c["x0"], dtype=np.float64)
        if self["dtheta"] is not None:
            theta = theta + eps * self["dtheta"][..., k, :]
        if self["dx0"] is not None:
            x0 = x0 + eps * self["dx0"][..., k, :, :]
        c.update(params=dict(theta=theta), x0=x0)
        return c

    def device_jvp(self, fn, ode=None):
        c = self["case"]
        return fn(None, *c.device_args(ode), c["y"], c["t"][list(c["nodes"])], c["D"], c["Om"], self.tangents(), **c["params"])


def _mixed(rng, lead, n, d, p):
    """One random direction in theta and ode_init, of largest entry 1."""
    dth, dx = rng.standard_normal(lead + (1, n)), rng.standard_normal(lead + (1, d, p))
    scale = max(np.max(np.abs(dth)), np.max(np.abs(dx)))
    return dth / scale, dx / scale


@functools.lru_cache(maxsize=None)
def grad_case(case, kind="standard", seed=1):
    d, p = case["W"].shape[-3], case["p"]
    n = np.shape(case["params"]["theta"])[-1]
    B = case["B"]
    rng = np.random.default_rng(seed)
    if kind == "standard":                                           # unit theta, unit ode_init, mixed, zero
        mth, mx = _mixed(rng, (), n, d, p)
        dth = np.concatenate([np.eye(n), np.zeros((d * p, n)), mth, np.zeros((1, n))])
        dx = np.concatenate([np.zeros((n, d, p)), np.eye(d * p).reshape(d * p, d, p), mx, np.zeros((1, d, p))])
    elif kind == "small":                                            # unit theta, mixed, zero: K = n + 2
        mth, mx = _mixed(rng, (), n, d, p)
        dth = np.concatenate([np.eye(n), mth, np.zeros((1, n))])
        dx = np.concatenate([np.zeros((n, d, p)), mx, np.zeros((1, d, p))])
    elif kind == "per_traj":                                         # the same with a mixed direction of every trajectory's own
        mth, mx = _mixed(rng, (B,), n, d, p)
        dth = np.concatenate([np.broadcast_to(np.eye(n), (B, n, n)), mth, np.zeros((B, 1, n))], axis=1)
        dx = np.concatenate([np.zeros((B, n, d, p)), mx, np.zeros((B, 1, d, p))], axis=1)
    elif kind == "theta":                                            # unit theta alone: no ode_init key
        dth, dx = np.eye(n), None
    elif kind == "one":                                              # K = 1: the mixed direction
        dth, dx = _mixed(rng, (), n, d, p)
    elif kind == "theta0":                                           # K = 1: the first unit theta direction
        dth, dx = np.eye(n)[:1], None
    else:
        raise ValueError(kind)
    K = dth.shape[-2]
    return GCase(case=case, dtheta=dth, dx0=dx, K=K, B=B, kind=kind, label=f"{case['label']} | {kind} K={K}")


def zero_directions(g):
    """Indices of the directions of ``g`` that are zero in every trajectory."""
    out = []
    for k in range(g["K"]):
        z = (g["dtheta"] is None or not np.any(g["dtheta"][..., k, :])) and (g["dx0"] is None or not np.any(g["dx0"][..., k, :, :]))
        if z:
            out.append(k)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """Every dalton_grid_jvp case of tests/test_gpu_dalton_grad.py."""
    make, fhn = dc.make, gc.fhn
    out = [grad_case(make(fhn(3, "kramer", kind))) for kind in ("distinct", "levels")]
    out += [grad_case(make(fhn(3, "rodeo", "distinct"))), grad_case(make(fhn(3, "schober", "levels", t_max=2.0)))]
    out += [grad_case(make(fhn(2, "rodeo", "levels", B=3)), "per_traj")]                              # (3, 5)
    # Lorenz63 on [0, 0.4]: on grid_cases' horizon 0.8 the two Richardson estimates of the value restatement disagree by 1.8e-7 of
    # max |grad| (a chaotic system: the difference quotient's own error), a bar above 1e-6; on 0.4 they disagree by 5.5e-9
    out += [grad_case(make(gc.lorenz(3, "rodeo", "distinct", t_max=0.4, B=5)), "theta")]
    out += [grad_case(make(fhn(3, "kramer", "levels", B=3, batched_sigma=True)), "small")]
    out += [grad_case(make(dc._short(3, "kramer", N), dc.SHORT_NODES[N]), "small") for N in (1, 2, 3)]
    out += [grad_case(make(fhn(3, "kramer", "distinct"), (0, 1, 20, 21, 40)))]
    out += [grad_case(dc.times_case(), "per_traj")]
    out += [grad_case(make(fhn(3, "kramer", "distinct", B=1)), "one")]                                # (1, 1)
    out += [grad_case(make(fhn(3, "kramer", "distinct", B=11)), "theta")]                             # (11, 3): 33 items
    # (33, 1).  A unit direction: with K = 1 the yardstick max |grad| is the one derivative itself, and along a random direction of
    # its own a trajectory can have a derivative 400 times smaller than its neighbours' (6.6 against 2.8e3), which no difference
    # quotient resolves to 1e-7 of itself (the Richardson estimates disagreed by 2.6e-7 there)
    out += [grad_case(make(fhn(3, "kramer", "distinct", B=33)), "theta0")]
    # the remaining instances that ship: three blocks through the Jacobian dual, and n_bstate = 2 with kramer and schober
    out += [grad_case(make(gc.lorenz(3, "kramer", "distinct", t_max=0.4, B=5)), "small"),
            grad_case(make(gc.lorenz(2, "kramer", "levels", t_max=0.4)), "small")]
    out += [grad_case(make(fhn(2, "kramer", "distinct", B=3)), "small"), grad_case(make(fhn(2, "schober", "levels", t_max=2.0)), "small")]
    return out
