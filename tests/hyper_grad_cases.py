"""
Test helper (not collected): the cases of tests/test_gpu_hyper_grad.py, in one place so that tests/test_oracle_hyper_grad.py can
check on the CPU, beforehand, that every one of them is a case the device bar can judge.

The problems, grids, nodes and observations are those of tests/dalton_grad_cases.py's and tests/fenrir_grad_cases.py's ``cases()``
(imported, not edited): N = 1, 2, 3 with SHORT_NODES, nodes (0, 1, 20, 21, 40), the four-slot ``times_case``, a batched sigma (R per
lane), Lorenz63's three blocks, schober on t_max = 2.  Each case keeps its problem and gets new directions, by the base case's kind:

  standard, small, theta -> "standard": the unit theta directions, the unit ``log_sigma`` directions (d), the unit ``log_obs_var``
                            directions (d), one mixed random direction over theta, ode_init, log_sigma and log_obs_var, one zero
                            direction: K = n_theta + 2 d + 2 (9 for FitzHugh-Nagumo, 11 for Lorenz63)
  per_traj               -> "per_traj": the same, the mixed direction of every trajectory's own -- all four arrays (B, K, .)
  one     (B = 1)        -> "one": one random direction in log_sigma and log_obs_var alone: 1 item.  (Not the mixed direction over
                            all four kinds: that one is differenced with h = 1e-4, where the difference quotients of a value of
                            4.5e3 are quantised to 9e-9 and the two Richardson estimates of a single number came out EQUAL for
                            Fenrir -- a bar of 0.  With h = 1e-3 their disagreement is resolved.)
  theta0  (B = 33)       -> "common": the common ``log_obs_var`` direction (1, .., 1) alone: 33 items
and ``fhn(3, "kramer", "distinct", B=13)`` with "small" (unit theta, mixed, zero: K = 5) is in both lists: 65 items.
"""
import functools
import numpy as np
import grid_cases as gc
import dalton_grid_cases as dgc
import dalton_grad_cases as gcs
import fenrir_grad_cases as fgcs
import fenrir_grid_cases as fc
import hyper_grad_oracle as hgo
from oracle import priors

KIND_OF = {"standard": "standard", "small": "standard", "theta": "standard", "per_traj": "per_traj", "one": "one", "theta0": "common"}
HYPER = ("log_sigma", "log_obs_var")


class HCase(dict):
    """A problem ("case": a dalton_grid_cases.DCase) of one family ("dalton" / "fenrir") with K directions: "dtheta" (K, n), "dx0"
    (K, d, p), "dls" and "dlo" (K, d), each with a leading B for "per_traj"; "K", "B" (None: unbatched), "kind", "label"."""
    __hash__ = object.__hash__
    NAMES = (("theta", "dtheta"), ("ode_init", "dx0"), ("log_sigma", "dls"), ("log_obs_var", "dlo"))

    @property
    def theta(self):
        return np.asarray(self["case"]["params"]["theta"], dtype=np.float64)

    def tangents(self, names=None):
        return {name: self[key] for name, key in self.NAMES if self[key] is not None and (names is None or name in names)}

    def restate(self, r_scale=1.0, forecast_vars=None):
        """(value (B,), dvalue (B, K)) of tests/hyper_grad_oracle.py."""
        c = self["case"]
        fn = hgo.dalton_grid_jvp if self["family"] == "dalton" else hgo.fenrir_grid_jvp
        return fn(c["oracle_ode"], c["W"], c["x0"], c["t"], c["itg"], c.prior_at(priors.ibm_init, r_scale), c["y"], c["nodes"],
                  c["D"], c["Om"], self.theta, self["dtheta"], self["dx0"], self["dls"], self["dlo"], forecast_vars=forecast_vars)

    def value_case(self, **changes):
        """The problem as the family's value case (``restate_value`` is the untouched value restatement's), with ``changes``."""
        c = (dgc.DCase if self["family"] == "dalton" else fc.FCase)(self["case"])
        c.update(**changes)
        return c

    def moved_value(self, k, eps, forecast_vars=None):
        """The value restatement (B,) at the point moved by eps along direction k -- theta and ode_init by addition, sigma_b ->
        sigma_b e^(eps l._b) through ``ibm_init``'s sigma, Om[:, b] -> e^(eps w._b) Om[:, b]: the definition, not the device's
        shortcut.  A per-trajectory ``log_obs_var`` direction is evaluated trajectory by trajectory (the restatement has one Om)."""
        c = self["case"]
        theta, x0, sigma = self.theta, np.asarray(c["x0"], dtype=np.float64), np.asarray(c["sigma"], dtype=np.float64)
        if self["dtheta"] is not None:
            theta = theta + eps * self["dtheta"][..., k, :]
        if self["dx0"] is not None:
            x0 = x0 + eps * self["dx0"][..., k, :, :]
        if self["dls"] is not None:
            sigma = sigma * np.exp(eps * self["dls"][..., k, :])
        changes = dict(params=dict(theta=theta), x0=x0, sigma=sigma)
        dlo = self["dlo"]
        if dlo is None:
            return np.atleast_1d(self.value_case(**changes).restate_value(forecast_vars=forecast_vars))
        if dlo.ndim == 2:
            Om = c["Om"] * np.exp(eps * dlo[k])[None, :, None, None]
            return np.atleast_1d(self.value_case(Om=Om, **changes).restate_value(forecast_vars=forecast_vars))
        out = np.zeros(dlo.shape[0])
        for b in range(dlo.shape[0]):
            Om = c["Om"] * np.exp(eps * dlo[b, k])[None, :, None, None]
            out[b] = np.atleast_1d(self.value_case(Om=Om, **changes).restate_value(forecast_vars=forecast_vars))[b]
        return out

    def device_jvp(self, fn, ode=None, names=None, columns=None):
        """``fn`` (a ``*_grid_jvp``) on the case; ``names``: these keys of the tangents only; ``columns``: these directions only."""
        c = self["case"]
        tangents = self.tangents(names)
        if columns is not None:
            tangents = {name: v[..., columns, :] if name != "ode_init" else v[..., columns, :, :] for name, v in tangents.items()}
        return fn(None, *c.device_args(ode), c["y"], c["t"][list(c["nodes"])], c["D"], c["Om"], tangents, **c["params"])


def _mixed(rng, lead, n, d, p):
    """One random direction over all four kinds, of largest entry 1."""
    parts = [rng.standard_normal(lead + (1,) + s) for s in ((n,), (d, p), (d,), (d,))]
    scale = max(np.max(np.abs(a)) for a in parts)
    return [a / scale for a in parts]


@functools.lru_cache(maxsize=None)
def hyper_case(case, family, kind="standard", seed=2):
    d, p = case["W"].shape[-3], case["p"]
    n = np.shape(case["params"]["theta"])[-1]
    B = case["B"]
    rng = np.random.default_rng(seed)
    z = np.zeros
    if kind in ("standard", "per_traj"):
        lead = (B,) if kind == "per_traj" else ()
        m = _mixed(rng, lead, n, d, p)
        units = [np.concatenate([np.eye(n), z((2 * d, n))]), z((n + 2 * d, d, p)), np.concatenate([z((n, d)), np.eye(d), z((d, d))]),
                 np.concatenate([z((n + d, d)), np.eye(d)])]
        dirs = [np.concatenate([np.broadcast_to(u, lead + u.shape), mm, z(lead + (1,) + u.shape[1:])], axis=len(lead))
                for u, mm in zip(units, m)]
    elif kind == "small":                                            # unit theta, mixed, zero
        m = _mixed(rng, (), n, d, p)
        units = [np.eye(n), z((n, d, p)), z((n, d)), z((n, d))]
        dirs = [np.concatenate([u, mm, z((1,) + u.shape[1:])]) for u, mm in zip(units, m)]
    elif kind == "one":                                              # K = 1: a random direction in the two log-scales alone
        m = _mixed(rng, (), n, d, p)
        scale = max(np.max(np.abs(m[2])), np.max(np.abs(m[3])))
        dirs = [None, None, m[2] / scale, m[3] / scale]
    elif kind == "common":                                           # K = 1: every block's observation variances together
        dirs = [None, None, None, np.ones((1, d))]
    else:
        raise ValueError(kind)
    K = dirs[3].shape[-2]                                            # (every kind has a log_obs_var array)
    return HCase(case=case, family=family, dtheta=dirs[0], dx0=dirs[1], dls=dirs[2], dlo=dirs[3], K=K, B=B, kind=kind,
                 label=f"{family} | {case['label']} | {kind} K={K}")


def zero_directions(g):
    """Indices of the directions of ``g`` that are zero in every trajectory."""
    arrays = [(g[key], 2 if key == "dx0" else 1) for _, key in HCase.NAMES if g[key] is not None]
    return [k for k in range(g["K"]) if not any(np.any(np.take(a, k, axis=a.ndim - 1 - nt)) for a, nt in arrays)]


def hyper_columns(g):
    """Indices of the directions of ``g`` with a non-zero ``log_sigma`` or ``log_obs_var`` entry."""
    arrays = [g[key] for key in ("dls", "dlo") if g[key] is not None]
    return [k for k in range(g["K"]) if any(np.any(a[..., k, :]) for a in arrays)]


@functools.lru_cache(maxsize=None)
def dalton_cases():
    out = [hyper_case(g["case"], "dalton", KIND_OF[g["kind"]]) for g in gcs.cases()]
    out += [hyper_case(dgc.make(gc.fhn(3, "kramer", "distinct", B=13)), "dalton", "small")]           # (13, 5): 65 items
    return out


@functools.lru_cache(maxsize=None)
def fenrir_cases():
    out = []
    for g in fgcs.cases():
        kind = "small" if (g["B"], g["kind"]) == (13, "small") else KIND_OF[g["kind"]]                # (13, 5): 65 items
        out.append(hyper_case(g["case"], "fenrir", kind))
    return out


def cases():
    return dalton_cases() + fenrir_cases()
