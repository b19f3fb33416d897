"""
Test helper (not collected): the cases of tests/test_gpu_calib_grid.py -- problems and grids from tests/grid_cases.py -- in one
place so that tests/test_oracle_calib_grid.py can check on the CPU, beforehand, that every one of them is a case the device
bars can judge: the restatement's own move under a 1e-15 relative perturbation of every R_n must stay below the bar.

Which pair regime of the forward walk a case hits (grid_calib_kernels.hpp): FitzHugh-Nagumo n_bstate 2, 3, 4 and Lorenz63 at 3 keep
two register sets; n_bstate 5, 6 and Lorenz63 at 4 stage a shared pair in LDS, or a row per lane with a batched sigma.
"""
import functools
import numpy as np
from oracle import priors
import calib_grid_oracle as cgo
import grid_cases as gc
from grid_cases import fhn, lorenz


def _short(p, itg, B):
    return [fhn(p, itg, "distinct", N=N, t_max=0.1 * N, B=B) for N in (1, 2, 3)]


def evidence_cases():
    out = [fhn(p, "kramer", kind) for p in (2, 3, 4) for kind in ("levels", "distinct")]
    out += [fhn(3, "rodeo", "levels"), fhn(3, "schober", "levels", t_max=2.0), fhn(4, "rodeo", "distinct")]
    out += [fhn(5, "rodeo", "levels"), fhn(5, "kramer", "distinct", B=3), fhn(5, "rodeo", "levels", B=65, batched_sigma=True)]
    out += [fhn(3, "kramer", "distinct", B=B) for B in (1, 3, 65)] + [fhn(3, "kramer", "levels", B=65, batched_sigma=True)]
    out += _short(3, "kramer", 65) + _short(5, "rodeo", 3) + _short(3, "kramer", None)
    out += [lorenz(3, "rodeo", "distinct"), lorenz(3, "kramer", "distinct", B=5), lorenz(4, "rodeo", "distinct", B=5)]
    out += [fhn(6, "rodeo", "levels", t_max=1.0)]
    return out


def dynamic_cases():
    """(p = 4 under kramer on [0, 4]: on [0, 1] the restatement's sqrt(scale) moves by 1e-8 under R (1 + 1e-15))"""
    out = [fhn(p, "kramer", kind) for p in (2, 3, 4) for kind in ("levels", "distinct")]
    out += [fhn(3, "rodeo", "levels"), fhn(3, "schober", "levels", t_max=2.0)]
    # (n_bstate 5 with a batched sigma on [0, 1]: on [0, 4] the restatement is not finite for every trajectory of the batch)
    out += [fhn(5, "rodeo", "levels"), fhn(5, "rodeo", "distinct", B=3), fhn(5, "rodeo", "levels", t_max=1.0, B=65, batched_sigma=True)]
    out += [fhn(3, "kramer", "distinct", B=B) for B in (1, 3, 65)] + [fhn(3, "kramer", "levels", B=65, batched_sigma=True)]
    out += _short(3, "kramer", 65) + _short(5, "rodeo", 3) + _short(3, "kramer", None)
    out += [lorenz(3, "rodeo", "distinct"), lorenz(3, "kramer", "distinct", B=5)]
    return out


def sim_cases():
    """(case, key): the sampler where 1e-7 absolute can tell a fault from rounding (tests/test_gpu_dynamic.py): rodeo at
    n_bstate 3, kramer at 2.  The horizons are short: under R (1 + 1e-15) the restatement's own path moves by 1.2e-3 on [0, 4]
    and 1.3e-7 on [0, 1] for the first case (1.2e-9 on [0, 0.5]), by 2.0e-8 for the second."""
    long = [(fhn(3, "rodeo", "distinct", t_max=0.5, B=65), 42), (fhn(2, "kramer", "levels", t_max=1.0, B=3), 42)]
    return long + [(c, 5) for c in _short(3, "rodeo", 3)]


def _args(c, r_scale):
    return (c["oracle_ode"], c["W"], c["x0"], c["t"], gc.ITG[c["itg"]][1], c.prior_at(priors.ibm_init, r_scale))


@functools.lru_cache(maxsize=None)
def restate_evidence(c, r_scale=1.0):
    """(logdens, quad, logdet) of a case, computed once and left unchanged (the cases are cached objects)."""
    return cgo.evidence(*_args(c, r_scale), **c["params"])


@functools.lru_cache(maxsize=None)
def restate_mv(c, r_scale=1.0, scale_min=0.0):
    return cgo.solve_mv_dynamic_grid(*_args(c, r_scale), scale_min=scale_min, **c["params"])


@functools.lru_cache(maxsize=None)
def restate_sim(c, key, r_scale=1.0):
    return cgo.solve_sim_dynamic_grid(key, *_args(c, r_scale), **c["params"])


def evidence_worst(got, ref):
    """largest difference of (logdens, quad, logdet) in units of max(1, |ref|) (tests/test_gpu_evidence.py: _check)"""
    return max(float(np.max(np.abs(np.asarray(g) - w) / np.maximum(1.0, np.abs(w)))) for g, w in zip(got, ref))


def dynamic_diffs(got, ref):
    """tests/test_gpu_dynamic.py's _check: mean and var of the largest entry, sqrt(scale) of the block's largest, logdens of
    max(1, |ref|); ``got`` and ``ref`` as (mean, var, scale, logdens)."""
    (m, v, s, ld), (mr, vr, sr, ldr) = got, ref
    dm = float(np.max(np.abs(m - mr)) / np.max(np.abs(mr)))
    dv = float(np.max(np.abs(v - vr)) / np.max(np.abs(vr)))
    root, root_ref = np.sqrt(s), np.sqrt(sr)
    ds = float(np.max(np.abs(root - root_ref) / np.max(root_ref, axis=-2, keepdims=True)))
    dl = float(np.max(np.abs(np.asarray(ld) - ldr) / np.maximum(1.0, np.abs(ldr))))
    return dm, dv, ds, dl
