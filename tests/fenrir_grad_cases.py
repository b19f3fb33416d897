"""
Test helper (not collected): the cases of tests/test_gpu_fenrir_grad.py, in one place so that tests/test_oracle_fenrir_grad.py can
check on the CPU, beforehand, that every one of them is a case the device bar can judge.

The 19 cases of tests/dalton_grad_cases.py, re-read as Fenrir cases -- the same problems, grids, nodes and directions: node 0 is
observed in three of them (Fenrir conditions on it; DALTON only adds a density), node N is unobserved in the ``times_case``, N = 1,
2, 3, n_bstate 2 and 3, Lorenz63's three blocks (the ordered block sum), a batched sigma, and (B, K) = (1, 1), (3, 5), (11, 3) --
33 items, 66 backward lanes: the backward kernel's second wave -- and (33, 1).  Three more:
  * ``fhn(3, "kramer", "distinct", B=13)`` with "small" (K = 5): 65 items, a second forward wave with one live item;
  * two cases at 100 x the prior scale.  In all the others the state's share of every y forecast variance is negligible next to
    Omega = 2.5e-3, so Sigma. hardly reaches the value; at x 100 the y forecast variances reach 17.8 (rodeo) and 1.6e-2 (kramer).
"""
import functools
import grid_cases as gc
import dalton_grid_cases as dgc
import dalton_grad_cases as gcs
import fenrir_grid_cases as fc
import fenrir_grad_oracle as fgr
from oracle import priors


class FGCase(gcs.GCase):
    """A dalton_grad_cases.GCase restated by tests/fenrir_grad_oracle.py; its finite differences are tests/fenrir_grid_oracle.py's."""
    __hash__ = object.__hash__

    def restate(self, r_scale=1.0, forecast_vars=None):
        """(value (B,), dvalue (B, K)) of tests/fenrir_grad_oracle.py."""
        c = self["case"]
        return fgr.fenrir_grid_jvp(c["oracle_ode"], c["W"], c["x0"], c["t"], c["itg"], c.prior_at(priors.ibm_init, r_scale), c["y"],
                                   c["nodes"], c["D"], c["Om"], self.theta, self["dtheta"], self["dx0"], forecast_vars=forecast_vars)

    def value_case(self):
        """The case as tests/fenrir_grid_cases.py's FCase: ``restate_value`` is fenrir_grid_oracle's."""
        return fc.FCase(self["case"])

    def moved(self, k, eps):
        """The FCase at (theta, ode_init) + eps * direction k: what the finite differences evaluate."""
        return fc.FCase(super().moved(k, eps))


def fenrir_case(case, kind="standard"):
    return FGCase(gcs.grad_case(case, kind))


zero_directions = gcs.zero_directions


@functools.lru_cache(maxsize=None)
def cases():
    """Every fenrir_grid_jvp case of tests/test_gpu_fenrir_grad.py."""
    out = [FGCase(g) for g in gcs.cases()]
    out += [fenrir_case(dgc.make(gc.fhn(3, "kramer", "distinct", B=13)), "small")]                    # (13, 5): 65 items
    out += [fenrir_case(dgc.make(gc.fhn(3, "rodeo", "distinct", B=3), scale=100.0)),
            fenrir_case(dgc.make(gc.fhn(3, "kramer", "levels"), scale=100.0))]
    return out
