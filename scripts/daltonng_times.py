"""Kernel times of dalton.daltonng and dalton.solve_mv_nn on the headline shape (FitzHugh-Nagumo, p = 3, 4000 steps, 1024
parameter sets, 41 Poisson observations per variable, kramer), next to Gaussian dalton of the same shape (scripts/dalton_times.py)."""
import sys, os, time, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rodeo_amd as ra
import bench
import rodeo_amd.inference.dalton  # noqa: F401
from rodeo_amd.trace import gammaln
dalton_mod = sys.modules["rodeo_amd.inference.dalton"]
W, x0, theta, prior = bench.make_problem(ra, 0)
n_obs = 41
obs_t = np.linspace(0, 40, n_obs)
rng = np.random.default_rng(0)
Yc = rng.poisson(1.5, size=(n_obs, 2, 1)).astype(np.float64)
Y = rng.standard_normal((n_obs, 2, 1))
Dw = np.zeros((n_obs, 2, 1, 3)); Dw[..., 0] = 1.0
Om = np.full((n_obs, 2, 1, 1), 0.005)


def poisson_loglik(obs_data_i, ode_data_i, ind, **params):
    eta = 0.1 + 0.5 * ode_data_i[:, 0]
    y = obs_data_i.flatten()
    return np.sum(y * eta - np.exp(eta) - gammaln(y + 1.0))


dev = ra.device.default_device()
args = (ra.ode.fitzhugh_nagumo, W, x0, 0.0, 40.0, 4000, ra.interrogate.interrogate_kramer, prior)
for name, call in [("daltonng", lambda: dalton_mod.daltonng(None, *args, Yc, obs_t, poisson_loglik, theta=theta)),
                   ("dalton.solve_mv_nn", lambda: dalton_mod.solve_mv_nn(None, *args, Yc, obs_t, poisson_loglik, theta=theta)),
                   ("dalton", lambda: dalton_mod.dalton(None, *args, Y, obs_t, Dw, Om, theta=theta))]:
    for rep in range(3):
        dev.sync(); t0 = time.perf_counter()
        dev.profile_enable(True)
        out = call()
        dev.sync(); t1 = time.perf_counter()
        head = out[:2] if name in ("dalton", "daltonng") else np.asarray(out[0]).shape
        print("%s: wall ms %.2f" % (name, (t1 - t0) * 1e3), {k: round(v, 4) for k, v in dev.profile_last()}, head, flush=True)
