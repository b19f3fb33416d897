"""Kernel times of inference.dalton and dalton.solve_mv on the headline shape (FitzHugh-Nagumo, p = 3, 4000 steps, 1024
parameter sets, 41 observations per variable, kramer), next to the plain solve_mv of the same shape."""
import sys, os, time, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rodeo_amd as ra
import bench
import rodeo_amd.inference.dalton  # noqa: F401
dalton_mod = sys.modules["rodeo_amd.inference.dalton"]
W, x0, theta, prior = bench.make_problem(ra, 0)
n_obs = 41
obs_t = np.linspace(0, 40, n_obs)
rng = np.random.default_rng(0)
Y = rng.standard_normal((n_obs, 2, 1))
Dw = np.zeros((n_obs, 2, 1, 3)); Dw[..., 0] = 1.0
Om = np.full((n_obs, 2, 1, 1), 0.005)
dev = ra.device.default_device()
args = (ra.ode.fitzhugh_nagumo, W, x0, 0.0, 40.0, 4000, ra.interrogate.interrogate_kramer, prior)
for name, call in [("dalton", lambda: dalton_mod.dalton(None, *args, Y, obs_t, Dw, Om, theta=theta)),
                   ("dalton.solve_mv", lambda: dalton_mod.solve_mv(None, *args, Y, obs_t, Dw, Om, theta=theta)),
                   ("solve_mv", lambda: ra.solve_mv(None, *args, theta=theta))]:
    for rep in range(3):
        dev.sync(); t0 = time.perf_counter()
        dev.profile_enable(True)
        out = call()
        dev.sync(); t1 = time.perf_counter()
        head = out[:2] if name == "dalton" else np.asarray(out[0]).shape
        print("%s: wall ms %.2f" % (name, (t1 - t0) * 1e3), {k: round(v, 4) for k, v in dev.profile_last()}, head, flush=True)
