"""Times of fenrir_at on the headline shape (FitzHugh-Nagumo, p = 3, 4000 steps, 1024 parameter sets, 41 observations per
variable, kramer) with all 41 times between grid nodes, per call and per kernel, next to fenrir on the same data (which it
snaps onto the grid).  Run it on this build and on the parent commit (there the fenrir_at part is skipped): fenrir's kernels
are unchanged, so its two figures should agree.  The first repeat of each call is the warm-up (plan, uploads, code objects)
and is shown, not used.  Appends its lines to profiles/fenrir_at_times.txt.

    python scripts/fenrir_at_times.py [label]
"""
import sys, os, time, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rodeo_amd as ra
import bench
import rodeo_amd.inference.fenrir  # noqa: F401
fenrir_mod = sys.modules["rodeo_amd.inference.fenrir"]
label = sys.argv[1] if len(sys.argv) > 1 else "this build"
W, x0, theta, prior = bench.make_problem(ra, 0)
n_obs, N, t_max = 41, 4000, 40.0
dt = t_max / N
obs_t = (np.linspace(40, 3960, n_obs).round() + 0.37) * dt                   # 41 times, each 0.37 dt behind a node
rng = np.random.default_rng(0)
Y = rng.standard_normal((n_obs, 2, 1))
Dw = np.zeros((n_obs, 2, 1, 3)); Dw[..., 0] = 1.0
Om = np.full((n_obs, 2, 1, 1), 0.005)
sigma = np.array([0.1, 0.1])                                                   # bench.make_problem's prior scale
assert np.allclose(ra.ibm_init(dt, 3, sigma)[1], prior[1], rtol=1e-12), "bench.make_problem's prior is not ibm_init(dt, 3, 0.1)"
dev = ra.device.default_device()
args = (ra.ode.fitzhugh_nagumo, W, x0, 0.0, t_max, N, ra.interrogate.interrogate_kramer, prior)
calls = [("fenrir (snapped)", lambda: fenrir_mod.fenrir(None, *args, Y, obs_t, Dw, Om, theta=theta))]
if hasattr(fenrir_mod, "fenrir_at"):
    calls.append(("fenrir_at", lambda: fenrir_mod.fenrir_at(None, *args, Y, obs_t, Dw, Om, lambda h: ra.ibm_init(h, 3, sigma),
                                                            theta=theta)))
lines = []
for name, call in calls:
    for rep in range(6):
        dev.sync(); t0 = time.perf_counter()
        dev.profile_enable(True)
        out = call()
        dev.sync(); t1 = time.perf_counter()
        line = "%s | %s%s: wall ms %.2f kernels %s head %s" % (label, name, " (warm-up)" if rep == 0 else "", (t1 - t0) * 1e3,
                                                                {k: round(v, 4) for k, v in dev.profile_last()}, out[:2])
        print(line, flush=True)
        lines.append(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "fenrir_at_times.txt"), "a") as f:
    f.write("\n".join(lines) + "\n")
