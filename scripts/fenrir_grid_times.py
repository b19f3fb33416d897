"""Kernel and wall times of fenrir_grid / fenrir.solve_mv_grid on the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2,
p = 3, kramer, 41 observations per variable) next to the yardsticks: fenrir's lane route (a plan with store_pred=True,
batch_minor=True: fwd_kernel + fenrir_bwd_kernel) and solve_mv_grid (grid_fwd_kernel + grid_bwd_mv_kernel) on the uniform grid.
Cases: (i) the uniform grid with the observations on every 100th node; (ii) the uniform nodes plus 41 times 0.37 dt behind a
node, put in by grid_with_times (the last one behind node N - 1).  Kernels are timed by the library's profile (HIP events
around each launch), the wall time around the whole Python call (prior_at runs per slot only); the first call of each kind is
discarded, five repeats follow.  Not a pass/fail number.  Appends its lines, under a header, to profiles/fenrir_grid_times.txt
or to the file named.

    python scripts/fenrir_grid_times.py [--root DIR] [--yardstick] [--label TEXT] [output file]

--yardstick times the yardsticks only; with --root DIR the package and bench.py are taken from another checkout (the parent
commit's, built), which is how the two are alternated in fresh processes.
"""
import argparse, os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
ap.add_argument("--yardstick", action="store_true")
ap.add_argument("--label", default="")
ap.add_argument("out", nargs="?", default=os.path.join(HERE, "profiles", "fenrir_grid_times.txt"))
opt = ap.parse_args()
sys.path.insert(0, os.path.abspath(opt.root))
import rodeo_amd as ra
import rodeo_amd.inference.fenrir  # noqa: F401
import bench
from rodeo_amd.inference.logpost import obs_index
from rodeo_amd.solve import cached_plan
fmod = sys.modules["rodeo_amd.inference.fenrir"]
HEADER = """# scripts/fenrir_grid_times.py on one MI355X: the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer, 41
# observations per variable), kernel ms (HIP events around each launch, profile_last) and wall ms of the Python call.  The first
# call of each kind is the warm-up, five repeats follow; every block of lines is one fresh process, this tree's and the parent
# commit's yardsticks alternating.
"""
W, x0, theta, prior = bench.make_problem(ra, 0)
N, t_max = bench.N_STEPS, bench.T_MAX
p = W.shape[-1]
dev = ra.device.default_device()
itg = ra.interrogate.interrogate_kramer
ode = ra.ode.fitzhugh_nagumo
t_uniform = np.linspace(0.0, t_max, N + 1)
dt = t_max / N
n_obs = 41
on_nodes = t_uniform[::N // (n_obs - 1)]
rng = np.random.default_rng(0)
y = rng.standard_normal((n_obs, 2, 1)) * 0.3
D = np.zeros((n_obs, 2, 1, p))
D[..., 0, 0] = 1.0
Om = np.full((n_obs, 2, 1, 1), 0.05 ** 2)


def prior_at(h):
    return ra.ibm_init(h, p, np.array([0.1, 0.1]))                     # bench.make_problem's prior, over a step of length h


def fenrir_lanes():
    """fenrir on the lane route: fwd_kernel with stored predictions, then fenrir_bwd_kernel (both launches in one profile)."""
    plan = cached_plan(ode, W, x0, 0.0, t_max, N, itg, prior, "standard", store_pred=True, batch_minor=True, theta=theta)
    return fmod._backward_on_grid(plan, None, y, D, Om, 1, obs_index(0.0, t_max, N, on_nodes))


calls = [("fenrir on the lanes", fenrir_lanes),
         # (the solver through its internal entry, which leaves the 0.8 GB of moments on the device)
         ("solve_mv_grid, uniform grid", lambda: ra.grid._run("solve_mv_grid", ra._lib.MODE_MV, None, ode, W, x0, t_uniform, itg, prior_at,
                                                            "standard", dict(theta=theta)).sync())]
if not opt.yardstick:
    behind = np.minimum(on_nodes + 0.37 * dt, t_max - 0.63 * dt)       # (the last one: behind node N - 1)
    t_more, _ = ra.grid_with_times(t_uniform, behind)
    for name, t, times in ((f"(i) uniform grid, observations on nodes: {len(ra.grid_slots(t_uniform)[0])} slot(s)", t_uniform, on_nodes),
                           (f"(ii) grid_with_times, {len(t_more)} nodes: {len(ra.grid_slots(t_more)[0])} slot(s)", t_more, behind)):
        calls.append((f"fenrir_grid, {name}", lambda t=t, times=times: fmod.fenrir_grid(
            None, ode, W, x0, t, itg, prior_at, y, times, D, Om, theta=theta)))
        calls.append((f"fenrir.solve_mv_grid, {name}", lambda t=t, times=times: fmod._solve_grid(
            None, ode, W, x0, t, itg, prior_at, y, times, D, Om, "standard", dict(theta=theta)).sync()))

lines = ["# " + (opt.label or os.path.abspath(opt.root))]
for name, call in calls:
    for rep in range(6):
        dev.sync()
        dev.profile_enable(True)
        t0 = time.perf_counter()
        call()
        dev.sync()
        wall = 1e3 * (time.perf_counter() - t0)
        times = {k: round(v, 4) for k, v in dev.profile_last()}
        dev.profile_enable(False)
        line = "%s%s: kernels %s sum %.4f wall %.2f" % (name, " (warm-up)" if rep == 0 else "", times, sum(times.values()), wall)
        print(line, flush=True)
        lines.append(line)
os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
new = not os.path.exists(opt.out)
with open(opt.out, "a") as f:
    f.write((HEADER if new else "") + "\n".join(lines) + "\n")
