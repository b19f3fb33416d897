"""Kernel times of solve_mv_grid on the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer) on three grids
-- uniform (1 slot), h and h / 2 alternating in runs of 100 (2 slots), 4000 distinct steps -- next to the yardstick, solve_mv on
the lane route of a batch-minor plan (fwd_kernel + bwd_mv_kernel).  Kernels are timed by the library's profile (HIP events around
each launch); the first call of each kind is discarded, five repeats follow.  Not a pass/fail number.  Appends its lines, under a
header, to profiles/grid_times.txt or to the file named.

    python scripts/grid_times.py [--root DIR] [--yardstick] [--label TEXT] [output file]

--yardstick times the lane route only; with --root DIR the package and bench.py are taken from another checkout (the parent
commit's, built), which is how the two are alternated in fresh processes.
"""
import argparse, os, sys
import numpy as np
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
ap.add_argument("--yardstick", action="store_true")
ap.add_argument("--label", default="")
ap.add_argument("out", nargs="?", default=os.path.join(HERE, "profiles", "grid_times.txt"))
opt = ap.parse_args()
sys.path.insert(0, os.path.abspath(opt.root))
import rodeo_amd as ra
import bench
HEADER = """# scripts/grid_times.py on one MI355X: the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer), kernel ms
# (HIP events around each launch, profile_last).  The first call of each kind is the warm-up, five repeats follow; every block of
# lines is one fresh process, this tree's and the parent commit's lane route alternating.
"""
W, x0, theta, prior = bench.make_problem(ra, 0)
N, t_max = bench.N_STEPS, bench.T_MAX
p = W.shape[-1]
dev = ra.device.default_device()
itg = ra.interrogate.interrogate_kramer
lane_plan = ra.SolvePlan(ra.ode.fitzhugh_nagumo, W, x0, 0.0, t_max, N, itg, prior, batch_minor=True, theta=theta)


def prior_at(h):
    return ra.ibm_init(h, p, np.array([0.1, 0.1]))                     # bench.make_problem's prior, over a step of length h


def grids():
    w2 = np.where((np.arange(N) // 100) % 2 == 0, 1.0, 0.5)
    w3 = 2.0 ** np.random.default_rng(3).uniform(-1.5, 1.5, N)
    yield "uniform (1 slot)", np.linspace(0.0, t_max, N + 1)
    yield "h, h/2 in runs of 100 (2 slots)", np.concatenate([[0.0], np.cumsum(w2 * (t_max / w2.sum()))])
    yield "4000 distinct steps", np.concatenate([[0.0], np.cumsum(w3 * (t_max / w3.sum()))])


def lanes():
    lane_plan.mv(None)
    lane_plan.sync()


calls = [("solve_mv on the lane route (batch_minor)", lanes)]
if not opt.yardstick:
    for name, t in grids():
        n_slots = len(ra.grid_slots(t)[0])

        def call(t=t):
            ra.grid._run("solve_mv_grid", ra._lib.MODE_MV, None, ra.ode.fitzhugh_nagumo, W, x0, t, itg, prior_at, "standard",
                         dict(theta=theta)).sync()
        calls.append((f"solve_mv_grid, {name}: {n_slots} slot(s)", call))

lines = ["# " + (opt.label or os.path.abspath(opt.root))]
for name, call in calls:
    for rep in range(6):
        dev.sync()
        dev.profile_enable(True)
        call()
        times = {k: round(v, 4) for k, v in dev.profile_last()}
        dev.profile_enable(False)
        line = "%s%s: kernels %s sum %.4f" % (name, " (warm-up)" if rep == 0 else "", times, sum(times.values()))
        print(line, flush=True)
        lines.append(line)
os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
new = not os.path.exists(opt.out)
with open(opt.out, "a") as f:
    f.write((HEADER if new else "") + "\n".join(lines) + "\n")
