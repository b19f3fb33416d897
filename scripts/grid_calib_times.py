"""Kernel times of solve_evidence_grid, solve_mv_dynamic_grid and solve_sim_dynamic_grid on the headline shape (FitzHugh-Nagumo,
B = 1024, N = 4000, d = 2, p = 3, kramer) on scripts/grid_times.py's three grids -- uniform (1 slot), h and h / 2 alternating in
runs of 100 (2 slots), 4000 distinct steps -- next to their yardsticks: solve_evidence on the lanes (RK_EVIDENCE_LANES=1,
evidence_kernel), solve_mv_dynamic / solve_sim_dynamic (dynamic_fwd_kernel + dynamic_bwd_*_kernel) and solve_mv_grid /
solve_sim_grid (grid_fwd_kernel + grid_bwd_*_kernel).  Kernels are timed by the library's profile (HIP events around each
launch); the first call of each kind is discarded, five repeats follow.  Not a pass/fail number.  Appends its lines, under a
header, to profiles/grid_calib_times.txt or to the file named.

    python scripts/grid_calib_times.py [--root DIR] [--yardsticks] [--label TEXT] [output file]

--yardsticks times only what the parent commit has; with --root DIR the package and bench.py are taken from another checkout
(the parent commit's, built), which is how the two are alternated in fresh processes.
"""
import argparse, os, sys
import numpy as np
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
ap.add_argument("--yardsticks", action="store_true")
ap.add_argument("--label", default="")
ap.add_argument("out", nargs="?", default=os.path.join(HERE, "profiles", "grid_calib_times.txt"))
opt = ap.parse_args()
os.environ["RK_EVIDENCE_LANES"] = "1"                                # the lanes at n_bstate = 3: evidence_kernel, not the tiles
sys.path.insert(0, os.path.abspath(opt.root))
import rodeo_amd as ra
import bench
HEADER = """# scripts/grid_calib_times.py on one MI355X: the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer), kernel
# ms (HIP events around each launch, profile_last).  The first call of each kind is the warm-up, five repeats follow; every block
# of lines is one fresh process, this tree and the parent commit alternating.
"""
W, x0, theta, prior = bench.make_problem(ra, 0)
N, t_max = bench.N_STEPS, bench.T_MAX
p = W.shape[-1]
dev = ra.device.default_device()
itg = ra.interrogate.interrogate_kramer
fhn = ra.ode.fitzhugh_nagumo


def prior_at(h):
    return ra.ibm_init(h, p, np.array([0.1, 0.1]))                     # bench.make_problem's prior, over a step of length h


def grids():
    w2 = np.where((np.arange(N) // 100) % 2 == 0, 1.0, 0.5)
    w3 = 2.0 ** np.random.default_rng(3).uniform(-1.5, 1.5, N)
    yield "uniform (1 slot)", np.linspace(0.0, t_max, N + 1)
    yield "h, h/2 in runs of 100 (2 slots)", np.concatenate([[0.0], np.cumsum(w2 * (t_max / w2.sum()))])
    yield "4000 distinct steps", np.concatenate([[0.0], np.cumsum(w3 * (t_max / w3.sum()))])


MV, SIM = ra._lib.MODE_MV, ra._lib.MODE_SIM
params = dict(theta=theta)
# (the runners behind the public functions: the moments stay on the device, (N, d, B) scales and (B,) sums come back)
calls = [("solve_evidence on the lanes", lambda: ra.solve_evidence(None, fhn, W, x0, 0.0, t_max, N, itg, prior, theta=theta)),
         ("solve_mv_dynamic", lambda: ra.dynamic._run("solve_mv_dynamic", MV, None, fhn, W, x0, 0.0, t_max, N, itg, prior, "standard", 0.0,
                                                      params)),
         ("solve_sim_dynamic", lambda: ra.dynamic._run("solve_sim_dynamic", SIM, 1, fhn, W, x0, 0.0, t_max, N, itg, prior, "standard", 0.0,
                                                       params))]
for name, t in grids():
    tag = f"{name}: {len(ra.grid_slots(t)[0])} slot(s)"
    calls.append((f"solve_mv_grid, {tag}", lambda t=t: ra.grid._run("solve_mv_grid", MV, None, fhn, W, x0, t, itg, prior_at, "standard", params)))
    calls.append((f"solve_sim_grid, {tag}", lambda t=t: ra.grid._run("solve_sim_grid", SIM, 1, fhn, W, x0, t, itg, prior_at, "standard", params)))
    if not opt.yardsticks:
        calls.append((f"solve_evidence_grid, {tag}", lambda t=t: ra.solve_evidence_grid(None, fhn, W, x0, t, itg, prior_at, theta=theta)))
        calls.append((f"solve_mv_dynamic_grid, {tag}", lambda t=t: ra.grid_calib._run_dynamic(
            "solve_mv_dynamic_grid", MV, None, fhn, W, x0, t, itg, prior_at, "standard", 0.0, params)))
        calls.append((f"solve_sim_dynamic_grid, {tag}", lambda t=t: ra.grid_calib._run_dynamic(
            "solve_sim_dynamic_grid", SIM, 1, fhn, W, x0, t, itg, prior_at, "standard", 0.0, params)))

lines = ["# " + (opt.label or os.path.abspath(opt.root))]
for name, call in calls:
    for rep in range(6):
        dev.sync()
        dev.profile_enable(True)
        call()
        dev.sync()
        times = {k: round(v, 4) for k, v in dev.profile_last()}
        dev.profile_enable(False)
        line = "%s%s: kernels %s sum %.4f" % (name, " (warm-up)" if rep == 0 else "", times, sum(times.values()))
        print(line, flush=True)
        lines.append(line)
os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
new = not os.path.exists(opt.out)
with open(opt.out, "a") as f:
    f.write((HEADER if new else "") + "\n".join(lines) + "\n")
