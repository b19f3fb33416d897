"""Times of daltonng_grid and solve_mv_nn_grid on the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer, Poisson
counts at the 41 times 0, 1, .. 40) on scripts/grid_times.py's three grids -- uniform (1 slot), h and h / 2 alternating in runs of
100 (2 slots, 3 with the times put in), 4000 distinct steps -- each with the 41 observation times put in by grid_with_times, next to daltonng / solve_mv_nn
on the uniform grid.  In one process, after one warm-up call of each kind (it includes the hiprtc builds), the kinds are run in
turn for ROUNDS rounds; kernel times are HIP events around each launch (LaunchTimer, profile_last) per kernel name, wall times host
clocks around the whole call with profiling off.  prior_at is memoised, as a caller with 4000 distinct steps would do.  Not a
pass/fail number.  Appends its lines, under a header, to profiles/daltonng_grid_times.txt or to the file named.

    python scripts/daltonng_grid_times.py [--root DIR] [--yardstick] [--label TEXT] [output file]

--yardstick times daltonng / solve_mv_nn only; with --root DIR the package and bench.py are taken from another checkout (the parent
commit's, built), which is how the two are alternated in fresh processes.
"""
import argparse, functools, os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
ap.add_argument("--yardstick", action="store_true")
ap.add_argument("--label", default="")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("out", nargs="?", default=os.path.join(HERE, "profiles", "daltonng_grid_times.txt"))
opt = ap.parse_args()
sys.path.insert(0, os.path.abspath(opt.root))
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401
from rodeo_amd.trace import gammaln
import bench
dmod = sys.modules["rodeo_amd.inference.dalton"]
ROUNDS = opt.rounds
HEADER = """# scripts/daltonng_grid_times.py on one MI355X: the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer), Poisson
# counts at 41 observation times, ms.  One warm-up of each kind, then five rounds of all kinds in turn.  wall: the whole call with its
# download, profiling off; kernels: HIP events around each launch, per kernel name.  Every block of lines is one fresh process,
# this tree's and the parent commit's daltonng / solve_mv_nn alternating.
"""
W, x0, theta, prior = bench.make_problem(ra, 0)
N, t_max = bench.N_STEPS, bench.T_MAX
p = W.shape[-1]
dev = ra.device.default_device()
itg = ra.interrogate.interrogate_kramer
ode = ra.ode.fitzhugh_nagumo
times = np.linspace(0.0, 40.0, 41)
y = np.random.default_rng(0).poisson(2.0, size=(41, 2, 1)).astype(np.float64)


def poisson_loglik(obs_data_i, ode_data_i, ind, **params):
    eta = 0.1 + 0.5 * ode_data_i[:, 0]
    yy = obs_data_i.flatten()
    return np.sum(yy * eta - np.exp(eta) - gammaln(yy + 1.0))


@functools.lru_cache(maxsize=None)
def prior_at(h):
    return ra.ibm_init(h, p, np.array([0.1, 0.1]))                     # bench.make_problem's prior, over a step of length h


def grids():
    w2 = np.where((np.arange(N) // 100) % 2 == 0, 1.0, 0.5)
    w3 = 2.0 ** np.random.default_rng(3).uniform(-1.5, 1.5, N)
    yield "uniform", np.linspace(0.0, t_max, N + 1)
    for name, w in (("h, h/2 in runs of 100", w2), ("4000 distinct steps", w3)):
        t = np.concatenate([[0.0], np.cumsum(w * (t_max / w.sum()))])
        t[-1] = t_max                                                  # (the sum ends a few ulp short: the last time is node N)
        yield name, t


kinds = []
if not opt.yardstick:
    for name, t0 in grids():
        t, _ = ra.grid_with_times(t0, times)
        label = f"{name}: {len(t) - 1} steps, {len(ra.grid_slots(t)[0])} slot(s)"
        g = (None, ode, W, x0, t, itg, prior_at, y, times, poisson_loglik)
        kinds.append((f"new daltonng_grid, {label}", functools.partial(dmod.daltonng_grid, *g, theta=theta)))
        kinds.append((f"new solve_mv_nn_grid, {label}", functools.partial(dmod.solve_mv_nn_grid, *g, theta=theta)))
u = (None, ode, W, x0, 0.0, t_max, N, itg, prior, y, times, poisson_loglik)
kinds.append(("daltonng, uniform", functools.partial(dmod.daltonng, *u, theta=theta)))
kinds.append(("solve_mv_nn, uniform", functools.partial(dmod.solve_mv_nn, *u, theta=theta)))

lines = ["# " + (opt.label or os.path.abspath(opt.root))]
walls, kern = {k: [] for k, _ in kinds}, {k: [] for k, _ in kinds}
for rnd in range(ROUNDS + 1):
    for name, call in kinds:
        dev.profile_enable(False)
        dev.sync(); t0 = time.perf_counter()
        call()
        dev.sync(); t1 = time.perf_counter()
        dev.profile_enable(True)
        call()
        ks = {k: round(v, 3) for k, v in dev.profile_last()}
        dev.profile_enable(False)
        line = "%s%s: wall ms %.2f kernels %s (sum %.3f)" % (name, " (warm-up)" if rnd == 0 else "", (t1 - t0) * 1e3, ks, sum(ks.values()))
        print(line, flush=True)
        lines.append(line)
        if rnd:
            walls[name].append((t1 - t0) * 1e3)
            kern[name].append(ks)
for name, _ in kinds:
    w, ks = walls[name], kern[name]
    per = {k: (min(d[k] for d in ks), max(d[k] for d in ks)) for k in ks[0]}
    lines.append("%s: wall ms min %.2f median %.2f max %.2f; kernel ms min .. max over %d rounds: %s"
                 % (name, min(w), float(np.median(w)), max(w), ROUNDS, ", ".join("%s %.3f .. %.3f" % (k, a, b) for k, (a, b) in per.items())))
    print(lines[-1], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
fresh = not os.path.exists(opt.out)
with open(opt.out, "a") as f:
    f.write((HEADER if fresh else "") + "\n".join(lines) + "\n")
