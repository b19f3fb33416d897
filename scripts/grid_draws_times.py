"""Times of solve_sim_draws_grid and dalton.solve_sim_draws_grid on the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2,
p = 3, kramer) on scripts/grid_times.py's three grids -- uniform (1 slot), h and h / 2 alternating in runs of 100 (2 slots), 4000
distinct steps -- each with the 41 observation times 0, 1, .. 40 put in by grid_with_times: 16 draws kept at those 41 nodes,
against the same 16 paths taken one sampler call at a time.  In one process, after one warm-up call of each kind, the kinds are
run in turn for ROUNDS rounds:

  new        solve_sim_draws_grid(key, .., n_draws=16, keep=nodes) and dalton.solve_sim_draws_grid likewise, per grid;
  (a)        the yardstick: 16 x (solve_sim_grid(key + s), its download, the host gather [nodes]), per grid; DALTON likewise with
             16 x dalton.solve_sim_grid;
  (b)        solve_sim_draws on the uniform grid (bwd_sim_draws_kernel, one loop-invariant pair).

Wall times are host clocks around calls that end in a download (profiling off); kernel times are HIP events around each launch
(LaunchTimer, profile_last), summed per kernel name, in a second pass of the same kind that leaves the paths on the device.
prior_at is memoised, as a caller with 4000 distinct steps would do.  Not a pass/fail number.  Appends its lines, under a
header, to profiles/grid_draws_times.txt or to the file named.

    python scripts/grid_draws_times.py [--root DIR] [--yardstick] [--label TEXT] [output file]

--yardstick times (a) and (b) only; with --root DIR the package and bench.py are taken from another checkout (the parent
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
ap.add_argument("out", nargs="?", default=os.path.join(HERE, "profiles", "grid_draws_times.txt"))
opt = ap.parse_args()
sys.path.insert(0, os.path.abspath(opt.root))
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401
import bench
dmod = sys.modules["rodeo_amd.inference.dalton"]
ROUNDS, N_DRAWS, KEY = opt.rounds, 16, 5
HEADER = """# scripts/grid_draws_times.py on one MI355X: the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer), 16 draws
# kept at the 41 observation nodes, ms.  new: solve_sim_draws_grid / dalton.solve_sim_draws_grid; (a) 16 x (solve_sim_grid /
# dalton.solve_sim_grid + download + gather); (b) solve_sim_draws on the uniform grid.  One warm-up of each kind, then five rounds
# of all kinds in turn.  wall: the whole call with its downloads, profiling off; kernels: HIP events around each launch, summed per
# kernel name, in a second pass that leaves the paths on the device.  Every block of lines is one fresh process, this tree's and
# the parent commit's yardsticks alternating.
"""
W, x0, theta, prior = bench.make_problem(ra, 0)
N, t_max = bench.N_STEPS, bench.T_MAX
p = W.shape[-1]
dev = ra.device.default_device()
itg = ra.interrogate.interrogate_kramer
ode = ra.ode.fitzhugh_nagumo
times = np.linspace(0.0, 40.0, 41)
y = np.random.default_rng(0).standard_normal((41, 2, 1)) * 0.3
D = np.zeros((41, 2, 1, p))
D[..., 0, 0] = 1.0
Om = np.full((41, 2, 1, 1), 0.05 ** 2)
obs = (y, times, D, Om)
MODE_SIM = ra._lib.MODE_SIM


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


def one_at_a_time(sample, nodes):
    out = np.empty((bench.N_TRAJ, N_DRAWS, nodes.size, bench.D, bench.P))
    for s in range(N_DRAWS):
        out[:, s] = sample(KEY + s)[:, nodes]
    return out


def on_device(launch):
    """16 sampler launches that leave their paths on the device: the kernel pass of a yardstick"""
    for s in range(N_DRAWS):
        launch(KEY + s)
    dev.sync()


# kind -> (the call that is timed on the wall, the call whose kernels are timed); a kind named "new ..." needs this tree
kinds, pairs = [], {}
for name, t0 in grids():
    t, nodes = ra.grid_with_times(t0, times)
    nodes = np.asarray(nodes, dtype=np.int64)
    label = f"{name}: {len(t) - 1} steps, {len(ra.grid_slots(t)[0])} slot(s)"
    g = (ode, W, x0, t, itg, prior_at)
    kw = dict(theta=theta)
    if not opt.yardstick:
        new = functools.partial(ra.solve_sim_draws_grid, KEY, *g, n_draws=N_DRAWS, keep=nodes, **kw)
        dnew = functools.partial(dmod.solve_sim_draws_grid, KEY, *g, *obs, n_draws=N_DRAWS, keep=nodes, **kw)
        kinds += [(f"new solve_sim_draws_grid, {label}", new, new), (f"new dalton.solve_sim_draws_grid, {label}", dnew, dnew)]
        pairs[f"new solve_sim_draws_grid, {label}"] = f"(a) 16 x solve_sim_grid, {label}"
        pairs[f"new dalton.solve_sim_draws_grid, {label}"] = f"(a) 16 x dalton.solve_sim_grid, {label}"
    kinds.append((f"(a) 16 x solve_sim_grid, {label}",
                  lambda g=g, nodes=nodes: one_at_a_time(lambda key: ra.solve_sim_grid(key, *g, **kw), nodes),
                  lambda g=g: on_device(lambda key: ra.grid._run("solve_sim_grid", MODE_SIM, key, *g, "standard", kw))))
    kinds.append((f"(a) 16 x dalton.solve_sim_grid, {label}",
                  lambda g=g, nodes=nodes: one_at_a_time(lambda key: dmod.solve_sim_grid(key, *g, *obs, **kw), nodes),
                  lambda g=g: on_device(lambda key: dmod._solve_grid("dalton.solve_sim_grid", MODE_SIM, key, *g, *obs, "standard", kw))))
uniform_nodes = np.round(times / (t_max / N)).astype(np.int64)
b_draws = functools.partial(ra.solve_sim_draws, KEY, ode, W, x0, 0.0, t_max, N, itg, prior, n_draws=N_DRAWS, keep=uniform_nodes,
                            theta=theta)
kinds.append(("(b) solve_sim_draws, uniform", b_draws, b_draws))


def kernel_sums():
    sums = {}
    for k, v in dev.profile_last(cap=256):
        sums[k] = sums.get(k, 0.0) + v
    return {k: round(v, 3) for k, v in sums.items()}


lines, results = ["# " + (opt.label or os.path.abspath(opt.root))], {}
walls, kern = {k: [] for k, _, _ in kinds}, {k: [] for k, _, _ in kinds}
for rnd in range(ROUNDS + 1):
    for name, call, kernels in kinds:
        dev.profile_enable(False)
        dev.sync(); t0 = time.perf_counter()
        results[name] = call()
        dev.sync(); t1 = time.perf_counter()
        dev.profile_enable(True, keep=True)
        kernels()
        ks = kernel_sums()
        dev.profile_enable(False)
        line = "%s%s: wall ms %.2f kernels %s (sum %.3f)" % (name, " (warm-up)" if rnd == 0 else "", (t1 - t0) * 1e3, ks, sum(ks.values()))
        print(line, flush=True)
        lines.append(line)
        if rnd:
            walls[name].append((t1 - t0) * 1e3)
            kern[name].append(sum(ks.values()))
for name, _, _ in kinds:
    w, k = walls[name], kern[name]
    lines.append("%s: wall ms min %.2f median %.2f max %.2f; kernel ms min %.3f median %.3f max %.3f over %d rounds"
                 % (name, min(w), float(np.median(w)), max(w), min(k), float(np.median(k)), max(k), ROUNDS))
    print(lines[-1], flush=True)
for name, ref in pairs.items():
    got, want = results[name], results[ref]
    lines.append("%s against (a): largest difference %.3e of max|x|, identical bits %s; wall %.1f-fold, kernels %.1f-fold"
                 % (name, float(np.max(np.abs(got - want)) / np.max(np.abs(want))), np.array_equal(got, want),
                    np.median(walls[ref]) / np.median(walls[name]), np.median(kern[ref]) / np.median(kern[name])))
    print(lines[-1], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
fresh = not os.path.exists(opt.out)
with open(opt.out, "a") as f:
    f.write((HEADER if fresh else "") + "\n".join(lines) + "\n")
