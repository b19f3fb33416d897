"""Times of solve_sim_draws on the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer): 16 draws kept at
the 41 observation nodes of scripts/dalton_times.py, against the same 16 paths taken one solve_sim at a time.  In one process,
after one warm-up call of each kind, the three are run in turn for ROUNDS rounds:

  (a) solve_sim_draws(key, .., n_draws=16, keep=nodes), end to end (the download included) and its two kernels;
  (b) the yardstick: 16 x (plan.sim(key + s), x_host()) and the host gather [nodes] on the same batch-minor plan (fwd_kernel +
      bwd_sim_kernel on the lanes);
  (c) the same on the default route (the p = 3 MFMA tiles).

Wall times are host clocks around calls that end in a download (profiling off); kernel times are HIP events around each launch
(profile_last) in a second call of the same kind.  Then the backward kernel alone with 1, 2 and 4 draws per lane
(RK_SIM_DRAWS_CHUNK) and with the launch's own choice, at 16 and at 128 draws: the per-draw cost, and where sharing the gain
work starts to pay.  The result of (a) is compared with (b)'s.  Writes
its lines, under a header, to profiles/sim_draws_times.txt or to the file named; a rerun replaces the file.

    python scripts/sim_draws_times.py [output file]
"""
import sys, os, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rodeo_amd as ra
from rodeo_amd import draws
import bench
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sim_draws_times.txt")
ROUNDS, N_DRAWS, KEY = 5, 16, 5
HEADER = """# scripts/sim_draws_times.py on one MI355X: the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer), 16 draws
# kept at 41 nodes, ms.  (a) solve_sim_draws; (b) 16 x plan.sim + x_host + gather on the lane route; (c) the same on the default
# (tile) route.  One warm-up call of each kind, then the three in turn per round.  wall: the whole call with its downloads,
# profiling off; kernels: HIP events around each launch, summed per kernel name, in a second call of the same kind.
"""
W, x0, theta, prior = bench.make_problem(ra, 0)
N, t_max = bench.N_STEPS, bench.T_MAX
nodes = np.round(np.linspace(0, 40, 41) / (t_max / N)).astype(np.int64)
dev = ra.device.default_device()
args = (ra.ode.fitzhugh_nagumo, W, x0, 0.0, t_max, N, ra.interrogate.interrogate_kramer, prior)
lane_plan = ra.SolvePlan(*args, batch_minor=True, theta=theta)
tile_plan = ra.SolvePlan(*args, theta=theta)


def a_draws():
    return ra.solve_sim_draws(KEY, *args, n_draws=N_DRAWS, keep=nodes, theta=theta)


def one_at_a_time(plan):
    out = np.empty((bench.N_TRAJ, N_DRAWS, nodes.size, bench.D, bench.P))
    for s in range(N_DRAWS):
        plan.sim(KEY + s)
        out[:, s] = plan.x_host()[:, nodes]
    return out


KINDS = (("(a) solve_sim_draws", a_draws), ("(b) 16 x sim on the lane route", lambda: one_at_a_time(lane_plan)),
         ("(c) 16 x sim on the default route", lambda: one_at_a_time(tile_plan)))


def kernel_sums():
    sums = {}
    for k, v in dev.profile_last(cap=256):
        sums[k] = sums.get(k, 0.0) + v
    return {k: round(v, 3) for k, v in sums.items()}


lines, results, walls, kern = [], {}, {k: [] for k, _ in KINDS}, {k: [] for k, _ in KINDS}
for rnd in range(ROUNDS + 1):
    for name, call in KINDS:
        dev.profile_enable(False)
        dev.sync(); t0 = time.perf_counter()
        results[name] = call()
        dev.sync(); t1 = time.perf_counter()
        dev.profile_enable(True, keep=True)
        call()
        ks = kernel_sums()
        dev.profile_enable(False)
        line = "%s%s: wall ms %.2f kernels %s (sum %.3f)" % (name, " (warm-up)" if rnd == 0 else "", (t1 - t0) * 1e3, ks, sum(ks.values()))
        print(line, flush=True)
        lines.append(line)
        if rnd:
            walls[name].append((t1 - t0) * 1e3)
            kern[name].append(sum(ks.values()))
for name, _ in KINDS:
    w, k = walls[name], kern[name]
    lines.append("%s: wall ms min %.2f median %.2f max %.2f; kernel ms min %.3f median %.3f max %.3f over %d rounds"
                 % (name, min(w), float(np.median(w)), max(w), min(k), float(np.median(k)), max(k), ROUNDS))
    print(lines[-1], flush=True)
ref = results[KINDS[1][0]]
for name, _ in (KINDS[0], KINDS[2]):
    lines.append("%s against (b): largest difference %.3e of max|x|, identical bits %s"
                 % (name, float(np.max(np.abs(results[name] - ref)) / np.max(np.abs(ref))), np.array_equal(results[name], ref)))
    print(lines[-1], flush=True)

# the backward kernel per draw: 1, 2 and 4 draws per lane and the launch's own choice, in turn, at 16 and at 128 draws
for n_draws in (N_DRAWS, 8 * N_DRAWS):
    per = {"1": [], "2": [], str(draws.chunk()): [], "chosen by the launch": []}
    for rnd in range(ROUNDS + 1):
        for c in per:
            if c.isdigit():
                os.environ["RK_SIM_DRAWS_CHUNK"] = c
            else:
                os.environ.pop("RK_SIM_DRAWS_CHUNK", None)
            dev.profile_enable(True)
            ra.solve_sim_draws(KEY, *args, n_draws=n_draws, keep=nodes, theta=theta)
            ms = dict(dev.profile_last())["bwd_sim_draws_kernel"]
            dev.profile_enable(False)
            if rnd:
                per[c].append(ms)
    os.environ.pop("RK_SIM_DRAWS_CHUNK", None)
    for c, v in per.items():
        lines.append("bwd_sim_draws_kernel, %d draws, draws per lane %s: ms min %.3f median %.3f max %.3f = %.3f ms per draw"
                     % (n_draws, c, min(v), float(np.median(v)), max(v), float(np.median(v)) / n_draws))
        print(lines[-1], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(HEADER + "\n".join(lines) + "\n")
