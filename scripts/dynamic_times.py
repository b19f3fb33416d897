"""Times of solve_mv_dynamic on the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer), per kernel and
end to end (the call with its download of mean, var and scale), next to solve_mv forced onto the same lane route
(SolvePlan(batch_minor=True): fwd_kernel + bwd_mv_kernel) and solve_mv on its default route (the p = 3 MFMA tiles), each with
its download.  First call of each kind discarded, five repeats.  Not a pass/fail number: the figures by which a tile route for
the dynamic scale can be judged later.  Writes its lines, under a header, to profiles/dynamic_times.txt or to the file named; a
rerun replaces the file.

    python scripts/dynamic_times.py [output file]
"""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rodeo_amd as ra
import bench
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dynamic_times.txt")
HEADER = """# scripts/dynamic_times.py on one MI355X: the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer), ms.
# The first call of each kind is the warm-up.  wall: the whole call, the download of its results included (mean and var, 0.79 GB;
# solve_mv_dynamic adds scale, 66 MB); kernels: HIP events around each launch (profile_last).
"""
W, x0, theta, prior = bench.make_problem(ra, 0)
N, t_max = bench.N_STEPS, bench.T_MAX
dev = ra.device.default_device()
args = (ra.ode.fitzhugh_nagumo, W, x0, 0.0, t_max, N, ra.interrogate.interrogate_kramer, prior)
lane_plan = ra.SolvePlan(*args, batch_minor=True, theta=theta)


def dynamic():
    return ra.solve_mv_dynamic(None, *args, theta=theta).mean


def lanes():
    lane_plan.mv(None)
    return lane_plan.state_host()[0]


def default():
    return ra.solve_mv(None, *args, theta=theta)[0]


lines = []
for name, call in (("solve_mv_dynamic", dynamic), ("solve_mv on the lane route (batch_minor)", lanes), ("solve_mv on its default route", default)):
    for rep in range(6):
        dev.sync(); t0 = time.perf_counter()
        dev.profile_enable(True)
        out = call()
        dev.sync(); t1 = time.perf_counter()
        line = "%s%s: wall ms %.2f kernels %s mean at t_max %s" % (name, " (warm-up)" if rep == 0 else "", (t1 - t0) * 1e3,
                                                                   {k: round(v, 4) for k, v in dev.profile_last()}, out[0, -1, :, 0])
        print(line, flush=True)
        lines.append(line)
dev.profile_enable(False)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(HEADER + "\n".join(lines) + "\n")
