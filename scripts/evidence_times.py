"""Times of solve_evidence on the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer), end to end and
per kernel, next to its yardstick from the same build -- dalton's log-likelihood kernel dalton_fwd_tile3_kernel<loglik> with
41 observations per variable, which runs twice as many filter instances (see HEADER below) -- and to fwd_tile3_kernel in filter
mode.  The tile route five times after a warm-up call; the lane and the square-root routes once each after theirs (functional,
untuned).  Run it on this build and on the parent commit (there the solve_evidence part is skipped): dalton's and the filter's
kernels are unchanged, so their figures should agree.  Writes its lines, under a header, to profiles/evidence_times.txt or to
the file named (profiles/evidence_times_parent.txt is the parent commit's run); a rerun replaces the file.

    python scripts/evidence_times.py [label] [output file]
"""
import sys, os, time, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rodeo_amd as ra
import bench
import rodeo_amd.inference.dalton  # noqa: F401
dalton_mod = sys.modules["rodeo_amd.inference.dalton"]
label = sys.argv[1] if len(sys.argv) > 1 else "this build"
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "evidence_times.txt")
HEADER = """# scripts/evidence_times.py on one MI355X: the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer), ms.
# The first call of each kind is the warm-up.  Yardstick: dalton_fwd_tile3_kernel<loglik> with 41 observations (2 B filter
# instances).  NB on this shape every forecast variance lies in 3.3e-9 .. 6.8e-9, below the 1e-8 threshold of utils.py:60-78, so
# the yardstick kernel skips its density block (a division and a log) at every step; solve_evidence has no threshold and
# evaluates the density at every step (DESIGN.md section 7 (12)).
"""
W, x0, theta, prior = bench.make_problem(ra, 0)
n_obs, N, t_max = 41, 4000, 40.0
obs_t = np.linspace(0, t_max, n_obs)
rng = np.random.default_rng(0)
Y = rng.standard_normal((n_obs, 2, 1))
Dw = np.zeros((n_obs, 2, 1, 3)); Dw[..., 0] = 1.0
Om = np.full((n_obs, 2, 1, 1), 0.005)
dev = ra.device.default_device()
args = (ra.ode.fitzhugh_nagumo, W, x0, 0.0, t_max, N, ra.interrogate.interrogate_kramer, prior)
plan = ra.SolvePlan(*args, theta=theta)


def run_filter():
    plan.filter(None)
    return np.zeros(2)


def evidence(lanes=False, form="standard"):
    def call():
        os.environ["RK_EVIDENCE_LANES"] = "1" if lanes else "0"
        pp = prior if form == "standard" else (prior[0], np.linalg.cholesky(prior[1]))
        return ra.solve_evidence(None, *args[:-1], pp, kalman_type=form, theta=theta).logdens
    return call


calls = [("dalton (41 observations)", lambda: dalton_mod.dalton(None, *args, Y, obs_t, Dw, Om, theta=theta), 6),
         ("filter()", run_filter, 6)]
if hasattr(ra, "solve_evidence"):
    calls += [("solve_evidence (tiles)", evidence(), 6), ("solve_evidence (lanes)", evidence(lanes=True), 2),
              ("solve_evidence (square-root lanes)", evidence(form="square-root"), 2)]
lines = []
for name, call, reps in calls:
    for rep in range(reps):
        dev.sync(); t0 = time.perf_counter()
        dev.profile_enable(True)
        out = call()
        dev.sync(); t1 = time.perf_counter()
        line = "%s | %s%s: wall ms %.2f kernels %s head %s" % (label, name, " (warm-up)" if rep == 0 else "", (t1 - t0) * 1e3,
                                                                {k: round(v, 4) for k, v in dev.profile_last()}, out[:2])
        print(line, flush=True)
        lines.append(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(HEADER + "\n".join(lines) + "\n")
