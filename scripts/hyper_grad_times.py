"""Kernel times of dalton_grid_jvp and fenrir_grid_jvp with and without the "log_sigma" / "log_obs_var" directions (DESIGN.md section 7
(25)) on the headline shape of scripts/dalton_grad_times.py / fenrir_grad_times.py (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3,
kramer, 41 observations on nodes 0, 100, .., 4000; the uniform grid):

  K = 5   theta's three directions and the two initial values, without hyper directions: the kernels of (21) / (23), the yardstick
  K = 9   the same five, then the two unit log_sigma and the two unit log_obs_var directions: the hyper kernels
  value   one dalton_grid / fenrir_grid call; a central difference of the four hyper directions takes eight

Kernels are timed by the library's profile (HIP events around each launch); the first call of each kind is discarded, five repeats
follow, medians are reported.  At K = 9 Fenrir's tangent records (7.1 GB) exceed the 4 GiB budget of ``_GRAD_WORKSPACE_BYTES`` and
would run in two chunks, of which the profile keeps the last; the budget is raised to 16 GiB here so that both K run as one call.
Not a pass/fail number.  Appends its lines, under a header, to profiles/hyper_grad_times.txt or to the file named.

    python scripts/hyper_grad_times.py [output file]
"""
import os, sys
import numpy as np
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401
import rodeo_amd.inference.fenrir  # noqa: F401
import bench
dmod, fmod = sys.modules["rodeo_amd.inference.dalton"], sys.modules["rodeo_amd.inference.fenrir"]
fmod._GRAD_WORKSPACE_BYTES = 2 ** 34                                # K = 9 in one chunk (see above)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "profiles", "hyper_grad_times.txt")
HEADER = """# scripts/hyper_grad_times.py on one MI355X: the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer, uniform
# grid), 41 observations on nodes 0, 100, .., 4000; kernel ms (HIP events around each launch, profile_last), summed over the
# launches of one call.  The first call of each kind is the warm-up, five repeats follow.  K = 5: theta's three directions and
# the two initial values (the kernels of the calls without hyper directions); K = 9: those and the unit log_sigma and
# log_obs_var directions (the hyper kernels; Fenrir's 7.1 GB of tangent records in one chunk).  "central difference": 2 x 4 = 8
# value calls for the four hyper directions.
"""
W, x0, theta, prior = bench.make_problem(ra, 0)
N, t_max = bench.N_STEPS, bench.T_MAX
d, p = W.shape[-3], W.shape[-1]
dev = ra.device.default_device()
itg = ra.interrogate.interrogate_kramer
nodes = np.arange(0, N + 1, 100)
rng = np.random.default_rng(0)
y = rng.standard_normal((len(nodes), d, 1)) * 0.3 - 0.5
D = np.zeros((len(nodes), d, 1, p))
D[..., 0, 0] = 1.0
Om = np.full((len(nodes), d, 1, 1), 0.05 ** 2)
t = np.linspace(0.0, t_max, N + 1)


def prior_at(h):
    return ra.ibm_init(h, p, np.array([0.1, 0.1]))                     # bench.make_problem's prior, over a step of length h


def directions(K):
    dth, dx = np.zeros((K, 3)), np.zeros((K, d, p))
    dth[:3] = np.eye(3)
    dx[3, 0, 0] = dx[4, 1, 0] = 1.0
    tangents = dict(theta=dth, ode_init=dx)
    if K == 9:
        tangents["log_sigma"] = np.concatenate([np.zeros((5, d)), np.eye(d), np.zeros((2, d))])
        tangents["log_obs_var"] = np.concatenate([np.zeros((7, d)), np.eye(d)])
    return tangents


lines = ["# B = %d, N = %d, %d observations" % (np.shape(theta)[0], N, len(nodes))]
args = (None, ra.ode.fitzhugh_nagumo, W, x0, t, itg, prior_at, y, t[nodes], D, Om)
for family, value, jvp in (("dalton", dmod.dalton_grid, dmod.dalton_grid_jvp), ("fenrir", fmod.fenrir_grid, fmod.fenrir_grid_jvp)):
    med = {}
    for kind, call in (("value", lambda: value(*args, theta=theta)), ("K = 5", lambda: jvp(*args, directions(5), theta=theta)),
                       ("K = 9 with hyper directions", lambda: jvp(*args, directions(9), theta=theta))):
        totals = []
        for rep in range(6):
            dev.sync()
            dev.profile_enable(True)
            call()
            times = [(k, round(v, 4)) for k, v in dev.profile_last()]
            dev.profile_enable(False)
            total = sum(v for _, v in times)
            if rep:
                totals.append(total)
            line = "%s_grid%s, %s%s: kernels %s sum %.4f" % (family, "" if kind == "value" else "_jvp", kind, " (warm-up)" if rep == 0 else "",
                                                          times, total)
            print(line, flush=True)
            lines.append(line)
        med[kind] = float(np.median(totals))
    v, k5, k9 = med["value"], med["K = 5"], med["K = 9 with hyper directions"]
    line = ("%s: K = 5 without hyper directions %.4f ms (%.4f ms a direction); K = 9 with them %.4f ms (%.4f ms a direction): the four "
            "hyper directions cost %.4f ms more; a central difference of the four, 8 value calls of %.4f ms: %.4f ms; ratio %.2f" % (
                family, k5, k5 / 5, k9, k9 / 9, k9 - k5, v, 8 * v, 8 * v / (k9 - k5)))
    print(line, flush=True)
    lines.append(line)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
new = not os.path.exists(out)
with open(out, "a") as f:
    f.write((HEADER if new else "") + "\n".join(lines) + "\n")
