"""Kernel times of fenrir_grid_jvp on the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer, 41 observations
on nodes 0, 100, .., 4000, K = 5 directions: the three of theta and the two initial values) on grid_times.py's three grids --
uniform (1 slot), h and h / 2 alternating in runs of 100 (2 slots), 4000 distinct steps -- next to what a central difference of
fenrir_grid costs for the same five derivatives: 2 K = 10 fenrir_grid calls.  The tangent records of the call take 3.9 GB.  Kernels are timed by the library's profile (HIP
events around each launch); the first call of each kind is discarded, five repeats follow.  Not a pass/fail number.  Appends its
lines, under a header, to profiles/fenrir_grad_times.txt or to the file named.

    python scripts/fenrir_grad_times.py [output file]
"""
import os, sys
import numpy as np
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import rodeo_amd as ra
import rodeo_amd.inference.fenrir  # noqa: F401
import bench
fmod = sys.modules["rodeo_amd.inference.fenrir"]
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "profiles", "fenrir_grad_times.txt")
HEADER = """# scripts/fenrir_grad_times.py on one MI355X: the headline shape (FitzHugh-Nagumo, B = 1024, N = 4000, d = 2, p = 3, kramer), 41
# observations on nodes 0, 100, .., 4000, K = 5 directions (theta's three, the two initial values); kernel ms (HIP events around
# each launch, profile_last).  The first call of each kind is the warm-up, five repeats follow.  "central difference": 2 K = 10
# fenrir_grid calls, the kernel time of one call times ten.
"""
W, x0, theta, prior = bench.make_problem(ra, 0)
N, t_max, K = bench.N_STEPS, bench.T_MAX, 5
d, p = W.shape[-3], W.shape[-1]
dev = ra.device.default_device()
itg = ra.interrogate.interrogate_kramer
nodes = np.arange(0, N + 1, 100)
rng = np.random.default_rng(0)
y = rng.standard_normal((len(nodes), d, 1)) * 0.3 - 0.5
D = np.zeros((len(nodes), d, 1, p))
D[..., 0, 0] = 1.0
Om = np.full((len(nodes), d, 1, 1), 0.05 ** 2)
dth = np.concatenate([np.eye(3), np.zeros((2, 3))])
dx = np.zeros((K, d, p))
dx[3, 0, 0] = dx[4, 1, 0] = 1.0


def prior_at(h):
    return ra.ibm_init(h, p, np.array([0.1, 0.1]))                     # bench.make_problem's prior, over a step of length h


def grids():
    w2 = np.where((np.arange(N) // 100) % 2 == 0, 1.0, 0.5)
    w3 = 2.0 ** np.random.default_rng(3).uniform(-1.5, 1.5, N)
    yield "uniform (1 slot)", np.linspace(0.0, t_max, N + 1)
    yield "h, h/2 in runs of 100 (2 slots)", np.concatenate([[0.0], np.cumsum(w2 * (t_max / w2.sum()))])
    yield "4000 distinct steps", np.concatenate([[0.0], np.cumsum(w3 * (t_max / w3.sum()))])


lines = ["# B = %d, N = %d, K = %d, %d observations" % (np.shape(theta)[0], N, K, len(nodes))]
for name, t in grids():
    args = (None, ra.ode.fitzhugh_nagumo, W, x0, t, itg, prior_at, y, t[nodes], D, Om)
    sums = {}
    for kind, call in (("fenrir_grid", lambda: fmod.fenrir_grid(*args, theta=theta)),
                       ("fenrir_grid_jvp", lambda: fmod.fenrir_grid_jvp(*args, dict(theta=dth, ode_init=dx), theta=theta))):
        for rep in range(6):
            dev.sync()
            dev.profile_enable(True)
            call()
            times = [(k, round(v, 4)) for k, v in dev.profile_last()]     # (a list: fenrir_grid_jvp's two block sums share a name)
            dev.profile_enable(False)
            total = sum(v for _, v in times)
            if rep:
                sums.setdefault(kind, []).append(total)
            line = "%s, %s%s: kernels %s sum %.4f" % (kind, name, " (warm-up)" if rep == 0 else "", times, total)
            print(line, flush=True)
            lines.append(line)
    one, jvp = float(np.median(sums["fenrir_grid"])), float(np.median(sums["fenrir_grid_jvp"]))
    line = "%s: one fenrir_grid_jvp call (K = %d) %.4f ms; central difference, 2 K = %d fenrir_grid calls of %.4f ms: %.4f ms; ratio %.2f" % (
        name, K, jvp, 2 * K, one, 2 * K * one, 2 * K * one / jvp)
    print(line, flush=True)
    lines.append(line)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
new = not os.path.exists(out)
with open(out, "a") as f:
    f.write((HEADER if new else "") + "\n".join(lines) + "\n")
