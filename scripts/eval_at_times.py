#!/usr/bin/env python3
"""
Times ``solve_mv_at`` at the headline shape (bench.py's problem: FitzHugh-Nagumo, B = 1024, N = 4000, p = 3) for T = 41
observation times, end to end (host clock around the call, which ends in the download) with its kernels split out
(rk_profile_enable), against ``solve_mv`` followed by a host gather of the same 41 grid points -- the only way to get them
without ``solve_mv_at``, and code that ``solve_mv_at`` does not touch.  The times are off the grid for ``solve_mv_at`` (the
general case: two predicts and a gain per query) and snapped to it for the gather.

    python scripts/eval_at_times.py [--reps 7] [--out profiles/eval_at_times.txt]      (needs an MI355X)
"""
import argparse
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                       # noqa: E402
import rodeo_amd as ra                                             # noqa: E402
from rodeo_amd.interrogate import interrogate_kramer              # noqa: E402

T = 41


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_at_times.txt"))
    a = ap.parse_args()
    W, x0, theta, prior = bench.make_problem(ra, 0)
    N, t_max, p = bench.N_STEPS, bench.T_MAX, bench.P
    dt = t_max / N
    t_off = (np.arange(T) * (N // (T - 1)) + 0.37) * dt
    t_off[-1] = t_max - 0.37 * dt
    nodes = np.minimum(np.arange(T) * (N // (T - 1)), N)

    def prior_at(h):
        return ra.ibm_init(h, p, np.array([0.1, 0.1]))
    args = (None, ra.ode.fitzhugh_nagumo, W, x0, 0.0, t_max, N, interrogate_kramer, prior)
    dev = ra.default_device()

    def at():
        return ra.solve_mv_at(*args, t_off, prior_at, theta=theta)

    def gather():
        m, v = ra.solve_mv(*args, theta=theta)
        return np.ascontiguousarray(m[:, nodes]), np.ascontiguousarray(v[:, nodes])
    wall = {"solve_mv_at": [], "solve_mv + host gather": []}
    for fn in (at, gather):
        fn()                                                       # warm-up: code objects, first allocations
    for _ in range(a.reps):                                        # alternate the two, as they share the machine
        for name, fn in (("solve_mv_at", at), ("solve_mv + host gather", gather)):
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    kern = {}
    for name, fn in (("solve_mv_at", at), ("solve_mv + host gather", gather)):
        dev.profile_enable(True, keep=True)
        fn()
        kern[name] = dev.profile_last(64)
        dev.profile_enable(False)
    lines = [f"# scripts/eval_at_times.py on {dev.name()}",
             f"# FitzHugh-Nagumo, B = {bench.N_TRAJ}, N = {N}, p = {p}, T = {T}; {a.reps} alternating repetitions after one warm-up",
             f"# downloaded: solve_mv_at {(bench.N_TRAJ * T * 2 * (p + p * p) * 8) / 1e6:.2f} MB, "
             f"solve_mv {(bench.N_TRAJ * (N + 1) * 2 * 12 * 8) / 1e6:.0f} MB"]
    for name, ms in wall.items():
        ms = np.array(ms)
        lines.append(f"{name:24s} end to end: median {np.median(ms):8.2f} ms   min {ms.min():8.2f}   max {ms.max():8.2f}")
        lines.append(f"{'':24s} kernels: " + ", ".join(f"{k} {t:.3f} ms" for k, t in kern[name]) +
                     f"   (sum {sum(t for _, t in kern[name]):.3f} ms)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
