#!/usr/bin/env python3
"""
Registers, scratch and LDS of daltonng_grid's kernels -> profiles/daltonng_grid_code_objects.txt.
Needs no GPU.

The forward kernel is a hiprtc build: for FitzHugh-Nagumo (n_bstate 2 .. 6) and Lorenz63 (3 .. 5) with the Poisson model of
examples/fitzhugh_daltonng.py and the three interrogations, rk_obs_compile_check builds daltonng_fwd_kernel and
rk_obs_grid_compile_check daltonng_grid_fwd_kernel, both forms each, under RK_JIT_VERBOSE, which prints every build's resources.
THE SHIP RULE: an instance ships if it has no more scratch than daltonng_fwd_kernel of the same form at the same (RHS, P, ITG).
The gain kernel is built ahead of time: its figures come from the library's code objects, next to daltonng_gain_kernel's.

    python3 scripts/daltonng_grid_code_objects.py [--jobs 4]            (one child process per (right-hand side, n_bstate))
"""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
OUT = os.path.join(ROOT, "profiles", "daltonng_grid_code_objects.txt")
ITG = ("rodeo", "schober", "kramer")
LINE = re.compile(r"\[rk\] jit build (\S+): (-?\d+) VGPRs \+ (-?\d+) AGPRs, (-?\d+) B scratch per lane, (-?\d+) B LDS")


def poisson_loglik(obs_data_i, ode_data_i, ind, **params):
    import numpy as np
    from rodeo_amd.trace import gammaln
    eta = 0.1 + 0.5 * ode_data_i[:, 0]
    y = obs_data_i.flatten()
    return np.sum(y * eta - np.exp(eta) - gammaln(y + 1.0))


def child(rhs, p):
    """Build the four forward kernels of every interrogation for one (right-hand side, n_bstate); the figures go to stderr."""
    from rodeo_amd import _lib
    from rodeo_amd.trace import trace_obs_source
    rid, d = {"fitzhugh_nagumo": (_lib.RHS_FITZHUGH_NAGUMO, 2), "lorenz63": (_lib.RHS_LORENZ63, 3)}[rhs]
    lib = _lib.load()
    name = f"PoissonObs_{rhs}_{p}"
    src, _ = trace_obs_source(poisson_loglik, d, p, 1, (("theta", 3),), name)
    oid = C.c_int32(0)
    _lib.check(lib.rk_register_obs_source(name.encode(), src.encode(), d, p, 1, 3, 1, C.byref(oid)))
    for itg in range(3):
        _lib.check(lib.rk_obs_compile_check(oid.value, rid, itg))
        _lib.check(lib.rk_obs_grid_compile_check(oid.value, rid, itg))


def measure(rhs, p):
    env = dict(os.environ, RK_JIT_VERBOSE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", rhs, str(p)], env=env, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(f"{rhs} p={p}: {r.stderr[-2000:]}")
    rows = {}
    for sym, vgpr, agpr, scratch, lds in LINE.findall(r.stderr):
        m = re.search(r"daltonng(_grid)?_fwd_kernelI.*ELi\d+ELi(\d+)ELi\d+ELb([01])EEEv", sym)      # <RHS, OBS, P, ITG, MO, BOTH>
        if m:
            rows[(int(m.group(2)), m.group(3) == "1", m.group(1) is not None)] = (int(vgpr), int(agpr), int(scratch), int(lds))
    return rhs, p, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2)
    ap.add_argument("--jobs", type=int, default=4)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]))
    import check_code_objects as cco
    cases = [("fitzhugh_nagumo", p) for p in range(2, 7)] + [("lorenz63", p) for p in range(3, 6)]
    with ThreadPoolExecutor(a.jobs) as pool:
        results = list(pool.map(lambda c: measure(*c), cases))
    lines = ["daltonng_grid: registers (.vgpr_count/.agpr_count of the metadata), scratch per lane and LDS of the new kernels, gfx950 (scripts/daltonng_grid_code_objects.py)",
             "", "forward kernel (hiprtc, Poisson model): daltonng_grid_fwd_kernel next to daltonng_fwd_kernel of the same form",
             "the ship rule: no more scratch than daltonng_fwd_kernel at the same (RHS, P, ITG, form)", "",
             f"{'rhs':16s} {'p':>1s} {'itg':8s} {'form':6s} | {'grid: regs':>10s} {'scratch':>8s} {'LDS':>7s} | {'uniform: regs':>13s} {'scratch':>8s} {'LDS':>5s} | rule"]
    broken = []
    for rhs, p, rows in results:
        for itg in range(3):
            for both in (True, False):
                g, u = rows[(itg, both, True)], rows[(itg, both, False)]
                ok = g[2] <= u[2]
                if not ok:
                    broken.append((rhs, p, ITG[itg], "both" if both else "store"))
                lines.append(f"{rhs:16s} {p:1d} {ITG[itg]:8s} {'both' if both else 'store':6s} | {f'{g[0]}/{g[1]}':>10s} {g[2]:8d} {g[3]:7d} | "
                             f"{f'{u[0]}/{u[1]}':>13s} {u[2]:8d} {u[3]:5d} | {'ships' if ok else 'LEFT OUT'}")
    lines += ["", f"instances that break the rule: {broken if broken else 'none'}", "",
              "gain kernel (ahead of time): daltonng_grid_gain_kernel<P> next to daltonng_gain_kernel<P>", ""]
    ks = [k for k in cco.kernels_of(os.path.join(ROOT, "rodeo_amd", "librodeo_kalman.so")) if "gain_kernel" in k["name"] and "daltonng" in k["name"]]
    def gain_name(k):
        return ("daltonng_grid_gain_kernel" if "grid" in k["name"] else "daltonng_gain_kernel") + "<%s>" % re.search(r"ILi(\d+)E", k["name"]).group(1)
    for k in sorted(ks, key=gain_name):
        lines.append(f"{gain_name(k):32s} regs {k.get('vgpr_count', 0):3d}/{k.get('agpr_count', 0):<3d}  scratch "
                     f"{k.get('private_segment_fixed_size', 0):5d} B  LDS {k.get('group_segment_fixed_size', 0):5d} B")
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
