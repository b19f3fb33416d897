#!/usr/bin/env python3
"""
Registers / scratch / LDS of every grid_evidence_kernel and grid_dynamic_fwd_kernel instance in rodeo_amd/librodeo_kalman.so
next to its uniform counterpart at the same (RHS, P, ITG), evidence_kernel or dynamic_fwd_kernel, and to grid_fwd_kernel, and of
the backward instances grid_dynamic_bwd_mv_kernel / grid_dynamic_bwd_sim_kernel next to grid_bwd_* and dynamic_bwd_*.  The rule
a forward instance ships by: no more scratch than its uniform counterpart.  Writes
profiles/grid_calib_code_objects.txt and prints the instances that break the rule.

    python3 scripts/grid_calib_code_objects.py [path/to/librodeo_kalman.so]
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_code_objects as cco                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITG = {0: "rodeo", 1: "schober", 2: "kramer", 3: "chkrebtii"}
PAIRS = {"grid_evidence_kernel": "evidence_kernel", "grid_dynamic_fwd_kernel": "dynamic_fwd_kernel"}
BWD = ("grid_dynamic_bwd_mv_kernel", "grid_dynamic_bwd_sim_kernel", "grid_bwd_mv_kernel", "grid_bwd_sim_kernel",
       "dynamic_bwd_mv_kernel", "dynamic_bwd_sim_kernel")


def _res(k):
    return (k.get("vgpr_count", 0) + k.get("agpr_count", 0), k.get("private_segment_fixed_size", 0),
            k.get("group_segment_fixed_size", 0))


def _fmt(r):
    return "        -        " if r is None else f"{r[0]:>4} /{r[1]:>5} /{r[2]:>6}"


def main():
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "rodeo_amd", "librodeo_kalman.so")
    cco.DPP_RESULTS = None
    fwd, bwd = {}, {}
    for k in cco.kernels_of(so):
        nm = k["name"]                                               # (mangled: the build needs no demangler)
        m = re.match(r"_ZN2rk\d+(\w+?_kernel)INS_\d+([A-Za-z]\w*?)ELi(\d+)ELi(\d+)EEEv", nm)
        if m:
            fwd[(m.group(1), m.group(2), int(m.group(3)), int(m.group(4)))] = _res(k)
            continue
        m = re.match(r"_ZN2rk\d+(\w+?_kernel)ILi(\d+)EEEv", nm)
        if m and m.group(1) in BWD:
            bwd[(m.group(1), int(m.group(2)))] = _res(k)
    lines = ["# registers (VGPR + AGPR) / scratch B per lane / LDS B of every grid_evidence_kernel<RHS, P, ITG> and",
             "# grid_dynamic_fwd_kernel<RHS, P, ITG> instance, next to its uniform counterpart (evidence_kernel / dynamic_fwd_kernel)",
             "# and grid_fwd_kernel at the same parameters.  A forward instance ships only if its scratch is no more than the",
             "# uniform counterpart's (scripts/grid_calib_code_objects.py).",
             f"# {'kernel':<24} {'rhs':<15} {'P':>1} {'itg':<8} | {'on the grid':>17} | {'uniform':>17} | {'grid_fwd_kernel':>17} | rule"]
    broken, n = [], 0
    for key in sorted(fwd):
        name, rhs, p, itg = key
        if name not in PAIRS:
            continue
        n += 1
        a, u, g = fwd[key], fwd.get((PAIRS[name], rhs, p, itg)), fwd.get(("grid_fwd_kernel", rhs, p, itg))
        if u is None:
            verdict = "NO COUNTERPART"
        else:
            verdict = "ok" if a[1] <= u[1] else "BREAKS THE RULE"
        if verdict != "ok":
            broken.append(key)
        lines.append(f"  {name:<24} {rhs:<15} {p} {ITG.get(itg, itg):<8} | {_fmt(a)} | {_fmt(u)} | {_fmt(g)} | {verdict}")
    lines.append(f"# {n} forward instances, {len(broken)} break the rule")
    lines.append("# backward instances (one lane per (trajectory, block); scripts/check_code_objects.py's limits: 2048 B of scratch)")
    lines.append(f"# {'P':>1} | {'grid_dynamic_bwd_mv':>19} | {'grid_bwd_mv':>17} | {'dynamic_bwd_mv':>17} | {'grid_dynamic_bwd_sim':>20} | "
                 f"{'grid_bwd_sim':>17} | {'dynamic_bwd_sim':>17}")
    for p in sorted({p for (nm, p) in bwd if nm.startswith("grid_dynamic")}):
        lines.append(f"  {p} |   {_fmt(bwd.get((BWD[0], p)))} | {_fmt(bwd.get((BWD[2], p)))} | {_fmt(bwd.get((BWD[4], p)))} |    "
                     f"{_fmt(bwd.get((BWD[1], p)))} | {_fmt(bwd.get((BWD[3], p)))} | {_fmt(bwd.get((BWD[5], p)))}")
    out = os.path.join(ROOT, "profiles", "grid_calib_code_objects.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"# {n} forward instances, {len(broken)} break the rule ->", out)
    for key in broken:
        print("  ", key)
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main())
