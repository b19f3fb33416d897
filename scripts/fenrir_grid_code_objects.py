#!/usr/bin/env python3
"""
Registers / scratch / LDS of every fenrir_grid_bwd_kernel<P, STORE, MO> instance in rodeo_amd/librodeo_kalman.so next to its two
yardsticks at the same P, fenrir_bwd_kernel<P, STORE, MO> (the lane route, not its tile form) and grid_bwd_mv_kernel<P>, and the
rule an instance ships by: no more scratch than the larger of the two.  Writes
profiles/fenrir_grid_code_objects.txt and prints the instances that break the rule (exit code 1 if any): fenrir_grid.hip ships
all 30, so there must be none.

    python3 scripts/fenrir_grid_code_objects.py [path/to/librodeo_kalman.so]
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_code_objects as cco                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _res(k):
    return (k.get("vgpr_count", 0) + k.get("agpr_count", 0), k.get("private_segment_fixed_size", 0),
            k.get("group_segment_fixed_size", 0))


def main():
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "rodeo_amd", "librodeo_kalman.so")
    cco.DPP_RESULTS = None
    new, fenrir, grid = {}, {}, {}
    for k in cco.kernels_of(so):
        nm = k["name"]                                               # (mangled: the build needs no demangler)
        m = re.match(r"_ZN2rk\d+fenrir_grid_bwd_kernelILi(\d+)ELb([01])ELi(\d+)EEEv", nm)
        if m:
            new[(int(m.group(1)), m.group(2) == "1", int(m.group(3)))] = _res(k)
            continue
        m = re.match(r"_ZN2rk\d+fenrir_bwd_kernelILi(\d+)ELb([01])ELi(\d+)ELb0EEEv", nm)
        if m:
            fenrir[(int(m.group(1)), m.group(2) == "1", int(m.group(3)))] = _res(k)
            continue
        m = re.match(r"_ZN2rk\d+grid_bwd_mv_kernelILi(\d+)EEEv", nm)
        if m:
            grid[int(m.group(1))] = _res(k)
    lines = ["# registers (VGPR + AGPR) / scratch B per lane / LDS B of every fenrir_grid_bwd_kernel<P, STORE, MO> instance, next to",
             "# fenrir_bwd_kernel<P, STORE, MO> and grid_bwd_mv_kernel<P>.  An instance ships only if its scratch is no more than the",
             "# larger of the two yardsticks' (scripts/fenrir_grid_code_objects.py).",
             f"# {'P':>1} {'MO':>2} {'form':<6} | {'fenrir_grid':>17} | {'fenrir':>17} | {'grid_bwd_mv':>17} | rule"]
    broken = []
    for key in sorted(new):
        p, store, mo = key
        a, f, g = new[key], fenrir.get(key), grid.get(p)
        if f is None or g is None:
            broken.append(key)
            verdict = "NO YARDSTICK"
        else:
            ok = a[1] <= max(f[1], g[1])
            verdict = "ok" if ok else "LEFT OUT (refused by the library and in Python)"
            if not ok:
                broken.append(key)

        def fmt(r):
            return "        -        " if r is None else f"{r[0]:>4} /{r[1]:>5} /{r[2]:>6}"
        lines.append(f"  {p} {mo:>2} {'store' if store else 'loglik':<6} | {fmt(a)} | {fmt(f)} | {fmt(g)} | {verdict}")
    lines.append(f"# {len(new)} instances, {len(broken)} break the rule")
    out = os.path.join(ROOT, "profiles", "fenrir_grid_code_objects.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(lines[-1], "->", out)
    for key in broken:
        print("  ", key)
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main())
