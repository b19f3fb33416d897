#!/usr/bin/env python3
"""
Registers / scratch / LDS of every dalton_grid_fwd_kernel instance in rodeo_amd/librodeo_kalman.so next to its two siblings at
the same parameters, dalton_fwd_kernel<RHS, P, ITG, MO, STORE> and grid_fwd_kernel<RHS, P, ITG>, and the rule an instance ships
by: no more scratch than the larger of the two.  Writes profiles/dalton_grid_code_objects.txt and
prints the instances that break the rule: those must be the ones dalton_grid.hip's dalton_grid_ships() leaves out (the listing is
made from a build with every instance in it, -DRK_DALTON_GRID_ALL_INSTANCES; in the shipped library they do not exist).

    python3 scripts/dalton_grid_code_objects.py [path/to/librodeo_kalman.so]
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_code_objects as cco                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITG = {0: "rodeo", 1: "schober", 2: "kramer", 3: "chkrebtii"}


def _res(k):
    return (k.get("vgpr_count", 0) + k.get("agpr_count", 0), k.get("private_segment_fixed_size", 0),
            k.get("group_segment_fixed_size", 0))


def main():
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "rodeo_amd", "librodeo_kalman.so")
    cco.DPP_RESULTS = None
    new, dalton, grid = {}, {}, {}
    for k in cco.kernels_of(so):
        nm = k["name"]                                               # (mangled: the build needs no demangler)
        m = re.match(r"_ZN2rk\d+(dalton_grid_fwd_kernel|dalton_fwd_kernel)INS_\d+([A-Za-z]\w*?)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])EEEv", nm)
        if m:
            key = (m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5)), m.group(6) == "1")
            (new if m.group(1) == "dalton_grid_fwd_kernel" else dalton)[key] = _res(k)
            continue
        m = re.match(r"_ZN2rk\d+grid_fwd_kernelINS_\d+([A-Za-z]\w*?)ELi(\d+)ELi(\d+)EEEv", nm)
        if m:
            grid[(m.group(1), int(m.group(2)), int(m.group(3)))] = _res(k)
    lines = ["# registers (VGPR + AGPR) / scratch B per lane / LDS B of every dalton_grid_fwd_kernel<RHS, P, ITG, MO, STORE> instance,",
             "# next to dalton_fwd_kernel at the same parameters and grid_fwd_kernel<RHS, P, ITG>.  An instance ships only if its",
             "# scratch is no more than the larger of the two siblings' (scripts/dalton_grid_code_objects.py).",
             f"# {'rhs':<15} {'P':>1} {'itg':<8} {'MO':>2} {'form':<6} | {'dalton_grid':>17} | {'dalton':>17} | {'grid':>17} | rule"]
    broken = []
    for key in sorted(new):
        rhs, p, itg, mo, store = key
        a, d, g = new[key], dalton.get(key), grid.get((rhs, p, itg))
        if d is None or g is None:
            broken.append(key)
            verdict = "NO SIBLING"
        else:
            ok = a[1] <= max(d[1], g[1])
            verdict = "ok" if ok else "LEFT OUT (refused by the library and in Python)"
            if not ok:
                broken.append(key)

        def fmt(r):
            return "        -        " if r is None else f"{r[0]:>4} /{r[1]:>5} /{r[2]:>6}"
        lines.append(f"  {rhs:<15} {p} {ITG.get(itg, itg):<8} {mo:>2} {'store' if store else 'loglik':<6} | {fmt(a)} | {fmt(d)} | {fmt(g)} | {verdict}")
    lines.append(f"# {len(new)} instances, {len(broken)} break the rule")
    out = os.path.join(ROOT, "profiles", "dalton_grid_code_objects.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1], "->", out)
    for key in broken:
        print("  ", key)
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main())
