#!/usr/bin/env python3
"""
Registers / scratch / LDS of every dalton_grid_jvp_kernel<RHS, P, ITG> instance in rodeo_amd/librodeo_kalman.so next to the value
kernel at the same parameters, dalton_grid_fwd_kernel<RHS, P, ITG, 1, false>, and the rule an instance ships by (DESIGN.md
section 7 (21)): no more scratch than that sibling.  Writes profiles/dalton_grad_code_objects.txt and prints the instances that
break the rule: those must be the ones dalton_grad.hip's dalton_grad_pmax() leaves out (the listing is made from a build with
the candidates in it, -DRK_DALTON_GRAD_ALL_INSTANCES; in the shipped library they do not exist).

    python3 scripts/dalton_grad_code_objects.py [path/to/librodeo_kalman.so]
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_code_objects as cco                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITG = {0: "rodeo", 1: "schober", 2: "kramer"}


def _res(k):
    return (k.get("vgpr_count", 0) + k.get("agpr_count", 0), k.get("private_segment_fixed_size", 0),
            k.get("group_segment_fixed_size", 0))


def main():
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "rodeo_amd", "librodeo_kalman.so")
    cco.DPP_RESULTS = None
    new, value = {}, {}
    for k in cco.kernels_of(so):
        nm = k["name"]                                               # (mangled: the build needs no demangler)
        m = re.match(r"_ZN2rk\d+dalton_grid_jvp_kernelINS_\d+([A-Za-z]\w*?)ELi(\d+)ELi(\d+)EEEv", nm)
        if m:
            new[(m.group(1), int(m.group(2)), int(m.group(3)))] = _res(k)
            continue
        m = re.match(r"_ZN2rk\d+dalton_grid_fwd_kernelINS_\d+([A-Za-z]\w*?)ELi(\d+)ELi(\d+)ELi1ELb0EEEv", nm)
        if m:
            value[(m.group(1), int(m.group(2)), int(m.group(3)))] = _res(k)
    lines = ["# registers (VGPR + AGPR) / scratch B per lane / LDS B of every dalton_grid_jvp_kernel<RHS, P, ITG> instance, next to",
             "# dalton_grid_fwd_kernel<RHS, P, ITG, 1, false>.  An instance ships only if its scratch is no more than the sibling's",
             "# (scripts/dalton_grad_code_objects.py).",
             f"# {'rhs':<15} {'P':>1} {'itg':<8} | {'dalton_grid_jvp':>17} | {'dalton_grid':>17} | rule"]
    broken = []
    for key in sorted(new):
        rhs, p, itg = key
        a, v = new[key], value.get(key)
        if v is None:
            verdict = "NO SIBLING"
        else:
            verdict = "ok" if a[1] <= v[1] else "LEFT OUT (refused by the library and in Python)"
        if verdict != "ok":
            broken.append(key)

        def fmt(r):
            return "        -        " if r is None else f"{r[0]:>4} /{r[1]:>5} /{r[2]:>6}"
        lines.append(f"  {rhs:<15} {p} {ITG.get(itg, itg):<8} | {fmt(a)} | {fmt(v)} | {verdict}")
    lines.append(f"# {len(new)} instances, {len(broken)} break the rule")
    out = os.path.join(ROOT, "profiles", "dalton_grad_code_objects.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1], "->", out)
    for key in broken:
        print("  ", key)
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main())
