#!/usr/bin/env python3
"""
Registers / scratch / LDS of every fenrir_grid_jvp_fwd_kernel<RHS, P, ITG> and fenrir_grid_jvp_bwd_kernel<P> instance in
rodeo_amd/librodeo_kalman.so next to its yardstick -- grid_fwd_kernel<RHS, P, ITG> and fenrir_grid_bwd_kernel<P, false, 1> -- and
the rule an instance ships by: no more scratch than the yardstick.  Writes
profiles/fenrir_grad_code_objects.txt and prints the instances that break the rule; those must not ship (fenrir_grad.hip's
FENRIR_GRAD_PMAX, ``_grad_config`` in Python).

    python3 scripts/fenrir_grad_code_objects.py [path/to/librodeo_kalman.so]
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


def _fmt(r):
    return "        -        " if r is None else f"{r[0]:>4} /{r[1]:>5} /{r[2]:>6}"


def main():
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "rodeo_amd", "librodeo_kalman.so")
    cco.DPP_RESULTS = None
    fwd, fwd_value, bwd, bwd_value = {}, {}, {}, {}
    for k in cco.kernels_of(so):
        nm = k["name"]                                               # (mangled: the build needs no demangler)
        m = re.match(r"_ZN2rk\d+fenrir_grid_jvp_fwd_kernelINS_\d+([A-Za-z]\w*?)ELi(\d+)ELi(\d+)EEEv", nm)
        if m:
            fwd[(m.group(1), int(m.group(2)), int(m.group(3)))] = _res(k)
            continue
        m = re.match(r"_ZN2rk\d+grid_fwd_kernelINS_\d+([A-Za-z]\w*?)ELi(\d+)ELi(\d+)EEEv", nm)
        if m:
            fwd_value[(m.group(1), int(m.group(2)), int(m.group(3)))] = _res(k)
            continue
        m = re.match(r"_ZN2rk\d+fenrir_grid_jvp_bwd_kernelILi(\d+)EEEv", nm)
        if m:
            bwd[int(m.group(1))] = _res(k)
            continue
        m = re.match(r"_ZN2rk\d+fenrir_grid_bwd_kernelILi(\d+)ELb0ELi1EEEv", nm)
        if m:
            bwd_value[int(m.group(1))] = _res(k)
    lines = ["# registers (VGPR + AGPR) / scratch B per lane / LDS B of every fenrir_grid_jvp_fwd_kernel<RHS, P, ITG> instance next to",
             "# grid_fwd_kernel<RHS, P, ITG>, and of every fenrir_grid_jvp_bwd_kernel<P> instance next to fenrir_grid_bwd_kernel<P, false, 1>.",
             "# An instance ships only if its scratch is no more than the yardstick's (scripts/fenrir_grad_code_objects.py).",
             f"# {'rhs':<15} {'P':>1} {'itg':<8} | {'fenrir_grid_jvp':>17} | {'yardstick':>17} | rule"]
    broken = []

    def row(label, key, a, v):
        verdict = "NO YARDSTICK" if v is None else ("ok" if a[1] <= v[1] else "LEFT OUT (refused by the library and in Python)")
        if verdict != "ok":
            broken.append(key)
        lines.append(f"  {label} | {_fmt(a)} | {_fmt(v)} | {verdict}")

    for key in sorted(fwd):
        rhs, p, itg = key
        row(f"{rhs:<15} {p} {ITG.get(itg, itg):<8}", key, fwd[key], fwd_value.get(key))
    for p in sorted(bwd):
        row(f"{'(backward)':<15} {p} {'':<8}", ("backward", p), bwd[p], bwd_value.get(p))
    lines.append(f"# {len(fwd)} forward and {len(bwd)} backward instances, {len(broken)} break the rule")
    out = os.path.join(ROOT, "profiles", "fenrir_grad_code_objects.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1], "->", out)
    for key in broken:
        print("  ", key)
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main())
