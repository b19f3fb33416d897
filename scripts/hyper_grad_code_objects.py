#!/usr/bin/env python3
"""
Registers / scratch / LDS of every hyper instance in rodeo_amd/librodeo_kalman.so -- dalton_grid_jvp_hyper_kernel<RHS, P, ITG>,
fenrir_grid_jvp_fwd_hyper_kernel<RHS, P, ITG> and fenrir_grid_jvp_bwd_hyper_kernel<P> -- next to its non-hyper sibling, and the rule
an instance ships by: no more scratch than that sibling.  Writes profiles/hyper_grad_code_objects.txt
and prints the instances that break the rule (exit code 1): such an instance must not ship -- it has to be refused by the
library and in Python, as dalton_grad.hip's ``dalton_grad_pmax`` does for the plain kernels.  Today every instance passes.

    python3 scripts/hyper_grad_code_objects.py [path/to/librodeo_kalman.so]
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_code_objects as cco                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITG = {0: "rodeo", 1: "schober", 2: "kramer"}
FAMILIES = (("dalton_grid_jvp", "dalton_grid_jvp_hyper_kernel", "dalton_grid_jvp_kernel"),
            ("fenrir_grid_jvp fwd", "fenrir_grid_jvp_fwd_hyper_kernel", "fenrir_grid_jvp_fwd_kernel"))


def _res(k):
    return (k.get("vgpr_count", 0) + k.get("agpr_count", 0), k.get("private_segment_fixed_size", 0),
            k.get("group_segment_fixed_size", 0))


def _fmt(r):
    return "        -        " if r is None else f"{r[0]:>4} /{r[1]:>5} /{r[2]:>6}"


def main():
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "rodeo_amd", "librodeo_kalman.so")
    cco.DPP_RESULTS = None
    found = {}
    for k in cco.kernels_of(so):
        nm = k["name"]                                               # (mangled: the build needs no demangler)
        m = re.match(r"_ZN2rk\d+([a-z_]+_kernel)INS_\d+([A-Za-z]\w*?)ELi(\d+)ELi(\d+)EEEv", nm)
        if m:
            found[(m.group(1), m.group(2), int(m.group(3)), int(m.group(4)))] = _res(k)
            continue
        m = re.match(r"_ZN2rk\d+(fenrir_grid_jvp_bwd(?:_hyper)?_kernel)ILi(\d+)EEEv", nm)
        if m:
            found[(m.group(1), "", int(m.group(2)), -1)] = _res(k)
    lines = ["# registers (VGPR + AGPR) / scratch B per lane / LDS B of every hyper instance next to its non-hyper sibling:",
             "# dalton_grid_jvp_hyper_kernel<RHS, P, ITG> / dalton_grid_jvp_kernel, fenrir_grid_jvp_fwd_hyper_kernel<RHS, P, ITG> /",
             "# fenrir_grid_jvp_fwd_kernel, fenrir_grid_jvp_bwd_hyper_kernel<P> / fenrir_grid_jvp_bwd_kernel.  An instance ships only if its",
             "# scratch is no more than the sibling's (scripts/hyper_grad_code_objects.py).",
             f"# {'family':<20} {'rhs':<15} {'P':>1} {'itg':<8} | {'hyper':>17} | {'sibling':>17} | rule"]
    broken, n = [], 0
    rows = [(fam, hyper, sib, key[1], key[2], key[3]) for fam, hyper, sib in FAMILIES for key in sorted(found) if key[0] == hyper]
    rows += [("fenrir_grid_jvp bwd", "fenrir_grid_jvp_bwd_hyper_kernel", "fenrir_grid_jvp_bwd_kernel", "", key[2], -1)
             for key in sorted(found) if key[0] == "fenrir_grid_jvp_bwd_hyper_kernel"]
    for fam, hyper, sib, rhs, p, itg in rows:
        a, v = found[(hyper, rhs, p, itg)], found.get((sib, rhs, p, itg))
        n += 1
        fits = v is not None and a[1] <= v[1]
        verdict = "ok" if fits else "BREAKS THE RULE"
        if not fits:
            broken.append((fam, rhs, p, itg))
        lines.append(f"  {fam:<20} {rhs or '(backward)':<15} {p} {ITG.get(itg, ''):<8} | {_fmt(a)} | {_fmt(v)} | {verdict}")
    lines.append(f"# {n} hyper instances, {len(broken)} break the rule")
    out = os.path.join(ROOT, "profiles", "hyper_grad_code_objects.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1], "->", out)
    for key in broken:
        print("  ", key)
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main())
