#!/usr/bin/env python3
"""
Registers / scratch of every grid_bwd_sim_draws_kernel<P, C> instance in rodeo_amd/librodeo_kalman.so next to its two nearest
siblings, bwd_sim_draws_kernel<P, C> (sim_draws.hip) and grid_bwd_sim_kernel<P> (grid.hip), and the rule an instance ships by
(DESIGN.md section 7 (19)): check_code_objects.py's own limit, at most SCRATCH_LIMIT bytes of scratch per lane.  Writes
profiles/grid_draws_code_objects.txt and prints the instances that break the rule (none today): the dispatch of grid_draws.hip
would have to run a smaller chunk at that n_bstate, which changes no draw.

    python3 scripts/grid_draws_code_objects.py [path/to/librodeo_kalman.so]
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_code_objects as cco                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _res(k):
    return k.get("vgpr_count", 0) + k.get("agpr_count", 0), k.get("private_segment_fixed_size", 0)


def main():
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "rodeo_amd", "librodeo_kalman.so")
    cco.DPP_RESULTS = None
    new, draws, grid = {}, {}, {}
    for k in cco.kernels_of(so):
        nm = k["name"]                                               # (mangled: the build needs no demangler)
        m = re.match(r"_ZN2rk\d+(grid_bwd_sim_draws_kernel|bwd_sim_draws_kernel)ILi(\d+)ELi(\d+)EEEv", nm)
        if m:
            (new if m.group(1).startswith("grid") else draws)[(int(m.group(2)), int(m.group(3)))] = _res(k)
            continue
        m = re.match(r"_ZN2rk\d+grid_bwd_sim_kernelILi(\d+)EEEv", nm)
        if m:
            grid[int(m.group(1))] = _res(k)
    lines = ["# registers (VGPR + AGPR) / scratch B per lane of every grid_bwd_sim_draws_kernel<P, C> instance, next to",
             "# bwd_sim_draws_kernel<P, C> and grid_bwd_sim_kernel<P>.  An instance ships only with at most "
             f"{cco.SCRATCH_LIMIT} B of scratch",
             "# (scripts/check_code_objects.py's limit; scripts/grid_draws_code_objects.py).",
             f"# {'P':>1} {'C':>1} | {'grid_draws':>11} | {'sim_draws':>11} | {'grid_sim':>11} | rule"]
    broken = []

    def fmt(r):
        return "     -     " if r is None else f"{r[0]:>4} /{r[1]:>5}"
    for key in sorted(new):
        ok = new[key][1] <= cco.SCRATCH_LIMIT
        if not ok:
            broken.append(key)
        lines.append(f"  {key[0]} {key[1]} | {fmt(new[key])} | {fmt(draws.get(key))} | {fmt(grid.get(key[0]))} | "
                     f"{'ok' if ok else 'OVER THE LIMIT (cap this chunk in the dispatch)'}")
    lines.append(f"# {len(new)} instances, {len(broken)} break the rule")
    out = os.path.join(ROOT, "profiles", "grid_draws_code_objects.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1], "->", out)
    for key in broken:
        print("  ", key)
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main())
