"""Bit-for-bit comparison of the gradient entries between two builds of the library: ``value`` and
``dvalue`` of dalton_grid_jvp / fenrir_grid_jvp, without and with the "log_sigma" / "log_obs_var" directions.

    RK_LIB_PATH=path/to/librodeo_kalman.so python scripts/grad_shared_bits.py dump OUT.npz     one build, one fresh process
    python scripts/grad_shared_bits.py compare REFERENCE.npz SAME_BUILD_AGAIN.npz OTHER_BUILD.npz [report]

The cases: the 42 of tests/hyper_grad_cases.py (the hyper entries), those of tests/dalton_grad_cases.py and
tests/fenrir_grad_cases.py (the plain entries) -- B = 1, K = 1; B = 3, K = 5; 33 and 65 items; N = 1, 2, 3; nodes 0 and N among
others; Lorenz63 and FitzHugh-Nagumo; n_bstate 2 and 3; the three interrogations; shared and per-trajectory directions -- and,
on N = 8 steps: observations on node 0 and node N only, N = 1 and N = 2 with 65 trajectories (a second backward wave one item
wide at K = 1), a traced right-hand side through hiprtc, and Fenrir in two chunks of directions.  `compare` prints how many arrays
are byte-identical and names every case that differs; the second file shows that two runs of one build agree in the first place.
"""
import os
import sys
import numpy as np
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE, os.path.join(HERE, "tests")]


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


def runs_of():
    """(label, case, *_grid_jvp, right-hand side or None) of every run, and the module whose chunk budget the last two change."""
    import rodeo_amd.inference.dalton  # noqa: F401
    import rodeo_amd.inference.fenrir  # noqa: F401
    import grid_cases as gc
    import dalton_grid_cases as dc
    import dalton_grad_cases as gcs
    import fenrir_grad_cases as fgcs
    import hyper_grad_cases as hc
    dmod, fmod = sys.modules["rodeo_amd.inference.dalton"], sys.modules["rodeo_amd.inference.fenrir"]
    jvp = {"dalton": dmod.dalton_grid_jvp, "fenrir": fmod.fenrir_grid_jvp}
    runs = [("hyper | " + g["label"], g, jvp[g["family"]], None) for g in hc.cases()]
    runs += [("plain dalton | " + g["label"], g, jvp["dalton"], None) for g in gcs.cases()]
    runs += [("plain fenrir | " + g["label"], g, jvp["fenrir"], None) for g in fgcs.cases()]
    ends = dc.make(dc._short(3, "kramer", 8, B=3), (0, 8))                                   # node 0 and node N only
    wide = [dc.make(dc._short(3, "kramer", N, B=65), dc.SHORT_NODES[N]) for N in (1, 2)]    # 65 items a block at K = 1
    for family in ("dalton", "fenrir"):
        plain = gcs.grad_case if family == "dalton" else fgcs.fenrir_case
        runs += [(f"extra plain {family} | ends", plain(ends, "small"), jvp[family], None),
                 (f"extra hyper {family} | ends", hc.hyper_case(ends, family, "standard"), jvp[family], None),
                 (f"extra plain {family} | ends, traced", plain(ends, "small"), jvp[family], _fitz),
                 (f"extra hyper {family} | ends, traced", hc.hyper_case(ends, family, "standard"), jvp[family], _fitz)]
        for c in wide:
            runs += [(f"extra plain {family} | {c['label']}", plain(c, "theta0"), jvp[family], None),
                     (f"extra hyper {family} | {c['label']}", hc.hyper_case(c, family, "common"), jvp[family], None)]
    # Fenrir in chunks, last: K = 5 (9 with the hyper directions) under a budget of three directions' records
    runs += [("extra plain fenrir | ends, chunks of 3", fgcs.fenrir_case(ends, "small"), jvp["fenrir"], "chunks"),
             ("extra hyper fenrir | ends, chunks of 3", hc.hyper_case(ends, "fenrir", "standard"), jvp["fenrir"], "chunks")]
    return runs, fmod, 3 * len(ends["t"]) * 2 * (3 + 9) * 3 * 8


def dump(out):
    runs, fmod, budget = runs_of()
    arrays = {}
    for i, (label, g, fn, ode) in enumerate(runs):
        if ode == "chunks":                                          # (the last two runs: the budget stays changed to the end)
            fmod._GRAD_WORKSPACE_BYTES, ode = budget, None
        value, dvalue = g.device_jvp(fn, ode=ode) if ode is not None else g.device_jvp(fn)
        arrays["%03d %s" % (i, label)] = np.concatenate([np.atleast_1d(np.asarray(value, dtype=np.float64)).ravel(),
                                                         np.asarray(dvalue, dtype=np.float64).ravel()])
    np.savez(out, labels=np.array(list(arrays), dtype=np.str_), **{"a%d" % i: a for i, a in enumerate(arrays.values())})
    print("dumped", len(arrays), "cases ->", out, "from", os.environ.get("RK_LIB_PATH", "the tree's library"))


def _load(path):
    z = np.load(path)
    return {str(label): z["a%d" % i] for i, label in enumerate(z["labels"])}


def compare(ref, again, other, report=None):
    a, b, c = _load(ref), _load(again), _load(other)
    lines = ["# scripts/grad_shared_bits.py: value and dvalue of every case, one fresh process a build, compared byte by byte"]
    for name, x, y in (("parent against parent", a, b), ("branch against parent", a, c)):
        assert list(x) == list(y), "the two files hold different cases"
        differ = [k for k in x if x[k].tobytes() != y[k].tobytes()]
        kinds = {kind: sum(1 for k in x if k[4:].startswith(kind)) for kind in ("hyper", "plain dalton", "plain fenrir", "extra")}
        lines.append(f"{name}: {len(x) - len(differ)} of {len(x)} cases byte-identical ({kinds}), {sum(v.size for v in x.values())} "
                     f"doubles; {len(differ)} differ")
        for k in differ:
            n = int(np.sum(x[k].view(np.uint64) != y[k].view(np.uint64))) if x[k].shape == y[k].shape else -1
            worst = float(np.max(np.abs(x[k] - y[k]))) if x[k].shape == y[k].shape else float("nan")
            lines.append(f"  DIFFERS {k}: {n} of {x[k].size} doubles, largest difference {worst:.3e}")
    print("\n".join(lines))
    if report:
        with open(report, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if any("DIFFERS" in line for line in lines) else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) in (5, 6) and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
