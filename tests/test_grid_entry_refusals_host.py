"""
What the twelve entries of the non-uniform-grid family answer on the configuration and the scalar arguments alone (no handle,
no pointers; no GPU): return code and message text of every configuration that differs from a served base in one or two places,
against the table recorded in ``tests/golden/grid_entry_refusals.npz`` (``tests/golden/make_grid_entry_refusals.py``).  Pairs of
deviations are what fix the order of an entry's tests: which of two refusals a doubly wrong configuration gets.  The table was
recorded from the library as it was before the entries' host sides were put on csrc/grid_entry.hpp.
"""
import ctypes as C
import functools
import itertools
import os
import re
import numpy as np
from rodeo_amd import _lib
from rodeo_amd.trace import from_python, gammaln, trace_obs_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "grid_entry_refusals.npz")
UNREGISTERED_OBS = 10 ** 6


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


def _poisson_loglik(obs_data_i, ode_data_i, ind, **params):
    eta = 0.1 + 0.5 * ode_data_i[:, 0]
    y = obs_data_i.flatten()
    return np.sum(y * eta - np.exp(eta) - gammaln(y + 1.0))


@functools.lru_cache(maxsize=None)
def _obs_id(d, p):
    """An observation model registered for (n_block, n_bstate) = (d, p), three parameters."""
    name = f"RefusalTableObs_{d}_{p}"
    src, _ = trace_obs_source(_poisson_loglik, d, p, 1, (("theta", 3),), name)
    oid = C.c_int32(0)
    _lib.check(_lib.load().rk_register_obs_source(name.encode(), src.encode(), d, p, 1, 3, 1, C.byref(oid)))
    return oid.value


@functools.lru_cache(maxsize=None)
def _user_rhs_id():
    return from_python(_fitz, 2, 3, theta=3).rhs_id


def bases():
    """(rhs_id, n_block, n_bstate) of the three served bases: FitzHugh-Nagumo, Lorenz63 and one traced right-hand side."""
    return [(_lib.RHS_FITZHUGH_NAGUMO, 2, 3), (_lib.RHS_LORENZ63, 3, 5), (_user_rhs_id(), 2, 3)]


# ---- the entries: name, the scalar extras each one takes, and the call with no handle and no pointers --------------------
_KEEP = (C.c_int32 * 2)(0, 1)


def _keep(a):
    return (C.cast(_KEEP, C.c_void_p), 0) if a["keep"] else (None, 0)


ENTRIES = [
    ("rk_solve_grid", ("mode",), lambda lib, c, a: lib.rk_solve_grid(None, c, None, None, a["mode"], None)),
    ("rk_solve_evidence_grid", (), lambda lib, c, a: lib.rk_solve_evidence_grid(None, c, None, None, None, None, None)),
    ("rk_solve_dynamic_grid", ("mode", "scale_min"),
     lambda lib, c, a: lib.rk_solve_dynamic_grid(None, c, None, None, a["mode"], None, a["scale_min"], None, None)),
    ("rk_solve_sim_draws_grid", ("n_draws", "keep"),
     lambda lib, c, a: lib.rk_solve_sim_draws_grid(None, c, None, None, None, a["n_draws"], *_keep(a), None)),
    ("rk_dalton_grid_sim_draws", ("n_bobs", "n_draws", "keep"),
     lambda lib, c, a: lib.rk_dalton_grid_sim_draws(None, c, None, None, None, None, None, None, 1, a["n_bobs"], None, a["n_draws"],
                                                    *_keep(a), None)),
    ("rk_dalton_grid_loglik", ("n_bobs",),
     lambda lib, c, a: lib.rk_dalton_grid_loglik(None, c, None, None, None, None, None, 1, a["n_bobs"], None, None)),
    ("rk_dalton_grid_solve", ("mode", "n_bobs"),
     lambda lib, c, a: lib.rk_dalton_grid_solve(None, c, None, None, a["mode"], None, None, None, None, 1, a["n_bobs"], None)),
    ("rk_daltonng_grid_loglik", ("obs_id",),
     lambda lib, c, a: lib.rk_daltonng_grid_loglik(None, c, None, a["obs_id"], None, None, 1, None, None, 0, None)),
    ("rk_daltonng_grid_solve", ("mode", "obs_id"),
     lambda lib, c, a: lib.rk_daltonng_grid_solve(None, c, None, None, a["mode"], a["obs_id"], None, None, 1, None)),
    ("rk_fenrir_grid_loglik", ("n_bobs",),
     lambda lib, c, a: lib.rk_fenrir_grid_loglik(None, c, None, None, None, None, None, None, 1, a["n_bobs"], None, None)),
    ("rk_fenrir_grid_solve_mv", ("n_bobs",),
     lambda lib, c, a: lib.rk_fenrir_grid_solve_mv(None, c, None, None, None, None, None, None, 1, a["n_bobs"], None, None)),
    ("rk_dalton_grid_jvp", ("n_bobs", "n_dir"),
     lambda lib, c, a: lib.rk_dalton_grid_jvp(None, c, None, None, None, None, None, 1, a["n_bobs"], None, a["n_dir"], None, 0, None,
                                              0, None, None)),
]

# ---- the deviations: (field, value); "other" is resolved per base, "keep" means n_keep = 0 next to a keep array ----------
CFG_DEVIATIONS = [("n_steps", 0), ("n_block", 0), ("n_block", "other"), ("n_bstate", 0), ("n_bstate", 1), ("n_bstate", 4),
                  ("n_bstate", 6), ("n_bstate", 7), ("n_bmeas", 0), ("n_bmeas", 2), ("interrogate", 3), ("interrogate", 9),
                  ("kalman_type", 1), ("kalman_type", 7), ("flags", 0), ("flags", _lib.FLAG_BATCH_MINOR | _lib.FLAG_STORE_PRED),
                  ("rhs_id", 77)]
EXTRA_DEVIATIONS = [("mode", 0), ("mode", 2), ("mode", 7), ("n_bobs", 0), ("n_bobs", 4), ("scale_min", -1.0), ("n_dir", 0),
                    ("n_draws", 0), ("keep", True), ("obs_id", UNREGISTERED_OBS)]
DEVIATIONS = CFG_DEVIATIONS + EXTRA_DEVIATIONS
CFG_FIELDS = {f for f, _ in CFG_DEVIATIONS}


def cases(extras):
    """Index tuples into DEVIATIONS: none (the base), every single deviation the entry has, every pair in two fields."""
    have = [i for i, (f, _) in enumerate(DEVIATIONS) if f in CFG_FIELDS or f in extras]
    pairs = [(i, j) for i, j in itertools.combinations(have, 2) if DEVIATIONS[i][0] != DEVIATIONS[j][0]]
    return [()] + [(i,) for i in have] + pairs


def _normalise(msg, user_id):
    """Ids handed out at registration depend on what else the process registered: a fixed token instead."""
    msg = re.sub(r"\b%d\b" % user_id, "<user rhs>", msg)
    return re.sub(r"observation model \d+", "observation model <obs>", msg)


def grid_entry_refusal_table():
    """(rows, messages): rows of (entry, base, first deviation, second deviation, return code, message), the deviations as
    indices into DEVIATIONS (-1: none) and the message as an index into `messages`, the distinct texts of rk_last_error() in
    order of first appearance ("" behind RK_OK, which no row has: every call ends at the null handle at the latest)."""
    lib = _lib.load()
    user_id = _user_rhs_id()
    rows, messages = [], {}
    for e, (name, extras, call) in enumerate(ENTRIES):
        for b, (rhs, d, p) in enumerate(bases()):
            for case in cases(extras):
                cfg = dict(n_traj=16, n_steps=50, n_block=d, n_bstate=p, n_bmeas=1, rhs_id=rhs, interrogate=_lib.INTERROGATE_KRAMER,
                           kalman_type=_lib.KALMAN_STANDARD, n_theta=3, flags=_lib.FLAG_BATCH_MINOR, t_min=0.0, t_max=1.0, seed=0,
                           traj_offset=0)
                args = dict(mode=_lib.MODE_MV, n_bobs=1, scale_min=0.0, n_dir=1, n_draws=2, keep=False, obs_id=_obs_id(d, p))
                for i in case:
                    field, value = DEVIATIONS[i]
                    if value == "other":
                        value = 5 - d                                  # (two blocks <-> three)
                    (cfg if field in CFG_FIELDS else args)[field] = value
                rc = call(lib, C.byref(_lib.SolveCfg(**cfg)), args)
                msg = _normalise(lib.rk_last_error().decode(), user_id) if rc else ""
                rows.append((e, b, case[0] if case else -1, case[1] if len(case) > 1 else -1, rc, messages.setdefault(msg, len(messages))))
    return np.array(rows, dtype=np.int32), np.array(list(messages), dtype=np.str_)


def describe(row):
    e, b, i, j = (int(v) for v in row[:4])
    devs = ", ".join("%s=%r" % DEVIATIONS[k] for k in (i, j) if k >= 0) or "the base itself"
    return "%s, base %d (rhs, n_block, n_bstate = %s): %s" % (ENTRIES[e][0], b, bases()[b], devs)


def test_every_refusal_is_the_recorded_one():
    """Return code and message text of every case, exactly; the first differing case is printed."""
    want = np.load(GOLDEN)
    want_rows, want_msg = want["rows"], want["messages"]
    rows, msg = grid_entry_refusal_table()
    assert rows.shape == want_rows.shape, (rows.shape, want_rows.shape)
    assert np.array_equal(rows[:, :4], want_rows[:, :4]), "the cases themselves differ from the recorded ones"
    got = [(int(r[4]), str(msg[r[5]])) for r in rows]
    exp = [(int(r[4]), str(want_msg[r[5]])) for r in want_rows]
    bad = [k for k in range(len(got)) if got[k] != exp[k]]
    if bad:
        k = bad[0]
        print("first of %d differing cases: %s\n  got  %r\n  want %r" % (len(bad), describe(rows[k]), got[k], exp[k]))
    assert not bad, "%d cases differ, first: %s: got %r, want %r" % (len(bad), describe(rows[bad[0]]), got[bad[0]], exp[bad[0]])
    assert np.array_equal(rows, want_rows) and np.array_equal(msg, want_msg)     # (the file itself would be rewritten as it is)


def test_the_table_covers_what_it_says():
    """Every entry with each of the three bases, every single deviation and pairs in two fields; no call returned RK_OK."""
    rows = np.load(GOLDEN)["rows"]
    assert set(rows[:, 0]) == set(range(len(ENTRIES))) and set(rows[:, 1]) == {0, 1, 2}
    for e, (_, extras, _) in enumerate(ENTRIES):
        mine = rows[(rows[:, 0] == e) & (rows[:, 1] == 0)]
        assert len(mine) == len(cases(extras))
        singles = {int(r[2]) for r in mine if r[2] >= 0 and r[3] < 0}
        assert singles == {i for i, (f, _) in enumerate(DEVIATIONS) if f in CFG_FIELDS or f in extras}
        assert all(DEVIATIONS[r[2]][0] != DEVIATIONS[r[3]][0] for r in mine if r[3] >= 0)
    assert (rows[:, 4] != _lib.RK_OK).all()
