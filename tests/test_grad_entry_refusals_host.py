"""
What the four gradient entries -- ``rk_dalton_grid_jvp``, ``rk_dalton_grid_jvp_hyper``, ``rk_fenrir_grid_jvp``,
``rk_fenrir_grid_jvp_hyper`` -- and ``rk_fenrir_grid_jvp_workspace_bytes`` answer on the configuration and the scalar arguments
alone (no handle, no pointers; no GPU): return code and message text of every configuration that differs from a served base in
one or two places, against the table recorded in ``tests/golden/grad_entry_refusals.npz``
(``tests/golden/make_grad_entry_refusals.py``), the way ``test_grid_entry_refusals_host.py`` does it for the grid family.  The
table was recorded from the library as it was before the two entries' checks became csrc/grid_entry.hpp's one ``grad_check``.
"""
import ctypes as C
import functools
import io
import os
import re
import zipfile
import numpy as np
from rodeo_amd import _lib
from rodeo_amd.trace import grad_from_python
from test_grid_entry_refusals_host import CFG_DEVIATIONS as GRID_CFG_DEVIATIONS, _fitz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "grad_entry_refusals.npz")


@functools.lru_cache(maxsize=None)
def _user_grad_id():
    return grad_from_python(_fitz, 2, 3, theta=3).rhs_id


def bases():
    """(rhs_id, n_block, n_bstate) of the served bases: FitzHugh-Nagumo at 3 and 2, Lorenz63, one traced right-hand side of the
    gradient kind."""
    return [(_lib.RHS_FITZHUGH_NAGUMO, 2, 3), (_lib.RHS_FITZHUGH_NAGUMO, 2, 2), (_lib.RHS_LORENZ63, 3, 3), (_user_grad_id(), 2, 3)]


def _bytes_call(lib, c, a):
    n = C.c_size_t(0)
    rc = lib.rk_fenrir_grid_jvp_workspace_bytes(c, a["n_dir"], C.byref(n))
    a["bytes"] = n.value if rc == 0 else -1
    return rc


ENTRIES = [
    ("rk_dalton_grid_jvp", ("n_bobs", "n_dir"),
     lambda lib, c, a: lib.rk_dalton_grid_jvp(None, c, None, None, None, None, None, 1, a["n_bobs"], None, a["n_dir"], None, 0, None,
                                              0, None, None)),
    ("rk_dalton_grid_jvp_hyper", ("n_bobs", "n_dir"),
     lambda lib, c, a: lib.rk_dalton_grid_jvp_hyper(None, c, None, None, None, None, None, 1, a["n_bobs"], None, a["n_dir"], None, 0,
                                                    None, 0, None, 0, None, 0, None, None)),
    ("rk_fenrir_grid_jvp", ("n_bobs", "n_dir"),
     lambda lib, c, a: lib.rk_fenrir_grid_jvp(None, c, None, None, None, None, None, None, 1, a["n_bobs"], None, a["n_dir"], None, 0,
                                              None, 0, None, None, None)),
    ("rk_fenrir_grid_jvp_hyper", ("n_bobs", "n_dir"),
     lambda lib, c, a: lib.rk_fenrir_grid_jvp_hyper(None, c, None, None, None, None, None, None, 1, a["n_bobs"], None, a["n_dir"], None,
                                                    0, None, 0, None, 0, None, 0, None, None, None)),
    ("rk_fenrir_grid_jvp_workspace_bytes", ("n_dir",), _bytes_call),
]

# the grid family's deviations of the configuration, the n_bstate values between what ships and what a variant build has, and the
# n_traj at which the two item limits part: 2^30 trajectories are 2^30 DALTON items and 2^31 or more Fenrir items
CFG_DEVIATIONS = GRID_CFG_DEVIATIONS + [("n_bstate", 2), ("n_bstate", 5), ("n_traj", 0), ("n_traj", 2 ** 30)]
EXTRA_DEVIATIONS = [("n_bobs", 0), ("n_bobs", 4), ("n_dir", 0), ("n_dir", -3), ("n_dir", 2), ("n_dir", 3)]
DEVIATIONS = CFG_DEVIATIONS + EXTRA_DEVIATIONS
CFG_FIELDS = {f for f, _ in CFG_DEVIATIONS}


def cases(extras):
    """Index tuples into DEVIATIONS: none (the base), every single deviation the entry has, every pair in two fields."""
    have = [i for i, (f, _) in enumerate(DEVIATIONS) if f in CFG_FIELDS or f in extras]
    pairs = [(i, j) for k, i in enumerate(have) for j in have[k + 1:] if DEVIATIONS[i][0] != DEVIATIONS[j][0]]
    return [()] + [(i,) for i in have] + pairs


def grad_entry_refusal_table():
    """(rows, messages): int64 rows of (entry, base, first deviation, second deviation, return code, message, bytes), the
    deviations as indices into DEVIATIONS (-1: none), the message as an index into `messages` -- the distinct texts of
    rk_last_error() in order of first appearance, the registration id replaced by a fixed token, "" behind RK_OK -- and bytes what
    rk_fenrir_grid_jvp_workspace_bytes stored (-1: it refused, or another entry)."""
    lib = _lib.load()
    user_id = _user_grad_id()
    rows, messages = [], {}
    for e, (name, extras, call) in enumerate(ENTRIES):
        for b, (rhs, d, p) in enumerate(bases()):
            for case in cases(extras):
                cfg = dict(n_traj=16, n_steps=50, n_block=d, n_bstate=p, n_bmeas=1, rhs_id=rhs, interrogate=_lib.INTERROGATE_KRAMER,
                           kalman_type=_lib.KALMAN_STANDARD, n_theta=3, flags=_lib.FLAG_BATCH_MINOR, t_min=0.0, t_max=1.0, seed=0,
                           traj_offset=0)
                args = dict(n_bobs=1, n_dir=1, bytes=-1)
                for i in case:
                    field, value = DEVIATIONS[i]
                    if value == "other":
                        value = 5 - d                                  # (two blocks <-> three)
                    (cfg if field in CFG_FIELDS else args)[field] = value
                rc = call(lib, C.byref(_lib.SolveCfg(**cfg)), args)
                msg = re.sub(r"\b%d\b" % user_id, "<user rhs>", lib.rk_last_error().decode()) if rc else ""
                rows.append((e, b, case[0] if case else -1, case[1] if len(case) > 1 else -1, rc, messages.setdefault(msg, len(messages)),
                             args["bytes"]))
    return np.array(rows, dtype=np.int64), np.array(list(messages), dtype=np.str_)


def write_table(path):
    """The table as an .npz with a fixed date, so that the same table gives the same bytes."""
    rows, messages = grad_entry_refusal_table()
    with zipfile.ZipFile(path, "w") as z:
        for name, array in (("rows", rows), ("messages", messages)):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, array, allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    return rows, messages


def describe(row):
    e, b, i, j = (int(v) for v in row[:4])
    devs = ", ".join("%s=%r" % DEVIATIONS[k] for k in (i, j) if k >= 0) or "the base itself"
    return "%s, base %d (rhs, n_block, n_bstate = %s): %s" % (ENTRIES[e][0], b, bases()[b], devs)


def test_every_gradient_refusal_is_the_recorded_one():
    """Return code, message text and workspace size of every case, exactly; the first differing case is printed."""
    want = np.load(GOLDEN)
    want_rows, want_msg = want["rows"], want["messages"]
    rows, msg = grad_entry_refusal_table()
    assert rows.shape == want_rows.shape, (rows.shape, want_rows.shape)
    assert np.array_equal(rows[:, :4], want_rows[:, :4]), "the cases themselves differ from the recorded ones"
    got = [(int(r[4]), str(msg[r[5]]), int(r[6])) for r in rows]
    exp = [(int(r[4]), str(want_msg[r[5]]), int(r[6])) for r in want_rows]
    bad = [k for k in range(len(got)) if got[k] != exp[k]]
    if bad:
        k = bad[0]
        print("first of %d differing cases: %s\n  got  %r\n  want %r" % (len(bad), describe(rows[k]), got[k], exp[k]))
    assert not bad, "%d cases differ, first: %s: got %r, want %r" % (len(bad), describe(rows[bad[0]]), got[bad[0]], exp[bad[0]])
    assert np.array_equal(rows, want_rows) and np.array_equal(msg, want_msg)     # (the file itself would be rewritten as it is)


def test_the_recorded_file_is_regenerated_byte_for_byte(tmp_path):
    """The archive of this library's table, as tests/golden/make_grad_entry_refusals.py writes it, has the committed file's bytes."""
    out = tmp_path / "grad_entry_refusals.npz"
    write_table(str(out))
    with open(GOLDEN, "rb") as f:
        assert out.read_bytes() == f.read()


def test_the_gradient_table_covers_what_it_says():
    """Every entry with each base, every single deviation and pairs in two fields; the four entries never return RK_OK (every
    call ends at the null handle at the latest), and the workspace size is served where the sizes and n_dir are valid."""
    rows = np.load(GOLDEN)["rows"]
    assert set(rows[:, 0]) == set(range(len(ENTRIES))) and set(rows[:, 1]) == set(range(len(bases())))
    for e, (_, extras, _) in enumerate(ENTRIES):
        mine = rows[(rows[:, 0] == e) & (rows[:, 1] == 0)]
        assert len(mine) == len(cases(extras))
        singles = {int(r[2]) for r in mine if r[2] >= 0 and r[3] < 0}
        assert singles == {i for i, (f, _) in enumerate(DEVIATIONS) if f in CFG_FIELDS or f in extras}
        assert all(DEVIATIONS[r[2]][0] != DEVIATIONS[r[3]][0] for r in mine if r[3] >= 0)
    jvp = rows[rows[:, 0] < 4]
    assert (jvp[:, 4] != _lib.RK_OK).all() and (jvp[:, 6] == -1).all()
    size = rows[rows[:, 0] == 4]
    assert ((size[:, 4] == _lib.RK_OK) == (size[:, 6] >= 0)).all() and (size[:, 4] == _lib.RK_OK).any()
    # the two item limits part where they should: 2^30 trajectories, one direction
    k = DEVIATIONS.index(("n_traj", 2 ** 30))
    msgs = np.load(GOLDEN)["messages"]
    for e, word in ((0, "n_traj * n_dir = "), (2, "n_traj * n_dir * n_block = ")):
        with_dirs = rows[(rows[:, 0] == e) & (rows[:, 1] == 0) & (rows[:, 2] == k) & (rows[:, 3] == DEVIATIONS.index(("n_dir", 3)))]
        assert len(with_dirs) == 1 and word in str(msgs[with_dirs[0, 5]])
