"""
The packed smoothed rows of solve_mv at p = 3 (RK_LAYOUT_TILE3_PACKED), checked on the host.  A stand-alone C++ program
(tests/tile3_pack_out_check.cpp, its own main) includes the header the kernels include (rodeo_amd/csrc/tile3_pack.hpp) and
sweeps every (N <= 70, tile count <= 12, step, tile, slot): the map is injective, never touches the rows 0 and N or another
tile-wave's stripe, equals the filtered record's bytes, and the smoother's store offsets reach it.  It writes the index of
every slot to a file, and the two NumPy gathers of ``SolvePlan`` (``tile3_unpack`` for a whole array, ``tile3_row_host`` for
single rows) must read exactly those doubles; the size rule Python uses is the library's (``rk_tile3_packed_waves``).
Built with the host compiler under AddressSanitizer and UBSan where the compiler has them.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

SLOTS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3))       # slot -> (row, column) of [Sigma | mu]


@pytest.fixture(scope="module")
def index_table(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tile3_pack_out")
    exe, table = str(tmp / "tile3_pack_out_check"), str(tmp / "index.bin")
    base = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rodeo_amd", "csrc"),
            os.path.join(ROOT, "tests", "tile3_pack_out_check.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:                               # a compiler without the sanitizer runtimes: the plain program
        r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, table], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "0 failure(s)" in r.stdout
    words = np.fromfile(table, dtype=np.int32)
    out, at = {}, 0
    while at < len(words):
        N, T, W = (int(x) for x in words[at:at + 3])
        at += 3
        n = (N - 1) * 4 * W * 9 if W else 0
        out[(N, T)] = (W, words[at:at + n].reshape(N - 1, 4 * W, 9) if W else None)
        at += n
    assert len(out) == 70 * 12
    return out


def test_map_invariants(index_table):
    """The program's own checks passed (the fixture asserts it); the sweep covers the gate and both kinds of tile-wave."""
    assert index_table[(15, 12)][0] == 0 and index_table[(16, 12)][0] == 3 and index_table[(16, 3)][0] == 0
    assert index_table[(70, 7)][0] == 1 and index_table[(70, 7)][1].shape == (69, 4, 9)


class _Rows:
    """var_state of a plan, on the host: the one method the row helper uses"""

    def __init__(self, raw):
        self.raw, self.shape = raw, raw.shape

    def slice0_host(self, i):
        return self.raw[i % self.shape[0]].copy()


def _plan(N, B, d, raw=None):
    from rodeo_amd import _lib
    from rodeo_amd.solve import SolvePlan

    class Dev:
        lib = _lib.load()

    p = SolvePlan.__new__(SolvePlan)
    p.dev, p.N, p.B, p.d, p.p = Dev(), N, B, d, 3
    p.layout, p.records_layout, p.smoothed_tile3 = _lib.LAYOUT_TILE3, _lib.LAYOUT_TILE3_PACKED, False
    p.var_state = _Rows(raw) if raw is not None else None
    return p


def _expected(raw, N, T, W, idx):
    """Natural tiles from `raw` by the program's indices: the packed records with their symmetric Sigma, the rest as it lies."""
    exp = raw.reshape(N + 1, T, 3, 4).copy()
    if W:
        flat = raw.ravel()
        for slot, (i, j) in enumerate(SLOTS):
            exp[1:N, :4 * W, i, j] = flat[idx[..., slot]]
            if j < 3:
                exp[1:N, :4 * W, j, i] = flat[idx[..., slot]]
    return exp


def test_whole_array_gather_reads_the_map(index_table):
    """SolvePlan.tile3_unpack on an array that holds its own indices, at every (N, tile count), n_block 1 and 2."""
    from rodeo_amd import _lib
    for (N, T), (W, idx) in index_table.items():
        for d in (1, 2):
            if T % d:
                continue
            plan = _plan(N, T // d, d)
            assert plan.packed_waves() == W, (N, T)
            raw = np.arange((N + 1) * T * 12, dtype=np.float64).reshape(N + 1, T // d, d, 3, 4)
            got = plan.tile3_unpack(raw.copy(), plan.packed_waves())
            np.testing.assert_array_equal(got.reshape(N + 1, T, 3, 4), _expected(raw, N, T, W, idx), err_msg=f"N {N} T {T} d {d}")
    natural = _plan(40, 8, 1)
    natural.records_layout = _lib.LAYOUT_TILE3                 # the library reported natural rows: nothing is gathered
    assert natural.packed_waves() == 0


@pytest.mark.parametrize("T", [4, 7, 12])
def test_row_gather_reads_the_map(index_table, T):
    """SolvePlan.tile3_row_host (one or two stripe rows per packed step) and mean_rows_host, every N and every row."""
    for N in range(1, 71):
        W, idx = index_table[(N, T)]
        raw = np.arange((N + 1) * T * 12, dtype=np.float64).reshape(N + 1, T, 1, 3, 4)
        plan, exp = _plan(N, T, 1, raw), _expected(raw, N, T, W, idx)
        for n in range(N + 1):
            np.testing.assert_array_equal(plan.tile3_row_host(n).reshape(T, 3, 4), exp[n], err_msg=f"N {N} T {T} n {n}")
        np.testing.assert_array_equal(plan.tile3_row_host(-1).reshape(T, 3, 4), exp[N])
        rows = [0, N // 2, N]
        np.testing.assert_array_equal(plan.mean_rows_host(rows), np.stack([exp[n][..., 3].reshape(T, 1, 3) for n in rows], axis=1))


def test_mirror_rule():
    """Smoothed p = 3 tiles: Sigma's lower triangle is the upper one, in place; filtered ones are left alone."""
    plan = _plan(20, 4, 1)
    t = np.arange(4 * 12, dtype=np.float64).reshape(4, 1, 3, 4)
    np.testing.assert_array_equal(plan._tile3_mirror(t.copy()), t)
    plan.smoothed_tile3 = True
    m = plan._tile3_mirror(t.copy())
    np.testing.assert_array_equal(m[..., :3], np.triu(t[..., :3]) + np.swapaxes(np.triu(t[..., :3], 1), -1, -2))
    np.testing.assert_array_equal(m[..., 3], t[..., 3])


def test_abi_is_opt_in(monkeypatch):
    """rk_solve_layout reports RK_LAYOUT_TILE3_PACKED only with RK_FLAG_TILE3_PACKED_MV, for RK_MODE_MV, on the route that
    packs (built-in tile-form right-hand side at n_block = 2, standard form, not chkrebtii, RK_TILE3_PACK not "0"); the buffer
    has one size in both layouts; rk_tile3_packed_waves is the size rule.  Host only: no device is touched."""
    import ctypes as C
    from rodeo_amd import _lib
    lib = _lib.load()
    monkeypatch.delenv("RK_TILE3_PACK", raising=False)

    def layout(mode=_lib.MODE_MV, flags=_lib.FLAG_TILE3_PACKED_MV, rhs=_lib.RHS_FITZHUGH_NAGUMO, d=2, p=3,
               itg=_lib.INTERROGATE_KRAMER, kalman=_lib.KALMAN_STANDARD, sizes=False):
        cfg = _lib.SolveCfg(n_traj=8, n_steps=50, n_block=d, n_bstate=p, n_bmeas=1, rhs_id=rhs, interrogate=itg, kalman_type=kalman,
                            n_theta=3, flags=flags, t_min=0.0, t_max=1.0, seed=0, traj_offset=0)
        lay = C.c_int32(-1)
        assert lib.rk_solve_layout(C.byref(cfg), mode, C.byref(lay)) == _lib.RK_OK
        if sizes:
            mb, vb = C.c_size_t(1), C.c_size_t(0)
            assert lib.rk_solve_sizes(C.byref(cfg), lay.value, C.byref(mb), C.byref(vb)) == _lib.RK_OK
            return lay.value, mb.value, vb.value
        return lay.value

    assert layout() == _lib.LAYOUT_TILE3_PACKED
    assert layout(flags=0) == _lib.LAYOUT_TILE3                                        # a caller who sets nothing: today's layout
    assert layout(mode=_lib.MODE_FILTER) == layout(mode=_lib.MODE_SIM) == _lib.LAYOUT_TILE3
    assert layout(itg=_lib.INTERROGATE_CHKREBTII) == _lib.LAYOUT_TILE3
    assert layout(rhs=_lib.RHS_LORENZ63, d=3) == _lib.LAYOUT_TILE3                     # n_block = 3
    assert layout(rhs=_lib.RHS_HIGHER_ORDER, d=1) == _lib.LAYOUT_TILE3                 # n_block = 1
    assert layout(flags=_lib.FLAG_TILE3_PACKED_MV | _lib.FLAG_BATCH_MINOR) == _lib.LAYOUT_BATCH_MINOR
    assert layout(kalman=_lib.KALMAN_SQRT) == layout(kalman=_lib.KALMAN_SQRT, flags=0)  # ignored off the tile route
    assert layout(p=4) == layout(p=4, flags=0) and layout(p=5) == layout(p=5, flags=0)
    packed, natural = layout(sizes=True), layout(flags=0, sizes=True)
    assert packed[1:] == natural[1:] == (0, (51 * 16 * 12 + 128 * 2) * 8)
    monkeypatch.setenv("RK_TILE3_PACK", "0")
    assert layout() == _lib.LAYOUT_TILE3
    monkeypatch.setenv("RK_TILE3_PACK", "1")
    assert layout() == _lib.LAYOUT_TILE3_PACKED
    waves = lib.rk_tile3_packed_waves
    assert [waves(15, 8), waves(16, 8), waves(16, 3), waves(16, 4), waves(4000, 2048), waves(4000, 2050)] == [0, 2, 0, 1, 512, 512]
    assert waves(17, 1520000) == 0                                                      # 18 rows of 146 MB: 2 GiB and more
    big = 0x7fff0000 // (96 * 17)
    assert waves(16, big) == big // 4 and waves(16, big + 1) == 0                       # the store window, to the tile
