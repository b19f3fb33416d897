"""
The packed in-place layout of the p = 3 filtered rows (rodeo_amd/csrc/tile3_pack.hpp), checked on the host: a stand-alone
C++ program (tests/tile3_pack_check.cpp, its own main) includes the header the kernels include and checks its invariants
exhaustively for N = 16 .. 300 -- the map is injective and stays in the tile-wave's own stripes of rows 1 .. N-1; stripe row m
holds steps >= m - 1 only; and the 16-byte pieces of every smoother chunk bring exactly that chunk's records to the places
the producers read them from.  Built with the host compiler under AddressSanitizer and UBSan where the compiler has them.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")


def test_tile3_pack_invariants(tmp_path):
    exe = str(tmp_path / "tile3_pack_check")
    base = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rodeo_amd", "csrc"),
            os.path.join(ROOT, "tests", "tile3_pack_check.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:                               # a compiler without the sanitizer runtimes: the plain program
        r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "0 failure(s)" in r.stdout
