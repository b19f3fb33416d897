"""
What hipcc makes of the headline forward filter's time loop (fwd_tile3_kernel<FitzHughNagumo, KRAMER>): one wave per SIMD
runs it, so every instruction of the loop body is on the critical path.  The store's buffer descriptor is
built once in front of the loop and the time row travels in the store's scalar offset; the loop runs four steps per
iteration.  This pins that property in the assembly, so that a later edit of the step or of RK_STORE_BEHIND cannot bring
the per-step descriptor rebuild (s_and_b32 / s_mov_b32 between the MFMAs, a 64-bit pointer add behind the store) back
unnoticed.

Needs hipcc only, no GPU.  Per time step (loop-body counts over the unroll factor): exactly 7 v_mfma_f64_4x4x4_4b_f64, exactly
one buffer_store_dwordx2, no s_and_b32 / s_mov_b32, at most 2 SALU instructions (one offset add per step plus the
amortised counter, compare and branch; the loop this replaced had 6).
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNEL = "_ZN2rk16fwd_tile3_kernelINS_14FitzHughNagumoELi2EEEvNS_9SolveArgsEPd"     # ITG = RK_INTERROGATE_KRAMER = 2

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not installed")


def _instructions(lines):
    """mnemonics of the instruction lines (labels, directives, comments and the empty-asm markers dropped)"""
    out = []
    for ln in lines:
        ln = ln.split(";")[0].strip()
        if not ln or ln.startswith(".") or ln.endswith(":"):
            continue
        out.append(ln.split()[0])
    return out


def _innermost_loops(body):
    """[(label, lines)] of the loops hipcc marks 'Inner Loop Header': from the label to the branch back to it"""
    loops = []
    for i, ln in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if not m:
            continue
        k = i + 1                                       # the loop comment may continue on the lines behind the label
        while k < len(body) and body[k].lstrip().startswith(";"):
            k += 1
        if not any("Inner Loop Header" in c for c in body[i:k]):
            continue
        for j in range(i + 1, len(body)):
            if re.match(r"^\s*s_cbranch_\w+\s+" + re.escape(m.group(1)) + r"\s*$", body[j]):
                loops.append((m.group(1), body[i:j + 1]))
                break
        else:
            raise AssertionError(f"no branch back to {m.group(1)}")
    return loops


@pytest.fixture(scope="module")
def kernel_asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asm") / "solve_tile3.s")
    subprocess.run(["bash", os.path.join(ROOT, "scripts", "asm_of.sh"), "solve_tile3.hip", out], check=True, timeout=1200)
    text = open(out).read().splitlines()
    start = next(i for i, ln in enumerate(text) if ln.startswith(KERNEL + ":"))
    end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
    return text[start:end]


def _salu(ins):
    return [m for m in ins if m.startswith("s_") and m not in ("s_nop", "s_waitcnt")]


def test_makefile_and_asm_script_flags_agree():
    # the assembly read here is the library's only if scripts/asm_of.sh compiles with the Makefile's code-generation flags
    mk = open(os.path.join(ROOT, "rodeo_amd", "csrc", "Makefile")).read()
    sh = open(os.path.join(ROOT, "scripts", "asm_of.sh")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).split()
    for f in flags:
        if f in ("-Wall", "-I../../include") or f.startswith("--offload-arch"):
            continue
        assert f in sh.split(), f
    assert "--offload-arch=gfx950" in sh and "-falign-loops=64" in sh


def test_headline_time_loop_instruction_inventory(kernel_asm):
    loops = _innermost_loops(kernel_asm)
    assert loops, "no innermost loop found"
    per_loop = [(label, _instructions(lines), lines) for label, lines in loops]
    per_loop = [(l, ins, lines) for l, ins, lines in per_loop if "v_mfma_f64_4x4x4_4b_f64" in ins]
    assert per_loop, "no loop with fp64 MFMAs"
    main_label, main, main_lines = max(per_loop, key=lambda t: len(t[1]))

    for label, ins, _ in per_loop:                     # the unrolled loop and its tail
        n_mfma = ins.count("v_mfma_f64_4x4x4_4b_f64")
        assert n_mfma % 7 == 0, (label, n_mfma)
        unroll = n_mfma // 7
        print(f"{label}: unroll {unroll}, {len(ins)} instructions, SALU {_salu(ins)}, s_nop {ins.count('s_nop')}")
        assert ins.count("buffer_store_dwordx2") == unroll, label
        assert "s_and_b32" not in ins and "s_mov_b32" not in ins, (label, "the buffer descriptor is rebuilt in the loop")
        assert not any(m.startswith(("global_", "flat_", "scratch_", "s_load", "s_buffer_load")) for m in ins), label

    unroll = main.count("v_mfma_f64_4x4x4_4b_f64") // 7
    assert unroll == 4, unroll
    assert len(_salu(main)) <= 2 * unroll, _salu(main)
    # the stores stay in their own steps: one between every seven MFMAs, none collected at the end
    since = 0
    for m in main:
        if m == "v_mfma_f64_4x4x4_4b_f64":
            since += 1
        elif m == "buffer_store_dwordx2":
            assert since < 14, "two steps without a store in between"
            since = 0
    # the scalar offset carries the time row: an SGPR (not 0) in the store's soffset operand
    for ln in main_lines:
        if "buffer_store_dwordx2" in ln:
            assert re.search(r"s\[\d+:\d+\],\s*s\d+\s+offen", ln), ln
    # -falign-loops=64: the loop head sits on a 64-byte boundary
    head = next(i for i, ln in enumerate(kernel_asm) if ln.startswith(main_label + ":"))
    assert kernel_asm[head - 1].split() == [".p2align", "6"], kernel_asm[head - 1]
