"""Launch head of the fused MNIST step's two kernels, read off the compiler's gfx950 assembly.

Both kernels start cold at every step, and nothing in them can happen before the kernel arguments have
arrived.  The property kept here: between a kernel's entry and its first vector-memory load there is
exactly ONE wait for scalar loads (``s_waitcnt ... lgkmcnt(0)`` with an ``s_load_dword*`` outstanding),
on every path of the control-flow graph -- all the arguments needed up to there are fetched in one
batch, not in dependent round trips.  It regresses silently when somebody adds an early use of a field
that is not fetched in the entry batch (the compiler then loads it where it is used and waits again).

A wait with no scalar load outstanding is not counted: the diagnostics stamp's ``s_memrealtime`` ends in
one (only when a stamp buffer is passed), and it fetches no argument.  Vector stores do not end a path
(the stamp is one), so the diagnostics path is held to the same count up to its first load.

The file is compiled with kernel-argument preloading (build_native.HIP_FILE_FLAGS): the dispatcher puts
the leading 14 argument dwords in SGPRs before a wave starts, and each kernel begins with a compatibility
prologue -- scalar loads of those dwords, one wait, a branch to the real entry -- that runs only where
the firmware does not preload.  The walk starts at the real entry, where the count is then 0 for
k_fwd_conv (everything in front of its first loads is preloaded) and still exactly 1 for
k_finalize_x<1, false> (its far fields, one batch); through the prologue both are one more, never two.

Only ``s_load_dword*``, ``s_waitcnt``, branch and vector-memory mnemonics are read.  No GPU needed.
"""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")


def _file_flags():
    spec = importlib.util.spec_from_file_location("build_native", os.path.join(HERE, "build_native.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.HIP_FILE_FLAGS.get("mnist_cnn.hip", []))

_VLOAD = re.compile(r"^(global|buffer|flat|scratch)_(load|atomic)")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("launch_head") / "mnist_cnn.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", *_file_flags(),
           "-I" + os.path.join(HERE, "csrc"), os.path.join(HERE, "csrc", "kernels", "mnist_cnn.hip"), "-o", str(out)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return out.read_text().splitlines()


def function_blocks(lines, symbol_re):
    """The function whose label matches symbol_re as basic blocks: [(label, [(mnemonic, operands)])], in
    text order (block 0 = the entry).  A block ends at a label or behind a branch."""
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l) and re.search(symbol_re, l.split(":")[0])]
    assert len(starts) == 1, (symbol_re, [lines[i] for i in starts])
    blocks, cur = [("entry", [])], None
    for l in lines[starts[0] + 1:]:
        if l.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            blocks.append((m.group(1), []))
            continue
        t = l.split(";")[0].strip()
        if not t or t.startswith("."):
            continue
        mn, _, ops = t.partition(" ")
        blocks[-1][1].append((mn, ops.strip()))
        if mn.startswith(("s_branch", "s_cbranch", "s_endpgm")):
            blocks.append((None, []))
    return blocks


def real_entry(blocks):
    """Index of the block that a preloading dispatcher enters: behind the compatibility prologue (block 0
    = nothing but scalar loads, ONE wait and a branch) if there is one, else 0."""
    ins = blocks[0][1]
    if not ins or ins[-1][0] != "s_branch":
        return 0
    body = [mn for mn, _ in ins[:-1]]
    if not all(mn.startswith("s_load_dword") or mn == "s_waitcnt" for mn in body):
        return 0
    assert body.count("s_waitcnt") == 1 and body[-1] == "s_waitcnt", ins
    return {lab: i for i, (lab, _) in enumerate(blocks) if lab}[ins[-1][1]]


def waits_to(blocks, stop, start=0):
    """Scalar-load waits on every path from block `start` to the first instruction that `stop` accepts
    (or to the program's end): the set of counts over all paths, and the instruction each path ended at."""
    index = {lab: i for i, (lab, _) in enumerate(blocks) if lab}
    counts, ends, seen = set(), set(), set()
    todo = [(start, False, 0)]
    while todo:
        state = todo.pop()
        if state in seen:
            continue
        seen.add(state)
        b, pending, n = state
        done = False
        for mn, ops in blocks[b][1]:
            if mn.startswith("s_load_dword"):
                pending = True
            elif mn == "s_waitcnt" and "lgkmcnt(0)" in ops:
                if pending:
                    n += 1
                pending = False
            elif stop(mn):
                counts.add(n)
                ends.add(mn)
                done = True
                break
            elif mn == "s_endpgm":
                counts.add(n)
                ends.add(mn)
                done = True
                break
            elif mn == "s_branch":
                todo.append((index[ops], pending, n))
                done = True
                break
            elif mn.startswith("s_cbranch"):
                todo.append((index[ops], pending, n))
            assert n < 64, "wait count runs away (a loop with a scalar load)"
        if not done and b + 1 < len(blocks):
            todo.append((b + 1, pending, n))  # fall through
    return counts, ends


FWD = r"k_fwd_conv"
FINALIZE = r"k_finalize_xILi1ELb0E"  # k_finalize_x<1, false>: one replica, one workgroup per range


def test_parser_sees_the_kernels(asm):
    for sym in (FWD, FINALIZE):
        blocks = function_blocks(asm, sym)
        mns = [mn for _, ins in blocks for mn, _ in ins]
        assert any(mn.startswith("s_load_dword") for mn in mns)
        assert any(_VLOAD.match(mn) for mn in mns)
        assert "s_endpgm" in mns
        # every branch target is a block of this function
        labels = {lab for lab, _ in blocks}
        for _, ins in blocks:
            for mn, ops in ins:
                if mn.startswith(("s_branch", "s_cbranch")):
                    assert ops in labels, (mn, ops)


def _is_vload(mn):
    return bool(_VLOAD.match(mn))


def test_fwd_conv_one_argument_wait_before_first_vector_load(asm):
    blocks = function_blocks(asm, FWD)
    entry = real_entry(blocks)
    counts, ends = waits_to(blocks, _is_vload, entry)
    # preloaded: nothing to wait for at the real entry, and exactly the prologue's wait where it runs
    assert counts == ({0} if entry else {1}), (counts, ends)
    assert all(_is_vload(e) for e in ends), ends  # no path ends the program without loading
    assert waits_to(blocks, _is_vload)[0] == {1}


def test_finalize_one_argument_wait_before_first_vector_load(asm):
    blocks = function_blocks(asm, FINALIZE)
    entry = real_entry(blocks)
    counts, ends = waits_to(blocks, _is_vload, entry)
    assert counts == {1}, (counts, ends)
    assert waits_to(blocks, _is_vload)[0] == ({2} if entry else {1})


def test_finalize_one_argument_wait_on_each_range_kinds_path(asm):
    # the operand loads of every range kind (dense tasks, conv2 quads, conv1 groups) are buffer loads; the
    # waves with no task run to the end.  Its learning-rate and epoch words are plain global loads in front
    # of the range-kind branch, so the walk does not stop at them.
    blocks = function_blocks(asm, FINALIZE)
    counts, ends = waits_to(blocks, lambda mn: mn.startswith("buffer_load"), real_entry(blocks))
    assert counts == {1}, (counts, ends)
    assert any(e.startswith("buffer_load") for e in ends), ends
