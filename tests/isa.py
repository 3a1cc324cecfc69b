"""Reading the emitted gfx950 assembly of the library's units (test_loader_isa_cpu.py, test_ws_superstep_isa_cpu.py,
test_ws_prologue_isa_cpu.py, test_wgrad_rows_isa_cpu.py): a unit of physicsvae_amd/csrc is compiled with the flags of
physicsvae_amd/build.py plus -S --cuda-device-only, once per (unit, extra flags) and process, and the helpers cut a kernel
out of it and group its instructions by hipcc's loop comments.  No GPU needed; the tests skip where there is no hipcc."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

from physicsvae_amd import build as B

DMA = re.compile(r"^\s+(global_load_lds_dwordx4|buffer_load_dwordx4\b.*\blds\b)")
KERNELS = {
    "ws<P_ROW, EpiBiasAct>": r"_ZN4pvae\d+gemm_splitk_ws_kernelILb1ENS_10EpiBiasActEEE",
    "ws<P_COL, EpiMask>": r"_ZN4pvae\d+gemm_splitk_ws_kernelILb0ENS_7EpiMaskEEE",
    "ws64<P_ROW, EpiBiasAct, 32>": r"_ZN4pvae\d+gemm_splitk_ws64_kernelILb1ENS_10EpiBiasActELi32EEE",
    "ws64<P_ROW, EpiBiasAct, 64>": r"_ZN4pvae\d+gemm_splitk_ws64_kernelILb1ENS_10EpiBiasActELi64EEE",
    "ws64<P_COL, EpiMask, 32>": r"_ZN4pvae\d+gemm_splitk_ws64_kernelILb0ENS_7EpiMaskELi32EEE",
    "ws64<P_COL, EpiMask, 64>": r"_ZN4pvae\d+gemm_splitk_ws64_kernelILb0ENS_7EpiMaskELi64EEE",
}
# DMA instructions a loader wave issues per k-tile: Q pieces + P pieces
PIECES = {"ws<P_ROW, EpiBiasAct>": 4, "ws<P_COL, EpiMask>": 4, "ws64<P_ROW, EpiBiasAct, 32>": 6,
          "ws64<P_ROW, EpiBiasAct, 64>": 8, "ws64<P_COL, EpiMask, 32>": 6, "ws64<P_COL, EpiMask, 64>": 8}


@functools.lru_cache(maxsize=None)
def assembly(unit, flags=()):
    """The lines of `unit`'s device assembly (skips the calling test where there is no hipcc)."""
    try:
        cc = B._hipcc()
    except RuntimeError:
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory(prefix="pvae_isa_") as tmp:
        out = os.path.join(tmp, "unit.s")
        res = subprocess.run([cc] + B.FLAGS + list(flags) + ["-S", "--cuda-device-only", os.path.join(B.CSRC, unit), "-o", out],
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        with open(out) as f:
            return f.read().split("\n")


@pytest.fixture(scope="module")
def asm():
    return assembly("pvae_net.hip")


def function_lines(asm, pattern):
    start = [i for i, l in enumerate(asm) if re.match(r"^%s\w*:" % pattern, l)]
    assert len(start) == 1, (pattern, len(start))
    end = next(i for i in range(start[0], len(asm)) if asm[i].startswith(".Lfunc_end"))
    return asm[start[0]:end]


def loader_loop_blocks(fn):
    """Basic blocks (lists of instruction lines) of the innermost loops that hold an LDS-DMA.  hipcc labels every block
    with the loop it belongs to: `=>This Inner Loop Header: Depth=d` on the header, `in Loop: Header=BBn_m Depth=d` on the
    rest (no deeper loop exists inside an `Inner Loop`)."""
    loops, cur = {}, None
    for l in fn:
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", l) or re.match(r"^; %bb\.\d+:(.*)$", l)
        if m:
            note = m.group(m.lastindex)
            head = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
            if "This Inner Loop Header" in note:
                cur = loops.setdefault(m.group(1)[2:], [])
                cur.append([])
            elif head and head.group(1) in loops:
                cur = loops[head.group(1)]
                cur.append([])
            else:
                cur = None
        elif cur is not None and l.startswith("\t") and not l.strip().startswith(";"):
            cur[-1].append(l)
    return [blocks for blocks in loops.values() if any(DMA.match(i) for b in blocks for i in b)]


def inner_loops(fn):
    """{header label: flat list of instruction lines} of every innermost loop of the function (hipcc's block comments, as in
    loader_loop_blocks)."""
    loops, cur = {}, None
    for l in fn:
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", l) or re.match(r"^; %bb\.\d+:(.*)$", l)
        if m:
            note = m.group(m.lastindex)
            head = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
            if "This Inner Loop Header" in note:
                cur = loops.setdefault(m.group(1)[2:], [])
            elif head and head.group(1) in loops:
                cur = loops[head.group(1)]
            else:
                cur = None
        elif cur is not None and l.startswith("\t") and not l.strip().startswith(";"):
            cur.append(l)
    return loops
