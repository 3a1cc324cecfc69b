"""The loader waves of the wave-specialised forward / input-gradient kernels share their SIMDs with compute waves that
issue fp32 MFMAs back to back, which hold the vector issue (tools/dual_pipe.hip).  Their steady state must therefore issue
NO vector-ALU instruction: every LDS-DMA takes a wave-uniform SGPR base and a lane offset computed once in front of the
loop, one VGPR per DMA piece of a tile (pvae_gemm_ws.h, lds_dma16_sbase).  This test compiles pvae_net.hip to gfx950 assembly
with the flags of physicsvae_amd/build.py and reads the loader loops of the dense instances.  No GPU needed; skipped
where there is no hipcc."""
import os
import re
import subprocess

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


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    try:
        cc = B._hipcc()
    except RuntimeError:
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("isa") / "pvae.s")
    res = subprocess.run([cc] + B.FLAGS + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "pvae_net.hip"), "-o", out],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    with open(out) as f:
        return f.read().split("\n")


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


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_loader_loop_issues_no_vector_alu(asm, kernel):
    loops = loader_loop_blocks(function_lines(asm, KERNELS[kernel]))
    assert len(loops) == 1, "one loader loop expected, found %d" % len(loops)
    tiles = 0
    for block in loops[0]:
        dmas = [i for i in block if DMA.match(i)]
        if not dmas:
            continue
        tiles += 1
        last = max(n for n, i in enumerate(block) if DMA.match(i))
        valu = [i.strip() for i in block[:last] if i.split()[0].startswith("v_")]
        assert not valu, "vector-ALU instructions in front of a loader DMA:\n" + "\n".join(valu)
        addr = [re.split(r"[\s,]+", i.strip())[1] for i in dmas]          # the VGPR (pair) each DMA reads its address from
        assert len(dmas) == PIECES[kernel], (len(dmas), block)
        assert len(set(addr)) == len(addr), "DMAs of one tile share an address register: %s" % addr
    assert tiles >= 1
