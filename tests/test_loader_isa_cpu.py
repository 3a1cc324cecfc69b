"""The loader waves of the wave-specialised forward / input-gradient kernels share their SIMDs with compute waves that
issue fp32 MFMAs back to back, which hold the vector issue (tools/dual_pipe.hip).  Their steady state must therefore issue
NO vector-ALU instruction: every LDS-DMA takes a wave-uniform SGPR base and a lane offset computed once in front of the
loop, one VGPR per DMA piece of a tile (pvae_gemm_ws.h, lds_dma16_sbase).  This test compiles pvae_net.hip to gfx950 assembly
with the flags of physicsvae_amd/build.py and reads the loader loops of the dense instances.  No GPU needed; skipped
where there is no hipcc."""
import re

import pytest

from isa import DMA, KERNELS, PIECES, asm, function_lines, loader_loop_blocks  # noqa: F401  (asm: the fixture)


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
