"""The prologue of the plain dense 32x32 forward / input-gradient kernels (pvae_gemm_ws.h, splitk_ws_superstep_body) in the emitted
gfx950 assembly, beside test_loader_isa_cpu.py and test_ws_superstep_isa_cpu.py: k-tiles 0, 1 and 2 are fetched by all eight
waves, so the path every wave runs issues six LDS-DMA instructions through the two lane offsets of tile 0 (the only ones a
compute wave ever issues), the compute waves' loop holds none, the loaders add tiles 3 and 4 (four instructions each) outside
their loop, and the loader loop is what it was (two tiles of four DMAs per super-step, no vector-ALU instruction in front of
them); the blocks that request tiles 3 and 4 are scalar-only as well.  pvae_net.hip is compiled with the flags of
physicsvae_amd/build.py.  No GPU needed; skipped where there is no hipcc."""
import re

import pytest

from isa import DMA, KERNELS, asm, function_lines, inner_loops, loader_loop_blocks  # noqa: F401  (asm: the fixture)
from test_ws_superstep_isa_cpu import PLAIN


@pytest.mark.parametrize("kernel", sorted(PLAIN))
def test_prologue_fetches_three_tiles_with_all_waves(asm, kernel):
    fn = function_lines(asm, KERNELS[kernel])
    # the compute waves' loop: no DMA inside
    compute = [body for body in inner_loops(fn).values() if any(i.split()[0].startswith("v_mfma") for i in body)]
    assert len(compute) == 1, "one compute loop expected, found %d" % len(compute)
    assert not [i for i in compute[0] if DMA.match(i)], "LDS-DMA inside the compute waves' loop"
    # the loader loop: unchanged
    loops = loader_loop_blocks(fn)
    assert len(loops) == 1, "one loader loop expected, found %d" % len(loops)
    tiles = 0
    for block in loops[0]:
        dmas = [i for i in block if DMA.match(i)]
        if not dmas:
            continue
        tiles += 1
        last = max(n for n, i in enumerate(block) if DMA.match(i))
        assert not [i for i in block[:last] if i.split()[0].startswith("v_")], "vector-ALU in front of a loader DMA"
        assert len(dmas) == 4 and len({re.split(r"[\s,]+", i.strip())[1] for i in dmas}) == 4, dmas
    assert tiles == 2, "a loader super-step requests two k-tiles, found %d" % tiles
    # outside the loops: the shared prologue, three blocks (one per k-tile, each behind its guard) of two DMAs through the
    # same two lane-offset registers, and the loaders' tiles 3 and 4, four DMAs each in a scalar-only block -- a vector-ALU
    # instruction on the loader path behind the shared DMAs makes hipcc put an s_waitcnt vmcnt(0) in front of it, and
    # tiles 3 and 4 are then requested only after tiles 0-2 have landed
    cur, blocks = [], []
    for l in fn:
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", l):
            cur = []
            if "Loop" not in l:                            # (hipcc's block comments name the loop a block belongs to)
                blocks.append(cur)
        elif l.startswith("\t") and not l.strip().startswith(";"):
            cur.append(l)
    blocks = [b for b in blocks if any(DMA.match(i) for i in b)]
    count = lambda b: sum(1 for i in b if DMA.match(i))
    shared = [b for b in blocks if count(b) == 2]
    assert len(shared) == 3, "blocks of the shared prologue: %d" % len(shared)
    regs = {re.split(r"[\s,]+", i.strip())[1] for b in shared for i in b if DMA.match(i)}
    assert len(regs) == 2, "the six shared DMAs read their lane offsets from %s" % sorted(regs)
    own = [b for b in blocks if count(b) == 4]
    assert len(own) == 2 and len(blocks) == 5, "blocks that request tiles 3 and 4: %d of %d" % (len(own), len(blocks))
    for b in own:
        assert not [i for i in b if i.split()[0].startswith("v_")], "vector-ALU beside the loaders' prologue DMAs"
