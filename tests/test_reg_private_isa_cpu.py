"""Wave-private staging of the register-staged split-K bodies (pvae_gemm_reg.h) in the emitted gfx950 assembly: every wave
stages exactly the chunks of a k-tile that it reads back, so the k-loops of splitk_reg_body and splitk_reg16_body hold no
workgroup barrier, and the first barrier behind a loop stands in front of the split-K reduction buffer, which overlays the
staging ring.  Read in bwd_pair_kernel<EpiMask, EpiGradStore, 0> (the input-gradient half of the hidden pairs) and in
gemm_splitk_reg16_kernel<true, EpiBiasAct> / <false, EpiActionSeed>:

  * the k-loop holds no s_barrier;
  * it still holds 16 (32x32 body) and 4 (16x16 body) MFMAs per k-tile -- a loop iteration is one group of D k-tiles,
    D = kRegDepthD = 2 and kRegDepth16 = 4 (pvae_gemm_common.h) -- and as many global_load_dwordx4 as before the change:
    four (32x32: two chunks of each operand) and two (16x16) per thread and k-tile;
  * behind the loop -- past the guarded tail tiles, that is past the last MFMA of the body -- an s_barrier comes in front of
    the first LDS write (the partial tile going into the reduction buffer).

The pair kernel holds four MFMA loops (two weight-gradient bodies, the 16x16 and the 32x32 input gradient); the 32x32
input-gradient loop is the one whose fragment reads are ds_read_b128 (dZ, one per 16-row block) and ds_read_b64 (W, one per
k-step) in the ratio 2 : 4 per k-tile.  pvae_net.hip is compiled with the flags of physicsvae_amd/build.py.  No GPU needed;
skipped where there is no hipcc."""
import re

import pytest

from isa import asm, function_lines  # noqa: F401  (asm: the fixture)

PAIR = r"_ZN4pvae\d+bwd_pair_kernelINS_7EpiMaskENS_12EpiGradStoreELi0EEE"
REG16 = {"reg16<P_ROW, EpiBiasAct>": r"_ZN4pvae\d+gemm_splitk_reg16_kernelILb1ENS_10EpiBiasActEEE",
         "reg16<P_COL, EpiActionSeed>": r"_ZN4pvae\d+gemm_splitk_reg16_kernelILb0ENS_13EpiActionSeedEEE"}
D32, D16 = 2, 4                      # kRegDepthD, kRegDepth16: k-tiles per loop iteration
LOADS32, LOADS16 = 4, 2              # global_load_dwordx4 per thread and k-tile, before and after the change


def mfma_loops(fn):
    """[(index of the loop's last line in fn, [mnemonics])] of the innermost loops that hold an MFMA (hipcc's block comments,
    as in isa.inner_loops)."""
    loops, cur = {}, None
    for n, l in enumerate(fn):
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", l) or re.match(r"^; %bb\.\d+:(.*)$", l)
        if m:
            note = m.group(m.lastindex)
            head = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
            if "This Inner Loop Header" in note:
                cur = loops.setdefault(m.group(1)[2:], [n, []])
            elif head and head.group(1) in loops:
                cur = loops[head.group(1)]
            else:
                cur = None
        elif cur is not None and l.startswith("\t") and not l.strip().startswith(";"):
            cur[0] = n
            cur[1].append(l.split()[0])
    return [(last, ops) for last, ops in loops.values() if any(o.startswith("v_mfma") for o in ops)]


def count(ops, prefix):
    return sum(1 for o in ops if o.startswith(prefix))


def check_behind_the_loop(fn, last):
    """From the loop's last line to the body's end: an s_barrier between the last MFMA and the first LDS write behind it."""
    tail = [l.split()[0] for l in fn[last + 1:] if l.startswith("\t") and not l.strip().startswith(";")]
    if "s_endpgm" in tail:
        tail = tail[:tail.index("s_endpgm")]
    mf = [n for n, o in enumerate(tail) if o.startswith("v_mfma")]
    after = tail[(mf[-1] + 1) if mf else 0:]
    writes = [n for n, o in enumerate(after) if o.startswith("ds_write")]
    assert writes, "no LDS write (the split-K reduction) behind the loop"
    assert "s_barrier" in after[:writes[0]], "the partial tile goes into the ring without a barrier behind the k-loop"


def test_pair_input_gradient_loop_has_no_barrier(asm):
    fn = function_lines(asm, PAIR)
    loops = [(last, ops) for last, ops in mfma_loops(fn)
             if count(ops, "ds_read_b128") == 2 * D32 and count(ops, "ds_read_b64") == 4 * D32 and count(ops, "ds_read") == 6 * D32]
    assert len(loops) == 1, "the 32x32 input-gradient loop: found %d" % len(loops)
    last, ops = loops[0]
    assert count(ops, "s_barrier") == 0
    assert count(ops, "v_mfma") == 16 * D32
    assert count(ops, "global_load_dwordx4") == LOADS32 * D32
    assert count(ops, "ds_write_b128") == LOADS32 * D32
    check_behind_the_loop(fn, last)


@pytest.mark.parametrize("kernel", sorted(REG16))
def test_16x16_loop_has_no_barrier(asm, kernel):
    fn = function_lines(asm, REG16[kernel])
    loops = mfma_loops(fn)
    assert len(loops) == 1, "one k-loop expected, found %d" % len(loops)
    last, ops = loops[0]
    assert count(ops, "s_barrier") == 0
    assert count(ops, "v_mfma") == 4 * D16
    assert count(ops, "global_load_dwordx4") == LOADS16 * D16
    assert count(ops, "ds_write_b128") == LOADS16 * D16
    check_behind_the_loop(fn, last)
