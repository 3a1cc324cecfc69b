"""The compute waves' k-loop of the plain 32x32 forward / input-gradient kernels (pvae_gemm_ws.h, splitk_ws_superstep_body) in the
emitted gfx950 assembly, beside test_loader_isa_cpu.py: a compute wave opens every super-step with MFMAs -- at least two
v_mfma stand between each s_barrier of its loop and the first ds_read behind it (the next tile's fragment reads go between
the MFMAs, not in front of them), every barrier is preceded by the `s_waitcnt lgkmcnt(0)` that retires the fragment reads
(round 5's race fix), and a super-step holds both tiles' reads (no branch inside it for hipcc to sink reads behind).
pvae_net.hip is compiled with the flags of physicsvae_amd/build.py.  No GPU needed; skipped where there is no hipcc."""
import pytest

from isa import KERNELS, asm, function_lines, inner_loops  # noqa: F401  (asm: the fixture)

PLAIN = {"ws<P_ROW, EpiBiasAct>": 4, "ws<P_COL, EpiMask>": 6}      # ds_read instructions per fragment set


@pytest.mark.parametrize("kernel", sorted(PLAIN))
def test_compute_loop_opens_each_superstep_with_mfmas(asm, kernel):
    loops = [body for body in inner_loops(function_lines(asm, KERNELS[kernel])).values()
             if any(i.split()[0].startswith("v_mfma") for i in body)]
    assert len(loops) == 1, "one compute loop expected, found %d" % len(loops)
    body = loops[0]
    ops = [i.split()[0] for i in body]
    barriers = [n for n, op in enumerate(ops) if op == "s_barrier"]
    assert len(barriers) == 1, "one barrier per super-step expected, found %d" % len(barriers)
    assert sum(op.startswith("v_mfma") for op in ops) == 32, "a super-step is two k-tiles of 16 MFMAs"
    assert sum(op.startswith("ds_read") for op in ops) == 2 * PLAIN[kernel], "a super-step reads two tiles' fragments"
    for n in barriers:
        rest = ops[n + 1:] + ops[:n]                      # (the loop wraps: what follows the barrier in execution order)
        mfmas = 0
        for op in rest:
            if op.startswith("ds_read"):
                break
            mfmas += op.startswith("v_mfma")
        assert mfmas >= 2, "%d v_mfma between an s_barrier and the first ds_read behind it" % mfmas
        # the wait that retires the previous super-step's reads sits between the last read and the barrier
        retired = False
        for line in reversed(body[n + 1:] + body[:n]):
            if line.split()[0].startswith("ds_read"):
                break
            retired = retired or line.split() == ["s_waitcnt", "lgkmcnt(0)"]
        assert retired, "no s_waitcnt lgkmcnt(0) between the last read and the barrier"
