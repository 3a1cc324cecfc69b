"""The epilogue of the 64x64 weight-gradient body (pvae_gemm_wgrad.h, wgrad_reg_body) in the emitted gfx950 assembly of
gemm_wgrad_reg_kernel<EpiGradStore>: the tile's four global stores come behind the last barrier of the kernel and behind
four ds_read_b128 (the tile returns from LDS as whole rows) with no MFMA between them, the kernel has exactly one barrier
more than the build with the old epilogue (-DPVAE_WGRAD_EPI_DIRECT), and no more registers.  pvae_probe.hip is compiled
with the flags of physicsvae_amd/build.py.  No GPU needed; skipped where there is no hipcc."""
import re

import pytest

from isa import assembly, function_lines

KERNEL = r"_ZN4pvae\d+gemm_wgrad_reg_kernelINS_12EpiGradStoreELi0EEE"


@pytest.fixture(scope="module")
def builds():
    """{"rows" / "direct": (instruction mnemonics of the kernel, its .vgpr_count)}"""
    out = {}
    for name, flags in (("rows", ()), ("direct", ("-DPVAE_WGRAD_EPI_DIRECT",))):
        lines = assembly("pvae_probe.hip", flags)
        text = "\n".join(lines)
        fn = function_lines(lines, KERNEL)
        ops = [l.split()[0] for l in fn if l.startswith("\t") and not l.strip().startswith(";")]
        m = re.search(r"\.name:\s+%s\w*\n(?:.*\n){0,40}?\s+\.vgpr_count:\s+(\d+)" % KERNEL, text)
        assert m, "no metadata for the kernel"
        out[name] = (ops, int(m.group(1)))
    return out


def test_tile_leaves_behind_lds_reads_with_one_more_barrier_and_no_more_registers(builds):
    (rows, vg_rows), (direct, vg_direct) = builds["rows"], builds["direct"]
    assert rows.count("s_barrier") == direct.count("s_barrier") + 1
    assert vg_rows <= vg_direct, (vg_rows, vg_direct)
    last = len(rows) - 1 - rows[::-1].index("s_barrier")
    tail = rows[last + 1:]
    stores = [n for n, op in enumerate(tail) if op == "global_store_dwordx4"]
    reads = [n for n, op in enumerate(tail) if op == "ds_read_b128"]
    assert len(stores) == 4 and len(reads) == 4, (len(stores), len(reads))
    assert all(r < s for r, s in zip(reads, stores)), (reads, stores)       # the i-th store follows the i-th read
    assert not any(op.startswith("v_mfma") for op in tail)
