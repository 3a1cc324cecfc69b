"""Every edge of the plain 32x32 forward / input-gradient k-loop (splitk_ws_superstep_body: six-slot ring, super-steps of two k-tiles
per workgroup barrier, a loader wave's four DMAs of a tile behind one M0 write, the compute waves' fragment reads between
the MFMAs): contraction lengths of nk = 1 ... 7 and 13 k-tiles -- every branch of the loaders' prologue (issue(2..4)
present or absent), odd and even tails of the super-step, and the first wrap of the ring (nk >= 7) -- through gemm_probe,
forward with bias + ReLU and input gradient with mask.

512 rows x 256 columns is 128 workgroups of 32x32, the smallest grid the planner still gives this body (and it gives it
whatever PVAE_WS64 says); 512 x 1024 is the smallest it hands to the untouched 64x32 body (splitk_ws64_body) unless
PVAE_WS64=0 forces 32x32 tiles, which makes that body an independent bit-for-bit witness of the loop.  Both shapes run in
two child processes (the switch is read when the library loads) and every output must be equal to the bit; each is also
held against a float64 contraction at the kernel tolerance of test_gpu_parity.py (2e-6 sqrt(K) of the tensor's max), so
that two wrong bodies cannot agree.  Outputs are pre-filled with NaN and must come back finite."""
import os
import subprocess
import sys

import pytest
import torch

from util import max_err_scaled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ROWS = 512
COLS = (256, 1024)
KS = (64, 128, 192, 256, 320, 384, 448, 832)

INPUTS = r'''
import torch
def inputs(m, cols, k):
    g = torch.Generator().manual_seed(100003 * cols + k)
    x, w, b = torch.randn(m, k, generator=g), torch.randn(cols, k, generator=g), torch.randn(cols, generator=g)
    dz, wd, act = torch.randn(m, k, generator=g), torch.randn(k, cols, generator=g), torch.randn(m, cols, generator=g)
    return x, w, b, dz, wd, act
'''
exec(INPUTS)

CHILD = INPUTS + r'''
import sys
sys.path.insert(0, %r)
from physicsvae_amd.engine import gemm_probe
m, outs = %d, {}
for cols in %r:
    for k in %r:
        x, w, b, dz, wd, act = (t.cuda() for t in inputs(m, cols, k))
        o = torch.full((m, cols), float("nan"), device="cuda")
        gemm_probe(0, x, w, o, bias_or_mask=b, relu=True, m=m, n=cols, k=k)
        d = torch.full((m, cols), float("nan"), device="cuda")
        gemm_probe(1, dz, wd, d, bias_or_mask=act, m=m, n=k, k=cols)
        outs[(cols, k)] = (o.cpu(), d.cpu())
torch.save(outs, sys.argv[1])
''' % (ROOT, ROWS, COLS, KS)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{PVAE_WS64 mode: {(cols, k): (forward, input gradient)}}, one child process per mode."""
    tmp = tmp_path_factory.mktemp("ws_edges")
    out = {}
    for mode in ("0", "1"):
        f = str(tmp / ("out%s.pt" % mode))
        subprocess.run([sys.executable, "-c", CHILD, f], check=True, env=dict(os.environ, PVAE_WS64=mode), timeout=300)
        out[mode] = torch.load(f)
    return out


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("cols", COLS)
def test_superstep_edges_bit_for_bit_and_against_float64(runs, cols, k):
    x, w, b, dz, wd, act = inputs(ROWS, cols, k)                         # noqa: F821  (defined by INPUTS)
    want_f = (x.double() @ w.double().t() + b.double()).clamp_min(0)
    want_d = (dz.double() @ wd.double()) * (act > 0)
    tol = 2e-6 * (k ** 0.5)
    for mode in ("0", "1"):
        o, d = runs[mode][(cols, k)]
        assert torch.isfinite(o).all() and torch.isfinite(d).all()
        ef, ed = max_err_scaled(o, want_f), max_err_scaled(d, want_d)
        print("cols %d K %d PVAE_WS64=%s: forward %.3g, input gradient %.3g (bound %.3g)" % (cols, k, mode, ef, ed, tol))
        assert ef < tol and ed < tol
    assert torch.equal(runs["0"][(cols, k)][0], runs["1"][(cols, k)][0])
    assert torch.equal(runs["0"][(cols, k)][1], runs["1"][(cols, k)][1])
