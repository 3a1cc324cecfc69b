"""The prologue of the plain dense 32x32 forward / input-gradient body (pvae_gemm_ws.h, splitk_ws_superstep_body): k-tiles 0, 1 and 2
are fetched by all eight waves (six LDS-DMAs each, counted waits), the loaders add tile 3 in front of barrier #0 and tile 4
behind it, and the compute waves certify their shares of tiles 1 and 2 in front of their loop.  Contraction lengths of nk = 1, 2, 3, 4, 5,
6, 8, 9 and 16 k-tiles take every guard of that prologue (tiles 1 ... 4 present or absent), the first loop iteration with
and without tiles 5 and 6, and the first wrap of the six-slot ring -- through gemm_probe, forward with bias + ReLU and input
gradient with mask, at 512 rows x 256 columns (128 workgroups, the smallest grid the planner gives this body).

Every length runs once as it is and once in a child process with PVAE_KROT=1, where each workgroup starts at a rotated k-tile
and the prologue's tile walk wraps.  Outputs are pre-filled with NaN and must come back finite; each is held against a
float64 contraction at the kernel tolerance of test_gpu_parity.py (2e-6 sqrt(K) of the tensor's max).  The un-rotated
512 x 1024 run on 32x32 tiles (PVAE_WS64=0) must also equal the untouched 64x32 body's (PVAE_WS64=1) to the bit."""
import os
import subprocess
import sys

import pytest
import torch

from util import max_err_scaled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ROWS = 512
KS = tuple(64 * nk for nk in (1, 2, 3, 4, 5, 6, 8, 9, 16))
# child processes (the switches are read when the library loads): name -> (environment, columns)
RUNS = {"plain": ({}, 256), "krot": ({"PVAE_KROT": "1"}, 256), "ws32": ({"PVAE_WS64": "0"}, 1024), "ws64": ({"PVAE_WS64": "1"}, 1024)}

INPUTS = r'''
import torch
def inputs(m, cols, k):
    g = torch.Generator().manual_seed(700001 * cols + k)
    x, w, b = torch.randn(m, k, generator=g), torch.randn(cols, k, generator=g), torch.randn(cols, generator=g)
    dz, wd, act = torch.randn(m, k, generator=g), torch.randn(k, cols, generator=g), torch.randn(m, cols, generator=g)
    return x, w, b, dz, wd, act
'''
exec(INPUTS)

CHILD = INPUTS + r'''
import sys
sys.path.insert(0, %r)
from physicsvae_amd.engine import gemm_probe
m, cols, outs = %d, int(sys.argv[2]), {}
for k in %r:
    x, w, b, dz, wd, act = (t.cuda() for t in inputs(m, cols, k))
    o = torch.full((m, cols), float("nan"), device="cuda")
    gemm_probe(0, x, w, o, bias_or_mask=b, relu=True, m=m, n=cols, k=k)
    d = torch.full((m, cols), float("nan"), device="cuda")
    gemm_probe(1, dz, wd, d, bias_or_mask=act, m=m, n=k, k=cols)
    outs[k] = (o.cpu(), d.cpu())
torch.save(outs, sys.argv[1])
''' % (ROOT, ROWS, KS)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{run name: {k: (forward, input gradient)}}, one child process per run."""
    tmp = tmp_path_factory.mktemp("ws_prologue")
    out = {}
    for name, (env, cols) in RUNS.items():
        f = str(tmp / ("%s.pt" % name))
        clean = {k: v for k, v in os.environ.items() if k not in ("PVAE_KROT", "PVAE_WS64")}
        subprocess.run([sys.executable, "-c", CHILD, f, str(cols)], check=True, env=dict(clean, **env), timeout=300)
        out[name] = torch.load(f)
    return out


@pytest.fixture(scope="module")
def wanted():
    """{(cols, k): float64 (forward, input gradient)}, computed once per shape."""
    cache = {}

    def get(cols, k):
        if (cols, k) not in cache:
            x, w, b, dz, wd, act = inputs(ROWS, cols, k)                  # noqa: F821  (defined by INPUTS)
            cache[(cols, k)] = ((x.double() @ w.double().t() + b.double()).clamp_min(0), (dz.double() @ wd.double()) * (act > 0))
        return cache[(cols, k)]
    return get


@pytest.mark.parametrize("k", KS)
def test_prologue_edges_against_float64(runs, wanted, k):
    tol = 2e-6 * (k ** 0.5)
    for name, (_, cols) in RUNS.items():
        want_f, want_d = wanted(cols, k)
        o, d = runs[name][k]
        assert torch.isfinite(o).all() and torch.isfinite(d).all(), name
        ef, ed = max_err_scaled(o, want_f), max_err_scaled(d, want_d)
        print("%s cols %d K %d: forward %.3g, input gradient %.3g (bound %.3g)" % (name, cols, k, ef, ed, tol))
        assert ef < tol and ed < tol, name


@pytest.mark.parametrize("k", KS)
def test_prologue_32x32_equals_64x32_body_bit_for_bit(runs, k):
    assert torch.equal(runs["ws32"][k][0], runs["ws64"][k][0])
    assert torch.equal(runs["ws32"][k][1], runs["ws64"][k][1])
