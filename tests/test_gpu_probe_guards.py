"""The contraction bodies alone, inside poison: every operand of a `gemm_probe` call (kinds 0 forward, 1 input gradient,
2 weight gradient), its bias or mask and its output are views inside buffers that hold tests/guards.py's POISON everywhere
else.  Two placements:

  dense    the operand is dense, 64 poison rows directly before and after it;
  strided  the operand is a column block of a wider poisoned matrix (leading dimension = width rounded up to 64, plus 128:
           a multiple of 64 floats, as every panel and weight block of the step has), 64 poison columns to its left, the
           rest to its right, 64 poison rows above and below.

The output starts as poison and must come back finite (every element written, no poison consumed), every float outside
the views keeps its bits, and the result meets the kernel bound of test_gpu_parity.py -- 2e-6 sqrt(K) of the tensor's max
against a float64 contraction.  The shapes take each body once: 16x16 tiles, the wave-specialised 32x32 body at the
contraction lengths at which its prologue's tiles 1-4 are present or absent, 64x32, 64x64, the two row counts that are a
multiple of 32 but not of 64 at widths that would otherwise take 64-row tiles, and both weight-gradient geometries at row
counts that are no multiple of 64.  The geometry each shape is meant to take is asserted with tests/tile_rules.py.

Every body takes a leading dimension larger than its width: `gemm_probe` passes lda / ldb / ldc / ld_mask through
GemmArgs as the step's call sites do, so the strided placement runs for every shape."""
import pytest
import torch

import guards as G
import tile_rules as T
from physicsvae_amd.engine import gemm_probe
from util import max_err_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD_ROWS = 64

# (geometry, output rows, output columns, k-tiles of 64)
FWD = [("16x16", 32, 32, 1)] + [("32x32", 512, 256, nk) for nk in (1, 2, 3, 5, 7)] + \
      [("64x32", 512, 1024, nk) for nk in (1, 3)] + [("64x64", 1024, 1024, nk) for nk in (1, 3)] + \
      [("32x32", 544, 1024, 2), ("32x32", 1056, 1024, 2)]
WGRAD = [(1, 64, 64, 64)] + [(0, m, n, k) for m in (32, 96, 544) for n in (64, 128, 320) for k in (64, 128, 320)]


def _place(t, placement):
    """(buffer, view holding `t`) on the GPU; a [n] vector is dense in both placements (it has no leading dimension)."""
    t = t.to(DEV)
    if t.dim() == 1 or placement == "dense":
        w = t.shape[-1] if t.dim() == 2 else 1
        buf, view = G.guarded(t.shape, guard=GUARD_ROWS * max(w, 64), fill=None, device=DEV)
    else:
        ld = (t.shape[1] + 63) // 64 * 64 + 128
        buf, view = G.strided_block(t.shape[0], t.shape[1], ld, guard_rows=GUARD_ROWS, left=64, device=DEV)
        assert view.stride(0) == ld and ld > t.shape[1] and ld % 64 == 0
    view.copy_(t)
    return buf, view


def _out(rows, cols, placement):
    buf, view = _place(torch.zeros(rows, cols), placement)
    view.copy_(G.poison(rows * cols, DEV).view(rows, cols))
    return buf, view


def _intact(placed, what):
    torch.cuda.synchronize()
    for name, (buf, view) in placed.items():
        ok = G.guards_intact(buf, view) if view.is_contiguous() else G.surroundings_intact(buf, view)
        assert ok, "%s: a float outside %s changed" % (what, name)


@pytest.mark.parametrize("placement", ["dense", "strided"])
@pytest.mark.parametrize("geom,m,cols,nk", FWD, ids=lambda v: str(v))
def test_forward_body_inside_poison(geom, m, cols, nk, placement):
    k = 64 * nk
    assert T.plan_tiles("forward", m, cols)[0] == geom
    g = torch.Generator().manual_seed(11 + m + cols + k)
    x, w, b = torch.randn(m, k, generator=g), torch.randn(cols, k, generator=g), torch.randn(cols, generator=g)
    want = (x.double() @ w.double().t() + b.double()).clamp_min(0)
    p = {"x": _place(x, placement), "w": _place(w, placement), "bias": _place(b, placement), "out": _out(m, cols, placement)}
    gemm_probe(0, p["x"][1], p["w"][1], p["out"][1], bias_or_mask=p["bias"][1], relu=True, m=m, n=cols, k=k)
    _intact(p, "forward %s" % geom)
    out = p["out"][1].cpu()
    assert torch.isfinite(out).all()
    err, tol = max_err_scaled(out, want), 2e-6 * (k ** 0.5)
    print("forward %s %dx%d K %d %s: %.3g (bound %.3g)" % (geom, m, cols, k, placement, err, tol))
    assert err < tol


@pytest.mark.parametrize("placement", ["dense", "strided"])
@pytest.mark.parametrize("geom,m,cols,nk", FWD, ids=lambda v: str(v))
def test_input_gradient_body_inside_poison(geom, m, cols, nk, placement):
    n = 64 * nk                                                  # (the contraction runs over the layer's outputs)
    assert T.plan_tiles("dgrad", m, cols)[0] == geom
    g = torch.Generator().manual_seed(13 + m + cols + n)
    dz, w, act = torch.randn(m, n, generator=g), torch.randn(n, cols, generator=g), torch.randn(m, cols, generator=g)
    want = (dz.double() @ w.double()) * (act > 0)
    p = {"dz": _place(dz, placement), "w": _place(w, placement), "mask": _place(act, placement), "out": _out(m, cols, placement)}
    gemm_probe(1, p["dz"][1], p["w"][1], p["out"][1], bias_or_mask=p["mask"][1], m=m, n=n, k=cols)
    _intact(p, "input gradient %s" % geom)
    out = p["out"][1].cpu()
    assert torch.isfinite(out).all()
    err, tol = max_err_scaled(out, want), 2e-6 * (n ** 0.5)
    print("input gradient %s %dx%d N %d %s: %.3g (bound %.3g)" % (geom, m, cols, n, placement, err, tol))
    assert err < tol


@pytest.mark.parametrize("placement", ["dense", "strided"])
@pytest.mark.parametrize("t32,m,n,k", WGRAD, ids=lambda v: str(v))
def test_weight_gradient_body_inside_poison(t32, m, n, k, placement):
    assert T.plan_wgrad(n, k, m)[0] == t32                       # 32x32 tiles need a multiple of 64 rows; the rest is 64x64
    g = torch.Generator().manual_seed(17 + m + n + k)
    dz, x = torch.randn(m, n, generator=g), torch.randn(m, k, generator=g)
    want = dz.double().t() @ x.double()
    p = {"dz": _place(dz, placement), "x": _place(x, placement), "out": _out(n, k, placement)}
    gemm_probe(2, p["dz"][1], p["x"][1], p["out"][1], m=m, n=n, k=k)
    _intact(p, "weight gradient %s" % ("32x32" if t32 else "64x64"))
    out = p["out"][1].cpu()
    assert torch.isfinite(out).all()
    err, tol = max_err_scaled(out, want), 2e-6 * (m ** 0.5)
    print("weight gradient %d rows %dx%d %s: %.3g (bound %.3g)" % (m, n, k, placement, err, tol))
    assert err < tol
