"""CPU-side checks of the autograd surface (physicsvae_amd/autograd.py): the two backward entry points are declared,
exported and bound, chunking covers every row once, and the Functions refuse a double backward."""
import os
import re

import pytest
import torch

from physicsvae_amd import _lib
from physicsvae_amd import autograd as AG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_backward_entry_points_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pvae.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("pvae_net_backward", "pvae_reparam_backward"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.pvae_abi_version() == 12
    # argument checks run before anything touches a device
    assert lib.pvae_net_backward(None, 0, None, 1, None, None, None, 0, None) < 0
    assert b"null ctx" in lib.pvae_last_error()
    assert lib.pvae_reparam_backward(None, None, None, None, 1, 0, None, None) < 0


def test_chunks_cover_every_row_once():
    for rows, mb in ((1, 256), (256, 256), (257, 256), (600, 256), (500, 64)):
        spans = AG.chunks(rows, mb)
        assert spans[0][0] == 0 and spans[-1][1] == rows
        assert all(hi - lo <= mb and hi > lo for lo, hi in spans)
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))


class _StubEngine:
    """An engine whose one stack is y = x @ W^T (CPU, torch): enough to drive HipNet's plumbing without a GPU."""
    device = torch.device("cpu")
    max_batch = 4

    def __init__(self, w):
        self.w = w
        self.segments = {0: (0, w.numel())}
        self.layers = [dict(net=0, w_offset=0, b_offset=w.numel(), n_out_pad=w.shape[0], ld=w.shape[1], n_out=w.shape[0],
                            col0=0, n_in=w.shape[1])]

    def net_forward(self, net, x):
        return x @ self.w.detach().t()

    def net_backward(self, net, x, dy, want_dx, grad=None, accumulate=False):
        if grad is not None:
            g = (dy.t() @ x).reshape(-1)
            grad[: g.numel()] = grad[: g.numel()] + g if accumulate else g
        return dy @ self.w.detach() if want_dx else None


def test_hipnet_chunks_its_backward_and_rejects_double_backward():
    w = torch.randn(3, 5, requires_grad=True)
    eng = _StubEngine(w)
    eng.segments = {0: (0, w.numel())}
    x = torch.randn(10, 5, requires_grad=True)                  # 3 chunks of <= 4 rows
    y = AG.HipNet.apply(eng, 0, x, w)
    dy = torch.randn(10, 3, requires_grad=True)                # (a graph through the backward itself: what double backward needs)
    gx, gw = torch.autograd.grad(y, (x, w), dy, create_graph=True)
    assert torch.allclose(gx, dy.detach() @ w.detach(), atol=1e-5) and torch.allclose(gw, dy.detach().t() @ x.detach(), atol=1e-5)
    with pytest.raises(RuntimeError, match="differentiate twice"):
        gx.sum().backward()
