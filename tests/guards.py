"""Guard bands for the supervised step's caller-owned buffers (tests/test_gpu_step_guards.py, test_gpu_step_history.py,
test_gpu_probe_guards.py; self-test: test_guards_cpu.py).

The kernels of the step run whole padded tiles without bounds checks over buffers the caller sizes with
pvae_arena_floats / pvae_workspace_bytes.  A buffer built here is a view in the middle of a larger allocation whose
two ends hold POISON, a quiet NaN with a payload no arithmetic produces.  The ends are compared as int32 bit patterns,
so ONE pattern catches both kinds of error: a store outside the view changes bits of a guard, and a load outside the
view that still reaches a result makes that result NaN.  Index buffers (window_row) cannot hold a NaN: their guards hold
the index of a dedicated dataset row that is poison itself and that no real window touches (poison_row_dataset), so an
index fetched from outside the table gathers NaN -- from mapped memory."""
import ctypes as C

import torch

POISON_BITS = 0x7FC12345                                       # quiet NaN, payload 0x012345
ALIGN = 64                                                     # floats: 256 bytes, what pvae_bind_workspace asks for


def poison(n, device="cpu"):
    return torch.full((int(n),), POISON_BITS, dtype=torch.int32, device=device).view(torch.float32)


POISON = poison(1)[0]                                          # the 0-dim float32 tensor; compare through .view(torch.int32)


def _round_up(n, q=ALIGN):
    return (int(n) + q - 1) // q * q


def guarded(shape, dtype=torch.float32, guard=ALIGN, fill=0.0, device="cpu", guard_value=None):
    """(whole buffer, view of `shape` in its middle) with at least `guard` elements of poison on both sides.  The guard is
    rounded up to 64 elements and the buffer's base is 256-byte aligned (checked), so the view starts 256-byte aligned
    whatever its size.  float32: the guards hold POISON_BITS; int32: `guard_value` (required).  `fill` None: the view
    keeps the poison too (an output every element of which must be written)."""
    shape = (shape,) if isinstance(shape, int) else tuple(int(s) for s in shape)
    n = 1
    for s in shape:
        n *= s
    g = _round_up(max(int(guard), 1))
    assert dtype in (torch.float32, torch.int32)
    if dtype == torch.int32:
        assert guard_value is not None, "an index buffer's guards hold the poison row's index"
        buf = torch.full((n + 2 * g,), int(guard_value), dtype=torch.int32, device=device)
    else:
        buf = poison(n + 2 * g, device)
    assert buf.data_ptr() % 256 == 0 or buf.device.type == "cpu"
    view = buf[g: g + n].view(shape)
    if fill is not None:
        view.fill_(fill)
    return buf, view


def _span(buf, view):
    """(first element, element count) of `view` inside the flat `buf`; the view must be dense."""
    assert view.is_contiguous() and buf.dim() == 1 and buf.dtype == view.dtype
    off = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    assert 0 < off and off + view.numel() < buf.numel(), "the view has no guard on one side"
    return int(off), int(view.numel())


def _differing(part, pattern):
    """Indices of the elements of the int32 tensor `part` that are not `pattern` (the one comparison every check makes)."""
    return torch.nonzero(part != int(pattern))[:, 0]


def guard_damage(buf, view, pattern=None):
    """[(side, element offset inside that guard, int32 bits found)] of every guard element that no longer holds the
    pattern -- at most 8 per side.  Offsets of the back guard count from the first element past the view."""
    off, n = _span(buf, view)
    if pattern is None:
        assert buf.dtype == torch.float32, "pass the guard value of an index buffer"
        pattern = POISON_BITS
    bits = buf.view(torch.int32)
    out = []
    for side, part in (("front", bits[:off]), ("back", bits[off + n:])):
        bad = _differing(part, pattern)[:8].tolist()
        out += [(side, int(i), int(part[i])) for i in bad]
    return out


def guards_intact(buf, view, pattern=None):
    return not guard_damage(buf, view, pattern)


def strided_block(rows, width, ld, guard_rows=1, left=ALIGN, device="cpu"):
    """(buffer, [rows, width] view with row stride `ld`) -- a column block of a wider poisoned matrix: `left` poison
    columns before it, ld - left - width after it, `guard_rows` whole poison rows above and below."""
    assert ld % ALIGN == 0 and left % ALIGN == 0 and left + width <= ld
    buf = poison((rows + 2 * guard_rows) * ld, device)
    view = buf.view(rows + 2 * guard_rows, ld)[guard_rows: guard_rows + rows, left: left + width]
    return buf, view


def surroundings_intact(buf, view):
    """Everything of `buf` outside the (possibly strided, 2-D) `view` still holds the poison pattern."""
    keep = view.clone()
    view.copy_(poison(view.numel(), view.device).view(view.shape))
    ok = _differing(buf.view(torch.int32), POISON_BITS).numel() == 0
    view.copy_(keep)
    return ok


def poison_row_dataset(states, actions, window_row, next_states=None, guard=ALIGN, device="cpu"):
    """The dataset arrays inside guard bands.  The states / actions guards are poison and at least four rows wide, so the
    row with index n_rows -- the first row of the back guard -- is the dedicated poison row, and so are its successors up to
    lookahead 3; window_row's guards hold that index.  Returns ({name: (buffer, view)}, poison row index).  The arrays to
    bind are the views: n_rows rows, the poison row not among them, and guard_damage still checks its bits."""
    out = {}
    n_rows = int(states.shape[0])
    for name, a in (("states", states), ("actions", actions), ("next_states", next_states)):
        if a is None:
            continue
        a = torch.as_tensor(a, dtype=torch.float32)
        w = int(a.shape[1])
        g = _round_up(max(guard, 4 * w))                       # the poison row, its successors up to lookahead 3
        buf, view = guarded(a.shape, guard=g, device=device)
        view.copy_(a)
        out[name] = (buf, view)
    wr = torch.as_tensor(window_row, dtype=torch.int32)
    buf, view = guarded(wr.shape, dtype=torch.int32, guard=guard, device=device, guard_value=n_rows)
    view.copy_(wr)
    out["window_row"] = (buf, view)
    return out, n_rows


def gather_rows(states_buf, states_view, index):
    """Row `index` of the array as an out-of-range gather sees it: address arithmetic from the view's first element."""
    off, _ = _span(states_buf, states_view.reshape(-1))
    w = states_view.shape[1]
    return states_buf[off + int(index) * w: off + (int(index) + 1) * w]


def widest_padded_row(eng):
    return max(max(l["ld"], l["n_out_pad"]) for l in eng.layers)


def guard_engine(eng, joint_s_rec=False, direct=False, guard_rows=64, workspace_shift=0):
    """Move a bare HipEngine's four arenas and its workspace into guarded buffers and bind them again.  `eng` must not come
    from a trainer (whose nn.Parameters are views of the ORIGINAL arena).  The workspace view is zero-filled, bound with
    exactly pvae_workspace_bytes bytes and starts 256-byte aligned; every guard is `guard_rows` (>= 64) rows of the
    architecture's widest padded row, so a 64-row tile that overruns a 32-row-padded panel lands inside it.  Context
    options are applied after the re-bind.  `workspace_shift` (floats, a multiple of 64, test of the test only): bind the
    workspace that far behind the view's start, in-bounds of the guarded buffer -- its tail then overlaps the back guard."""
    from physicsvae_amd import _lib
    assert guard_rows >= 64 and eng.ctx is not None
    g = guard_rows * widest_padded_row(eng)
    eng.guards = {}
    for name in ("params", "grads", "exp_avg", "exp_avg_sq"):
        buf, view = guarded(eng.arena_floats, guard=g, device=eng.device)
        view.copy_(getattr(eng, name))
        setattr(eng, name, view)
        eng.guards[name] = (buf, view)
    nbytes = int(eng.lib.pvae_workspace_bytes(C.byref(eng.cfg)))
    assert nbytes > 0 and nbytes % 256 == 0
    buf, view = guarded(nbytes // 4, guard=g, fill=0.0, device=eng.device)
    assert view.data_ptr() % 256 == 0
    eng.workspace = view
    eng.guards["workspace"] = (buf, view)
    buf, view = guarded(5, device=eng.device)
    eng._loss_scratch = view
    eng.guards["loss_scratch"] = (buf, view)
    _lib.check(eng.lib.pvae_bind_arenas(eng.ctx, eng.params.data_ptr(), eng.grads.data_ptr(), eng.exp_avg.data_ptr(),
                                        eng.exp_avg_sq.data_ptr()), "pvae_bind_arenas")
    assert workspace_shift % ALIGN == 0 and 0 <= workspace_shift <= g
    _lib.check(eng.lib.pvae_bind_workspace(eng.ctx, eng.workspace.data_ptr() + 4 * workspace_shift, nbytes), "pvae_bind_workspace")
    _lib.apply_context_options(eng.lib, eng.ctx)
    if joint_s_rec:
        eng.set_joint_s_rec(True)
    if direct:
        eng.set_direct(True)
    return eng


def check_engine_guards(eng, what, extra=()):
    """Every guard of every buffer of a guarded engine (and of `extra` = [(name, buffer, view[, pattern])]) is intact;
    `what` names the entry point that ran last."""
    torch.cuda.synchronize(eng.device)
    for name, (buf, view) in eng.guards.items():
        bad = guard_damage(buf, view)
        assert not bad, "%s broke the guard of %s: (side, offset, bits) %s" % (what, name, bad)
    for item in extra:
        name, buf, view = item[:3]
        bad = guard_damage(buf, view, item[3] if len(item) > 3 else None)
        assert not bad, "%s broke the guard of %s: (side, offset, bits) %s" % (what, name, bad)


def pad_mask(eng):
    """bool [arena_floats]: True at the pad entries -- every arena element outside the union of named_views."""
    marks = torch.zeros(eng.arena_floats, dtype=torch.float32, device=eng.params.device)
    for v in eng.named_views(marks).values():
        v.fill_(1.0)
    return marks == 0
