"""Self-test of tests/guards.py on CPU tensors: a planted one-element write is found in the front and in the back guard, a
clean buffer passes, the alignment arithmetic holds for odd sizes, and an index fetched from outside window_row gathers
the poison row.  A guard check that found nothing would make every GPU test built on it vacuous, so the detection is
also shown to matter: with the check made a no-op the same planted writes go unnoticed."""
import math

import pytest
import torch

import guards as G


def test_poison_is_a_quiet_nan_with_its_payload():
    p = G.poison(3)
    assert p.dtype == torch.float32 and torch.isnan(p).all() and torch.isnan(G.POISON)
    assert p.view(torch.int32).tolist() == [G.POISON_BITS] * 3 and int(G.POISON.view(torch.int32)) == G.POISON_BITS
    assert G.POISON_BITS & 0x7FC00000 == 0x7FC00000              # exponent all ones, quiet bit set
    assert math.isnan(float((p + 1.0)[0]))                       # a consumed load shows in the result


@pytest.mark.parametrize("shape", [(1,), (5,), (7, 3), (63,), (64,), (65,), (130, 17), (3, 5, 7)])
@pytest.mark.parametrize("guard", [1, 63, 64, 65, 1000])
def test_clean_buffers_pass_and_views_start_on_256_bytes(shape, guard):
    buf, view = G.guarded(shape, guard=guard, fill=1.5)
    off, n = G._span(buf, view)
    assert off % 64 == 0 and off >= guard and buf.numel() - off - n == off     # (256 bytes; both guards as wide)
    assert (view.data_ptr() - buf.data_ptr()) % 256 == 0
    assert tuple(view.shape) == tuple(shape) and bool((view == 1.5).all())
    assert G.guards_intact(buf, view) and G.guard_damage(buf, view) == []
    view.mul_(2.0)                                               # writes inside the view are nobody's business
    assert G.guards_intact(buf, view)


@pytest.mark.parametrize("where", ["front_first", "front_last", "back_first", "back_last"])
@pytest.mark.parametrize("value", [0.0, 1.0, float("nan")])
def test_a_planted_one_element_write_is_found(where, value, monkeypatch):
    buf, view = G.guarded((7, 3), guard=64, fill=0.0)
    off, n = G._span(buf, view)
    at = {"front_first": 0, "front_last": off - 1, "back_first": off + n, "back_last": buf.numel() - 1}[where]
    buf[at] = value                                              # (the default NaN differs from POISON in its payload)
    assert not G.guards_intact(buf, view)
    side, idx, bits = G.guard_damage(buf, view)[0]
    assert side == where.split("_")[0]
    assert idx == (at if side == "front" else at - off - n)
    assert bits == int(torch.tensor(value).view(torch.int32))
    # the detection is what finds it: with the comparison made a no-op the same buffer passes
    monkeypatch.setattr(G, "_differing", lambda part, pattern: torch.zeros(0, dtype=torch.int64))
    assert G.guards_intact(buf, view)


def test_without_the_planted_write_nothing_is_reported():
    buf, view = G.guarded((7, 3), guard=64, fill=None)
    assert torch.isnan(view).all()                               # fill=None: the view is poison too
    view.zero_()
    assert G.guards_intact(buf, view)


def test_index_buffers_take_a_guard_value():
    buf, view = G.guarded((10,), dtype=torch.int32, guard=3, fill=0, guard_value=41)
    assert G.guards_intact(buf, view, 41) and buf[0] == 41 and buf[-1] == 41
    buf[-1] = 40
    assert G.guard_damage(buf, view, 41) == [("back", 63, 40)]
    with pytest.raises(AssertionError):
        G.guarded((10,), dtype=torch.int32)


@pytest.mark.parametrize("lookahead", [1, 2, 3])
@pytest.mark.parametrize("Db,Da", [(5, 1), (23, 7), (197, 45)])
def test_an_out_of_range_window_reads_the_poison_row(Db, Da, lookahead):
    n_rows = 37
    g = torch.Generator().manual_seed(Db)
    states, actions = torch.randn(n_rows, Db, generator=g), torch.randn(n_rows, Da, generator=g)
    nxt = torch.randn(n_rows, Db, generator=g)
    wr = torch.arange(n_rows - lookahead, dtype=torch.int32)
    ds, prow = G.poison_row_dataset(states, actions, wr, next_states=nxt)
    assert prow == n_rows and int(wr.max()) + lookahead < prow   # no real window touches the poison row
    wbuf, wview = ds["window_row"]
    assert torch.equal(wview, wr) and G.guards_intact(wbuf, wview, prow)
    off, n = G._span(wbuf, wview)
    for outside in (off - 1, off + n, 0, wbuf.numel() - 1):      # a window index fetched from outside the table ...
        row = int(wbuf[outside])
        for name in ("states", "actions", "next_states"):
            buf, view = ds[name]
            assert torch.equal(view, {"states": states, "actions": actions, "next_states": nxt}[name])
            for step in range(lookahead + 1):                    # ... gathers NaN for s_t .. s_{t+L}, a_t ..: mapped memory
                got = G.gather_rows(buf, view, row + step)
                assert got.numel() == view.shape[1] and torch.isnan(got).all()
                assert (got.view(torch.int32) == G.POISON_BITS).all()
            assert G.guards_intact(buf, view)
    # 16-byte chunks of the last real row reach at most 12 bytes past the array: poison, inside the allocation
    buf, view = ds["states"]
    off, n = G._span(buf, view.reshape(-1))
    assert torch.isnan(buf[off + n: off + n + 3]).all() and buf.numel() - off - n >= 4 * Db


def test_strided_blocks_have_poison_on_every_side():
    buf, view = G.strided_block(5, 64, 192, guard_rows=2, left=64)
    assert view.stride(0) == 192 and tuple(view.shape) == (5, 64) and torch.isnan(view).all()
    view.zero_()
    assert G.surroundings_intact(buf, view) and bool((view == 0).all())
    for r, c in ((1, 70), (2, 63), (2, 128), (7, 64), (6, 191)):   # above, left, right, below, right of the last row
        b2, v2 = G.strided_block(5, 64, 192, guard_rows=2, left=64)
        v2.zero_()
        b2.view(9, 192)[r, c] = 0.0
        assert not G.surroundings_intact(b2, v2), (r, c)


def test_pad_mask_is_the_arena_minus_the_named_views():
    class Eng:                                                   # the two members pad_mask reads, over a 2-layer arena
        arena_floats = 64 * 64 + 64
        params = torch.zeros(arena_floats)

        def named_views(self, arena):
            return {"w": arena[: 64 * 64].view(64, 64)[:5, 3:10], "b": arena[64 * 64: 64 * 64 + 5]}
    m = G.pad_mask(Eng())
    assert int((~m).sum()) == 5 * 7 + 5 and not m[3] and m[2] and m[10] and not m[64 * 64 + 4] and m[64 * 64 + 5]
