"""Nothing an earlier call left in the workspace reaches a later result of the supervised step.

The step's panels are sized for max_batch rows and lookahead blocks; a smaller call writes a corner of them and runs whole
padded tiles over the rest.  What keeps the rest out of every sum is code: the zero-rows launch in front of the <= 4-row
GEMV forward, the one-time memset of the seed panels' pad columns, the count of loss partials a small step sums, the row
blocks of a smaller batch lying next to an older batch's at lookahead > 1.  tests/test_gpu_fuzz.py cannot see a slip
there, because its two engines run the same sequence of row counts and so carry the same stale panels.

Here one guarded engine (tests/guards.py, max_batch 130) per lookahead is given a HISTORY through legitimate calls only --
the workspace contract (include/pvae.h, pvae_bind_workspace) forbids writing the buffer, so the library is made to
poison it itself:

  nan_joint / nan_world   one fused training call at 130 rows whose x and y are all NaN: every live entry of every panel,
                          the targets, the draws used and the loss partials then hold NaN
  large_joint             the same with x = y = 1000: finite and large -- a stale NaN that a ReLU mask or a max() swallows
                          would pass the finiteness check, a stale 1e3 still changes the bits
  nan_infer_4 / _33       a rollout forward on NaN observations, fused <= 4-row path and staged path
  nan_prefetch            a train_step_prefetch whose prefetched span is all-NaN dataset rows and is then NOT the next one

Parameters and moments are restored from clones, then the real calls run at 1, 3, 4, 5, 31, 33 and 97 rows in both
phases: forward_backward (gradient stored, and fused Adam), evaluation, train_step, `read` of every intermediate the call
produced, `infer` at 1-4 and 9 rows.  Everything must be finite, bit-equal to a FRESH engine that never saw any history
(one per block, built on a zero-filled workspace), and within the oracle's bounds (losses 1e-5, gradients 1e-4)."""
import functools

import numpy as np
import pytest
import torch

import guards as G
from oracle import refpath as R
from physicsvae_amd import _lib
from physicsvae_amd.engine import Arch, HipEngine, make_step_params
from test_gpu_step_guards import TERMS, Placer, _bits, _nets
from util import max_err_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda"
DB, DA, Z = 23, 7, 5
NETS = dict(te=(129, 2), md=(31, 2), wm=(100, 3))                # odd widths: every panel has pad columns
ARCH = R.make_arch(DB, DA, latent=Z, **NETS)
MAX_ROWS, POOL = 130, 130
ROWS = (1, 3, 4, 5, 31, 33, 97)
INFER_ROWS = (1, 2, 3, 4, 9)
HISTORIES = ("nan_joint", "nan_world", "large_joint", "nan_infer_4", "nan_infer_33", "nan_prefetch")
NAN_ROWS = 40                                                    # the all-NaN episode behind the real dataset rows
_fresh = {}


@functools.lru_cache(maxsize=None)
def _inputs(L):
    """Weights, a pool of windows with its 97 kink-free rows (both phases), and the dataset arrays: the real episodes
    followed by one episode of NaN rows that only the nan_prefetch history ever names."""
    data = R.synth_demo(7, 2, 70 + L, DB, DA, kind="dynamics")
    X, Y = R.build_windows(data, lookahead=L)
    x, y = next(iter(R.make_loader(X, Y, POOL)))
    sd = R.perturb_biases(R.init_state_dict(ARCH, seed=8), seed=9)
    es = R.eps_stream(10, Z)
    eps = torch.stack([es(t, (POOL, Z)) for t in range(L)])
    ok = (R.relu_kink_margin(ARCH, sd, x, y, eps, True) > 4e-6) & (R.relu_kink_margin(ARCH, sd, x, y, eps, False) > 4e-6)
    keep = torch.nonzero(ok)[:, 0]
    assert keep.numel() >= POOL - max(4, POOL // 4) and keep.numel() >= max(ROWS)
    keep = keep[: max(ROWS)]
    states = np.concatenate([np.stack(ep["state_body"]) for ep in data["episodes"]]).astype(np.float32)
    actions = np.concatenate([np.stack(ep["action"]) for ep in data["episodes"]]).astype(np.float32)
    rows, off = [], 0
    for ep in data["episodes"]:
        T = len(ep["time"])
        rows.append(off + np.arange(T - L))
        off += T
    n_real = len(np.concatenate(rows))
    rows.append(off + np.arange(NAN_ROWS - L))
    nan = lambda w: np.full((NAN_ROWS, w), np.nan, dtype=np.float32)     # noqa: E731
    return dict(x=x[keep], y=y[keep], eps=eps[:, keep], sd=sd, n_real=n_real,
                states=torch.from_numpy(np.concatenate([states, nan(DB)])),
                actions=torch.from_numpy(np.concatenate([actions, nan(DA)])),
                window_row=torch.from_numpy(np.concatenate(rows).astype(np.int32)))


@functools.lru_cache(maxsize=None)
def _want(L, world, rows):
    I = _inputs(L)
    e = I["eps"][:, :rows]
    return R.loss_and_grads(ARCH, I["sd"], I["x"][:rows], I["y"][:rows], e if L > 1 else e[0], world)


def _engine(L):
    I = _inputs(L)
    eng = HipEngine(Arch(DB, DA, Z, NETS["te"], NETS["md"], NETS["wm"]), MAX_ROWS, DEV, lookahead=L)
    G.guard_engine(eng)
    views = eng.named_views()
    assert set(views) <= set(I["sd"])
    for k, v in views.items():
        v.copy_(I["sd"][k])
    eng.p0 = eng.params.clone()
    placed, prow = G.poison_row_dataset(I["states"], I["actions"], I["window_row"], device=DEV)
    eng.dataset_guards = [(name, buf, view) + ((prow,) if name == "window_row" else ()) for name, (buf, view) in placed.items()]
    eng.bind_dataset(placed["states"][1], placed["actions"][1], placed["window_row"][1])
    return eng


@functools.lru_cache(maxsize=None)
def _history_engine(L):
    return _engine(L)


def _reset(eng):
    eng.params.copy_(eng.p0)
    eng.grads.zero_()
    eng.exp_avg.zero_()
    eng.exp_avg_sq.zero_()


def _sp(world, rows, t=1):
    c = R.phase_coeffs(world)
    return make_step_params(lr=5e-4, adam_t=(t, t, t), a_rec=c["a_rec_coeff"], kl=c["vae_kl_coeff"], s_rec=c["s_rec_coeff"],
                            cyc=c["vae_cycle_coeff"], global_rows=rows)


def _phase(world):
    return _lib.PHASE_WORLD if world else _lib.PHASE_JOINT


def _make_history(eng, L, kind, world):
    """Dirty the workspace through the library's own launches; parameters and moments are put back afterwards."""
    g = torch.Generator().manual_seed(3)
    if kind in ("nan_joint", "nan_world", "large_joint"):
        fill = 1000.0 if kind == "large_joint" else float("nan")
        hw = kind == "nan_world"
        eng.set_batch(torch.full((MAX_ROWS, L, 2 * DB), fill), torch.full((MAX_ROWS, L, DA), fill))
        loss = eng.forward_backward(_phase(hw), MAX_ROWS, _sp(hw, MAX_ROWS), eps=torch.randn(L, MAX_ROWS, Z, generator=g),
                                    fused_adam=True).cpu()
        assert torch.isnan(loss[0]) or kind == "large_joint"     # (the history did reach the loss partials)
    elif kind in ("nan_infer_4", "nan_infer_33"):
        r = int(kind.rsplit("_", 1)[1])
        eng.infer(torch.full((r, 2 * DB), float("nan")), noise=False)
        # (what comes OUT is NaN on the staged path only: the fused path's ReLU is a max, which drops a NaN operand -- the
        #  observation rows it keeps and the first layers' operands are the NaN this history leaves behind)
        assert torch.isnan(eng.workspace).any()
    else:
        assert kind == "nan_prefetch"
        n_real = _inputs(L)["n_real"]
        loss = eng.train_step(_phase(world), 0, 33, _sp(world, 33), eps=torch.randn(L, 33, Z, generator=g),
                              next_span=(n_real, 33)).cpu()
        assert torch.isfinite(loss).all()                        # (this step's own span is real rows; the NaN span is staged ahead)
    _reset(eng)


def _block(eng, L, world, rows):
    """The real calls of one (phase, row count) -> {name: CPU tensor}."""
    I = _inputs(L)
    P = Placer(eng)
    P.extra += eng.dataset_guards
    phase, sp, nets = _phase(world), _sp(world, rows), _nets(eng, world)
    x_d, y_d = P.put("x", I["x"][:rows].reshape(rows, -1)), P.put("y", I["y"][:rows].reshape(rows, -1))
    e = I["eps"][:, :rows]
    e_d = P.put("eps", e if L > 1 else e[0]) if (not world or L > 1) else None
    lo = P.put("loss_out", torch.zeros(5))
    out = {}
    eng.set_batch(x_d, y_d)
    eng.grads.fill_(float("nan"))
    eng.forward_backward(phase, rows, sp, eps=e_d, fused_adam=False, loss_out=lo)
    out["loss"], out["grads"] = lo.cpu().clone(), eng.segment(eng.grads, nets).cpu().clone()
    out["views"] = {k: v.cpu().clone() for k, v in eng.named_views(eng.grads).items()}
    # every intermediate this call produced (world phase, lookahead 1: the world model alone runs)
    names = ("s2_hat",) if (world and L == 1) else ("mu", "logvar", "z", "eps", "a_hat", "s2_hat")
    for t in range(L):
        for name in names:
            out["read_%s_%d" % (name, t)] = eng.read(name, rows, step=t).cpu()
    eng.set_batch(x_d, y_d)
    eng.forward_backward(phase, rows, sp, eps=e_d, backward=False, loss_out=lo)
    out["eval"] = lo.cpu().clone()
    eng.set_batch(x_d, y_d)
    eng.forward_backward(phase, rows, sp, eps=e_d, fused_adam=True, loss_out=lo)
    out["fused_loss"] = lo.cpu().clone()
    for name, a in (("params", eng.params), ("exp_avg", eng.exp_avg), ("exp_avg_sq", eng.exp_avg_sq)):
        out["fused_" + name] = a.cpu().clone()
    _reset(eng)
    eng.train_step(phase, 3, rows, sp, eps=e_d, loss_out=lo)
    out["train_step_loss"] = lo.cpu().clone()
    for name, a in (("params", eng.params), ("exp_avg", eng.exp_avg)):
        out["train_step_" + name] = a.cpu().clone()
    _reset(eng)
    if world:                                                    # (the rollout forward knows no phase: once per row count)
        g = torch.Generator().manual_seed(rows)
        for r in INFER_ROWS:
            obs, eps_r = P.put("obs", torch.randn(r, 2 * DB, generator=g)), P.put("infer_eps", torch.randn(r, Z, generator=g))
            for noise in (True, False):
                got = eng.infer(obs, eps=eps_r if noise else None, noise=noise)
                for name, v in zip(("a_hat", "s2_hat", "z"), got):
                    out["infer_%d_%s_%s" % (r, "noise" if noise else "mean", name)] = v.cpu().clone()
    P.check("the real calls at %d rows" % rows)
    return out


def _fresh_block(L, world, rows):
    key = (L, world, rows)
    if key not in _fresh:
        eng = _engine(L)                                         # a zero-filled workspace nothing has run on
        _fresh[key] = _block(eng, L, world, rows)
        del eng
    return _fresh[key]


def _check_block(got, want, L, world, rows, what):
    for k, v in got.items():
        if k != "views":
            assert torch.isfinite(v).all(), "%s: %s is not finite" % (what, k)
    assert got.keys() == want.keys()
    for k in want:
        if k != "views":
            assert _bits(want[k], got[k]), "%s: %s differs from the fresh engine's" % (what, k)
    ref = _want(L, world, rows)
    for key in ("loss", "eval", "fused_loss"):
        assert float(got[key][0]) == pytest.approx(float(ref["total"]), rel=1e-5, abs=1e-9), (what, key)
        for i, k in enumerate(TERMS):
            assert float(got[key][1 + i]) == pytest.approx(float(ref[k]), rel=1e-5, abs=1e-9), (what, key, k)
    for k, gr in ref["grads"].items():
        assert max_err_scaled(got["views"][k], gr) < 1e-4, (what, k)


@pytest.mark.parametrize("world", [True, False], ids=["world", "joint"])
@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("kind", HISTORIES)
def test_a_history_reaches_no_later_result(kind, L, world):
    eng = _history_engine(L)
    for rows in ROWS:
        want = _fresh_block(L, world, rows)
        _make_history(eng, L, kind, world)
        got = _block(eng, L, world, rows)
        _check_block(got, want, L, world, rows, "%s, lookahead %d, %s phase, %d rows" % (kind, L, "world" if world else "joint", rows))


def test_the_histories_do_leave_their_mark_next_to_the_live_rows():
    """The premise, so that the equalities above are not vacuous: after a history and a 5-row real call the panels still
    hold the history beyond the live rows.  Read back through the API at more rows than the call had, the decoder's output
    panel is zero there on a fresh engine and holds the 1000-input batch's actions after `large_joint`; after `nan_joint`
    the input panels' rows past the live block are still NaN."""
    I = _inputs(1)

    def five_rows(eng):
        eng.set_batch(I["x"][:5], I["y"][:5])
        eng.forward_backward(_lib.PHASE_JOINT, 5, _sp(False, 5), eps=I["eps"][0, :5], fused_adam=False)
        return eng.read("a_hat", 64).cpu()
    fresh = five_rows(_engine(1))
    eng = _history_engine(1)
    _make_history(eng, 1, "large_joint", False)
    a = five_rows(eng)
    assert _bits(a[:5], fresh[:5]) and float(fresh[32:].abs().max()) == 0.0
    assert torch.isfinite(a[32:]).all() and bool((a[32:] != 0).all())
    _make_history(eng, 1, "nan_joint", False)
    assert _bits(five_rows(eng)[:5], fresh[:5])
    assert int(torch.isnan(eng.workspace).sum()) >= (MAX_ROWS - 32) * 2 * DB
    _reset(eng)
