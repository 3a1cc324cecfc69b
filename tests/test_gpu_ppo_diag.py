"""Learner diagnostics from inside the fused PPO steps (include/pvae.h "Learner diagnostics") on the GPU: (1) the loss head
alone against float64 on every loss-head case, past the wave cap and on targets far from zero; (2) the fused step of a
stack set on all 24 step cases -- the bits of the stand-alone head on the forward's outputs, the float64 twin, and every
existing output bit-identical with and without a bound buffer; (3) the gradient norm against the float64 norm of the
gradient the device holds, with grad_scale and frozen stacks; (4) `ppo_sgd` row by row, the refusal of a short buffer, guard
bands; (5) the same for PhysicsVAE on three step cases; (6) the workers' exchange, world 1 and two processes on one GPU.
The cases, oracles and bounds: tests/ppo_diag_cases.py."""
import math
import os
import subprocess
import sys

import pytest
import torch

import fc_cases as F
import ppo_diag_cases as D
import ppo_diag_dp_worker as DW
import ppo_dp_worker as W
import vae_ppo_cases as V
from guards import guarded, guards_intact
from physicsvae_amd import ppo as P
from physicsvae_amd.engine import make_ppo_batch, ppo_loss, ppo_loss_diag
from physicsvae_amd.parallel import PPODataParallel
from test_gpu_fc_shapes import bound_engine, dirty, head_setup, stack_span, step_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def nan_rows(n):
    return torch.full((n, P.PPO_DIAG), NAN, device=DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------
# 1. the head alone
# ---------------------------------------------------------------------------------------
def head_diag_run(k, kind, idx, with_index, cur, dbatch, params, what):
    rows = idx.numel()
    if kind == "state_dependent":
        ls_dev = cur["log_std"][idx].to(DEV)
    else:
        ls_dev = cur["log_std"][0].to(DEV).reshape(1, k).expand(rows, k)             # row stride 0
    index = idx.to(DEV, torch.int32) if with_index else None
    args = (cur["mean"][idx].to(DEV), ls_dev, cur["value"][idx].to(DEV), dbatch, params, index)
    plain = ppo_loss(*args)
    got = ppo_loss_diag(*args, diag_out=nan_rows(1)[0])
    assert all(same_bits(a, b) for a, b in zip(plain, got[:4])), (what, "stats or gradients moved")
    diag = got[4].cpu()
    assert same_bits(diag, ppo_loss_diag(*args)[4].cpu())                            # fixed summation order
    want = D.head_diag(k, kind, idx)
    assert float(diag[4:].abs().max()) == 0.0                                        # entries 4..7 are written, as 0
    D.check_diag(diag, want, D.HEAD_BOUNDS(want), rows, what)


@pytest.mark.parametrize("k,kind", [key for key in F.HEAD_SEEDS if key[0] != F.WAVE_CAP_K])
def test_head_diagnostics_match_float64(k, kind):
    cur, dbatch, params = head_setup(k, kind)
    for rows, with_index, idx in F.head_runs(k, kind):
        D.assert_kink_free(k, kind, idx)
        head_diag_run(k, kind, idx, with_index, cur, dbatch, params, (k, kind, rows, with_index))


def test_head_diagnostics_past_the_wave_cap():
    k, kind = F.WAVE_CAP_K, F.WAVE_CAP_KIND
    cur, dbatch, params = head_setup(k, kind)
    for rows, with_index, idx in F.head_runs(k, kind):
        head_diag_run(k, kind, idx, with_index, cur, dbatch, params, (k, kind, rows, with_index))
    for rows in F.WAVE_CAP_ROWS:
        head_diag_run(k, kind, F.wave_cap_index(rows), True, cur, dbatch, params, (k, kind, rows, "gathered"))


@pytest.mark.parametrize("rows", [2, 33, 256])
def test_head_targets_far_from_zero(rows):
    mean, ls, value, cols, cfg = D.offset_case(rows)
    k = mean.shape[1]
    want = P.learner_diag_torch(mean.double(), ls.double(), value.double(), cfg=cfg, **{key: v.double() for key, v in cols.items()})
    dbatch = make_ppo_batch({key: v.to(DEV) for key, v in cols.items()}, DEV, k)
    params = P.PPOConfig(**F.LOSS).params("constant")
    got = ppo_loss_diag(mean.to(DEV), ls.to(DEV).contiguous(), value.to(DEV), dbatch, params)[4].cpu().double()
    raw = D.raw_sums_explained_var(value, cols["value_targets"])
    print(rows, "vf_explained_var", float(got[0]), "float64", float(want[0]), "raw float32 sums would give", raw)
    assert float(want[0]) > -1.0 and abs(float(got[0]) - float(want[0])) <= D.EV_BOUND
    assert abs(raw - float(want[0])) > 10 * D.EV_BOUND                              # (the case tells the two apart)


# ---------------------------------------------------------------------------------------
# 2. / 3. the fused step of a stack set, and the gradient norm
# ---------------------------------------------------------------------------------------
def mask_of(c):
    """Seeds < 4 (unequal depths): a proper subset of the stacks is trained; 0: all."""
    S = len(c.stacks)
    return 1 + c.seed % ((1 << S) - 2) if c.seed < 4 else 0


def fc_state(eng):
    out = {"params": eng.params, "m": eng.ppo_m, "v": eng.ppo_v}
    if eng.ls is not None:
        out["log_std"] = eng.ls
    if eng.ppo_ls_m is not None:
        out.update(ls_m=eng.ppo_ls_m, ls_v=eng.ppo_ls_v)
    return {key: v.clone() for key, v in out.items()}


def moved(a, b):
    return [key for key in a if not same_bits(a[key], b[key])]


@pytest.mark.parametrize("seed,kind", F.PPO_CASE_IDS)
def test_fused_step_diagnostics(seed, kind):
    c = F.ppo_step_case(seed, kind)
    mask, S = mask_of(c), len(c.stacks)
    trained = [s for s in range(S) if not mask or (mask >> s) & 1]
    p1 = step_params(c, 1, mask)
    a, batch_a, index = bound_engine(c)
    b, batch_b, _ = bound_engine(c)
    for eng in (a, b):
        dirty(eng)
    # without a buffer, and with one: every existing output keeps its bits, one launch more
    stats_a = a.ppo_step(batch_a, p1, c.first, c.rows, index)
    launches = a.ppo_launches()
    row = nan_rows(1)
    b.ppo_diag(row)
    x = c.used["obs"].to(DEV)
    outs = b.forward(x)
    ls = (F.LS_BASE + outs[2]) if kind == "state_dependent" else b.ls.reshape(1, c.k).expand(c.rows, c.k)
    sub = index[c.first: c.first + c.rows].contiguous() if index is not None else None
    head = ppo_loss_diag(outs[0], ls, outs[1][:, 0], batch_b, p1, sub)[4]
    stats_b = b.ppo_step(batch_b, p1, c.first, c.rows, index)
    assert b.ppo_launches() == launches + 1
    assert same_bits(stats_a, stats_b) and not moved(fc_state(a), fc_state(b)), moved(fc_state(a), fc_state(b))
    for s in trained:
        for off, n in stack_span(a, s):
            assert same_bits(a.ppo_grad[off: off + n], b.ppo_grad[off: off + n])
    diag = row[0].cpu()
    # entries 0..3: the bits of the stand-alone head on the forward's outputs over the same rows
    assert same_bits(diag[:4], head[:4].cpu()), (c.name, diag.tolist(), head.tolist())
    assert float(diag[5:].abs().max()) == 0.0 and math.isfinite(float(diag[4]))
    want, bounds, dev = D.step_diag_want(seed, kind)
    print(c.name, "rows", c.rows, "mask", mask, "float32 twin off by", dev.tolist(), "bounds", bounds)
    D.check_diag(diag, want, bounds, c.rows, c.name)
    # unbound again: the launch count and the bits of a second step are the plain ones
    b.ppo_diag(None)
    p2 = step_params(c, 2, mask)
    assert same_bits(a.ppo_step(batch_a, p2, c.first, c.rows, index), b.ppo_step(batch_b, p2, c.first, c.rows, index))
    assert b.ppo_launches() == launches and not moved(fc_state(a), fc_state(b))
    assert same_bits(row[0].cpu(), diag)                                             # nothing wrote the row after the unbind


@pytest.mark.parametrize("seed,kind", F.PPO_CASE_IDS)
def test_gradient_norm(seed, kind):
    c = F.ppo_step_case(seed, kind)
    mask, S = mask_of(c), len(c.stacks)
    trained = [s for s in range(S) if not mask or (mask >> s) & 1]
    train_ls = kind == "state_independent"
    a, batch_a, index = bound_engine(c)
    b, batch_b, _ = bound_engine(c)
    row_a, row_b = nan_rows(1), nan_rows(1)
    a.ppo_diag(row_a)
    b.ppo_diag(row_b)
    dirty(a)
    a.ppo_grad.fill_(1e6)                                                            # a frozen stack's part must not show
    p1 = step_params(c, 1, mask)
    _, ls_grad = a.ppo_grad_step(batch_a, p1, c.first, c.rows, index)
    launches_grad = a.ppo_launches()
    first_half = row_a[0].cpu().clone()
    assert math.isnan(float(first_half[4])) and float(first_half[5:].abs().max()) == 0.0      # the first half: 0..3 (+ reserved)
    grads = [a.ppo_grad[off: off + n] for s in trained for off, n in stack_span(a, s)]
    for s in range(S):
        if s not in trained:
            assert all(float((a.ppo_grad[off: off + n] - 1e6).abs().max()) == 0.0 for off, n in stack_span(a, s))
    norm = float(P.grad_gnorm_torch(grads + ([ls_grad] if train_ls else [])))
    a.ppo_apply(p1, 1.0, ls_grad if train_ls else None)
    assert a.ppo_launches() == 2
    got = row_a[0].cpu().clone()
    print(c.name, "mask", mask, "grad_gnorm", float(got[4]), "float64", norm)
    assert abs(float(got[4]) - norm) <= D.GNORM_RTOL * norm and norm > 0
    assert same_bits(got[:4], first_half[:4])                                        # the second half: entry 4 alone
    # the fused step from the same state: the same row, bit for bit, one launch more than the plain step
    dirty(b)
    b.ppo_step(batch_b, p1, c.first, c.rows, index)
    assert same_bits(row_b[0].cpu(), got), (row_b[0].tolist(), got.tolist())
    assert b.ppo_launches() == launches_grad - (2 if train_ls else 1) + 2
    # grad_scale 0.5 on the gradient the arena still holds
    a.ppo_apply(step_params(c, 2, mask), 0.5, ls_grad if train_ls else None)
    half = float(row_a[0, 4])
    assert abs(half - 0.5 * norm) <= D.GNORM_RTOL * 0.5 * norm


# ---------------------------------------------------------------------------------------
# 4. ppo_sgd
# ---------------------------------------------------------------------------------------
def test_sgd_rows_equal_the_steps_one_by_one():
    c = F.ppo_step_case(2, "state_independent")
    assert c.rows == 33 and c.index is None
    a, batch_a, _ = bound_engine(c)
    b, batch_b, _ = bound_engine(c)
    n, mb, passes = c.rows, 16, 2                                                    # minibatches of 16, 16 and 1 rows
    perm = torch.stack([torch.randperm(n, generator=torch.Generator().manual_seed(70 + p)) for p in range(passes)]).to(torch.int32).to(DEV)
    # a buffer of 5 rows is refused with nothing launched
    before = fc_state(a)
    a.ppo_diag(nan_rows(5))
    with pytest.raises(RuntimeError, match="6 steps"):
        a.ppo_sgd(batch_a, step_params(c, 1), mb, passes, perm=perm)
    torch.cuda.synchronize()
    assert not moved(before, fc_state(a))
    # 9 rows between guard bands: rows 6..8 and the bands stay
    buf, rows9 = guarded((9, P.PPO_DIAG), fill=7.0, device=DEV)
    a.ppo_diag(rows9)
    stats = a.ppo_sgd(batch_a, step_params(c, 1), mb, passes, perm=perm)
    assert stats.shape == (6, 5)
    one = nan_rows(1)
    b.ppo_diag(one)
    t = 0
    for p in range(passes):
        for first in range(0, n, mb):
            t += 1
            r = min(mb, n - first)
            st = b.ppo_step(batch_b, step_params(c, t), first, r, perm[p])
            assert same_bits(st, stats[t - 1]) and same_bits(one[0], rows9[t - 1]), (p, first, one[0].tolist(), rows9[t - 1].tolist())
            if r == 1:
                assert float(rows9[t - 1, 0]) == -1.0                               # a one-row step: exactly -1
    assert t == 6 and not moved(fc_state(a), fc_state(b))
    assert float((rows9[6:] - 7.0).abs().max()) == 0.0 and guards_intact(buf, rows9)
    assert bool(torch.isfinite(rows9[:6]).all())


def test_learn_fills_the_rows_and_refuses_a_wrong_buffer():
    case = dict(model="fcnn", kind="state_independent", n_rows=(131,), minibatch=64, passes=2)
    cfg = W.config(case)
    a, b = W.make_model(case), W.make_model(case)
    (batch,), _ = W.make_batches(case, a)
    dbatch = W.on_dev(batch)
    want = a.ppo_learn(dbatch, cfg)
    diag = P.diag_buffer(131, cfg, DEV)
    assert tuple(diag.shape) == (6, P.PPO_DIAG)
    got = b.ppo_learn(dbatch, cfg, diag_out=diag)
    assert same_bits(got, want) and W.same_state(W.state(a), W.state(b))
    assert bool(torch.isfinite(diag).all()) and float(diag[:, 4].min()) > 0 and float(diag[:, 5:].abs().max()) == 0.0
    info = P.learner_info(got, diag, cfg)
    assert info["grad_gnorm"] == pytest.approx(float(diag[:, 4].double().mean())) and -1.0 <= info["vf_explained_var"] <= 1.0
    for bad in (diag[:5], diag.cpu(), diag.double()):
        with pytest.raises(ValueError, match="diag_out must be"):
            b.ppo_learn(dbatch, cfg, diag_out=bad)
    # the buffer was unbound when the call returned: the next call is the plain one
    assert same_bits(a.ppo_learn(dbatch, cfg), b.ppo_learn(dbatch, cfg)) and a.engine.ppo_launches() == b.engine.ppo_launches()
    # rows the caller had bound itself are left alone by the call and bound again behind it
    own = nan_rows(1)
    b.engine.ppo_diag(own)
    b.ppo_learn(dbatch, cfg, diag_out=diag)
    assert b.engine.ppo_diag_bound()[0] is own and bool(torch.isnan(own).all())
    b.engine.ppo_diag(None)
    assert b.engine.ppo_diag_bound() is None


# ---------------------------------------------------------------------------------------
# 5. PhysicsVAE
# ---------------------------------------------------------------------------------------
VAE_CASES = ("no_prior_odd", "masks_6", "subsets_body_task_5")       # no prior | zero-mean prior, frozen encoder | an input subset


def vae_diag(c, dtype):
    params = V.leaves(c, dtype, 0)
    used = {key: t.to(dtype) for key, t in c.used.items()}
    with torch.no_grad():
        mean, ls, value, _, _ = V.forward(c, params, c.ls_vec.to(dtype), used["obs"], c.eps.to(dtype))
        return P.learner_diag_torch(mean, ls, value, cfg=c.cfg, **{key: used[key] for key in D.BATCH_KEYS})


@pytest.mark.parametrize("name", VAE_CASES)
def test_physics_vae_diagnostics(name):
    import test_gpu_ppo_vae_shapes as TS
    c = V.case(name)
    assert (name != "no_prior_odd" or not c.prior) and (name != "masks_6" or (c.prior and not c.mask & 1))
    train_ls = c.log_std_type == "state_independent"
    (ma, a, va), (mb, b, vb) = TS.setup(c), TS.setup(c)
    cols = a.ppo_batch({k: v.to(DEV) for k, v in c.batch.items()})
    index = c.index.to(DEV) if c.index is not None else None
    eps = c.eps.to(DEV)
    kw = dict(eps=eps, noise=c.noise, offset=1)
    p1 = TS.params_of(c, ma, 1)
    stats_a = a.ppo_step(cols, p1, c.first, c.rows, index, **kw)
    launches = a.ppo_launches()
    assert launches == TS.launches(c)
    # the two halves with a bound row: entries 0..3, then entry 4 against the float64 norm of what the arenas hold
    row_b = nan_rows(1)
    b.ppo_diag(row_b)
    # entries 0..3 are to be the stand-alone head's bits on the forward's outputs over the same rows: the evaluate pass
    # (same weights, same draws) gives that forward
    used = {k: v.to(DEV) for k, v in c.used.items()}
    fwd = b.ppo_evaluate({"obs": used["obs"], "actions": used["actions"]}, TS.CFG.gae_params(c.log_std_type), eps=eps, noise=c.noise)
    ls = mb._als.on_device(b.device).reshape(1, c.Da).expand(c.rows, c.Da)            # (a constant vector lives on the host)
    dense = make_ppo_batch({k: v for k, v in used.items() if k != "obs"}, DEV, c.Da)
    head = ppo_loss_diag(fwd["old_dist"][:, :c.Da], ls, fwd["vf_preds"], dense, p1)[4].cpu()
    grad = TS.buffers(mb, "grad")
    frozen = [k for k in grad if not c.mask & {n: bit for bit, n in zip((1, 2, 4), V.NETS)}[k.split(".")[0]]]
    for k in frozen:
        grad[k].fill_(1e6)
    st, ls_grad = b.ppo_grad_step(cols, p1, c.first, c.rows, index, **kw)
    assert same_bits(st, stats_a)
    first_half = row_b[0].cpu().clone()
    trained = [g for k, g in TS.buffers(mb, "grad").items() if k not in frozen]
    norm = float(P.grad_gnorm_torch(trained + ([ls_grad] if train_ls else [])))
    b.ppo_apply(p1, 1.0, ls_grad if train_ls else None)
    halves = row_b[0].cpu().clone()
    assert same_bits(halves[:4], first_half[:4]) and math.isnan(float(first_half[4]))
    print(name, "rows", c.rows, "mask", c.mask, "grad_gnorm", float(halves[4]), "float64", norm)
    assert abs(float(halves[4]) - norm) <= D.GNORM_RTOL * norm and norm > 0
    assert same_bits(halves[:4], head[:4]), (name, halves.tolist(), head.tolist())
    assert not TS.same_state(TS.state(ma), TS.state(mb)), TS.same_state(TS.state(ma), TS.state(mb))
    # grad_scale 0.5 on the gradient the arenas still hold: entry 4 alone moves, to half the norm
    b.ppo_apply(TS.params_of(c, mb, 2), 0.5, ls_grad if train_ls else None)
    scaled = row_b[0].cpu().clone()
    print(name, "grad_scale 0.5: grad_gnorm", float(scaled[4]), "float64", 0.5 * norm)
    assert abs(float(scaled[4]) - 0.5 * norm) <= D.GNORM_RTOL * 0.5 * norm and same_bits(scaled[:4], first_half[:4])
    # the fused step with a bound row on a third module: the same row, the same state, one launch more
    mc, e, vc = TS.setup(c)
    row_c = nan_rows(1)
    e.ppo_diag(row_c)
    assert same_bits(e.ppo_step(cols, p1, c.first, c.rows, index, **kw), stats_a)
    assert e.ppo_launches() == launches + 1
    assert not TS.same_state(TS.state(ma), TS.state(mc))
    diag = row_c[0].cpu()
    assert same_bits(diag, halves), (diag.tolist(), halves.tolist())
    assert float(diag[5:].abs().max()) == 0.0
    d32, d64 = vae_diag(c, torch.float32).double(), vae_diag(c, torch.float64)
    dev = (d32 - d64).abs()
    bounds = (max(D.EV_BOUND, 4 * float(dev[0])), D.FRAC_BOUND, D.FRAC_BOUND, max(D.RATIO_RTOL * float(d64[3]), 4 * float(dev[3])))
    D.check_diag(diag, d64, bounds, c.rows, name)
    e.ppo_diag(None)
    p2 = TS.params_of(c, ma, 2)
    kw2 = dict(kw, offset=2)
    assert same_bits(a.ppo_step(cols, p2, c.first, c.rows, index, **kw2), e.ppo_step(cols, p2, c.first, c.rows, index, **kw2))
    assert e.ppo_launches() == launches and not TS.same_state(TS.state(ma), TS.state(mc))


@pytest.mark.parametrize("name", VAE_CASES)
def test_physics_vae_sgd_rows_equal_the_steps_one_by_one(name):
    import test_gpu_ppo_vae_shapes as TS
    c = V.case(name)
    (ma, a, _), (mb, b, _) = TS.setup(c), TS.setup(c)
    g = torch.Generator().manual_seed(c.seed + 11)
    n, rows, passes = c.rows, (c.rows - 1) // 2, 2                                   # 33 rows: 16, 16 and 1; 5 rows: 2, 2 and 1
    assert n in (33, 5) and 2 * rows + 1 == n
    batch = {k: v.to(DEV) for k, v in c.used.items()}
    perm = torch.stack([torch.randperm(n, generator=g) for _ in range(passes)]).to(torch.int32).to(DEV)
    leps = torch.randn(6, rows, c.Z, generator=g).to(DEV)
    cols_a, cols_b = a.ppo_batch(batch), b.ppo_batch(batch)
    before = TS.state(ma)
    a.ppo_diag(nan_rows(5))
    with pytest.raises(RuntimeError, match="6 steps"):
        a.ppo_sgd(cols_a, TS.params_of(c, ma, 1), rows, passes, perm, eps=leps, noise=c.noise, offset=1)
    torch.cuda.synchronize()
    assert not TS.same_state(before, TS.state(ma))                                   # refused with nothing launched
    buf, rows9 = guarded((9, P.PPO_DIAG), fill=7.0, device=DEV)
    a.ppo_diag(rows9)
    stats = a.ppo_sgd(cols_a, TS.params_of(c, ma, 1), rows, passes, perm, eps=leps, noise=c.noise, offset=1)
    one = nan_rows(1)
    b.ppo_diag(one)
    i = 0
    for p in range(passes):
        for first in range(0, n, rows):
            r = min(rows, n - first)
            st = b.ppo_step(cols_b, TS.params_of(c, mb, 1 + i), first, r, perm[p].contiguous(), eps=leps[i, :r].contiguous(),
                            noise=c.noise, offset=1 + i)
            assert same_bits(st, stats[i]) and same_bits(one[0], rows9[i]), (i, one[0].tolist(), rows9[i].tolist())
            if r == 1:
                assert float(rows9[i, 0]) == -1.0
            i += 1
    assert i == 6 and not TS.same_state(TS.state(ma), TS.state(mb))
    assert float((rows9[6:] - 7.0).abs().max()) == 0.0 and guards_intact(buf, rows9)


# ---------------------------------------------------------------------------------------
# 6. workers
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["fcnn", "vae"])
def test_world_one_exchange_gives_the_plain_rows(model):
    case = dict(model=model, kind="state_independent", n_rows=(131,), minibatch=64, passes=1)
    cfg = W.config(case)
    a, b = W.make_model(case), W.make_model(case)
    (batch,), (eps,) = W.make_batches(case, a)
    dbatch = W.on_dev(batch)
    kw = {"eps": eps[0]} if eps is not None else {}
    da, db = P.diag_buffer(131, cfg, DEV), P.diag_buffer(131, cfg, DEV)
    want = a.ppo_learn(dbatch, cfg, diag_out=da, **kw)
    dp = PPODataParallel(0, 1, transport="p2p")
    dp.attach(b)
    got = b.ppo_learn(dbatch, cfg, dp=dp, diag_out=db, **kw)
    assert same_bits(got, want) and same_bits(da, db) and W.same_state(W.state(a), W.state(b))
    assert dp.timeouts(b) == 0 and float(da[:, 4].min()) > 0
    dp.detach(b)
    # the "torch" transport's two halves fill the same rows with the same bits
    c2 = W.make_model(case)
    dc = P.diag_buffer(131, cfg, DEV)
    got = c2.ppo_learn(dbatch, cfg, dp=PPODataParallel(0, 1, transport="torch"), diag_out=dc, **kw)
    assert same_bits(got, want) and same_bits(dc, da)


def run_workers(tmp_path, name, tag, port, **extra_env):
    """Two workers on cuda:0, each under its own time limit; the first non-zero status ends the test."""
    world = len(DW.CASES[name]["n_rows"])
    out = str(tmp_path / tag)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world),
               HSA_ENABLE_IPC_MODE_LEGACY="0", **extra_env)
    procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "ppo_diag_dp_worker.py"),
                               ROOT, out, name], env=dict(env, RANK=str(r), LOCAL_RANK="0"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = [p.communicate()[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [torch.load(out + ".%d" % r) for r in range(world)]


@pytest.mark.parametrize("name,port", [("fc", 29621), ("vae", 29623)])
def test_two_workers_report_the_norm_of_the_averaged_gradient(tmp_path, name, port):
    p2p = run_workers(tmp_path, name, name + "_p2p", port)
    tor = run_workers(tmp_path, name, name + "_torch", port + 1, PPO_DP_TRANSPORT="torch")
    norms, own = DW.emulate_norms(DW.CASES[name])
    for res in (p2p, tor):
        assert same_bits(res[0]["diag"][:, 4], res[1]["diag"][:, 4])                 # both ranks: the same norm, bit for bit
        assert res[0]["timeouts"] == 0 and res[1]["timeouts"] == 0
        for r in range(2):
            assert tuple(res[r]["diag"].shape) == (3, P.PPO_DIAG)
            assert same_bits(res[r]["diag"][:, :4], own[r])                          # entries 0..3 stay each worker's own
    assert same_bits(p2p[0]["diag"], tor[0]["diag"]) and same_bits(p2p[1]["diag"], tor[1]["diag"])
    assert not same_bits(p2p[0]["diag"][:, :4], p2p[1]["diag"][:, :4])
    for i, norm in enumerate(norms):
        got = float(p2p[0]["diag"][i, 4])
        print(name, "step", i, "grad_gnorm", got, "float64 norm of the averaged gradient", norm)
        assert abs(got - norm) <= D.GNORM_RTOL * norm and norm > 0
