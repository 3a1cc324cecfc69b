"""The fused PPO learner step on the GPU (include/pvae.h "PPO learner step"; physicsvae_amd/ppo.py, fcnn.ppo_learn): the
loss head against the float64 torch restatement, one step and five steps against a torch twin (nn.Linear stacks +
ppo_loss_torch + torch.optim.Adam) from identical weights, the SGD loop against the same steps issued one by one, the
fused step's gradient arena against forward + HipPPOLoss + backward(), launch counts, stale buffers, a frozen stack, and
that nothing else moved.  Bounds are the suite's standing ones (tests/test_gpu_fcnn.py): outputs / stats of the head 1e-5,
gradients 1e-4 (max_err_scaled), per-step loss rel 2e-4, parameters after five steps 2e-3."""
import math

import pytest
import torch

from physicsvae_amd import ppo as P
from physicsvae_amd.engine import make_ppo_batch, ppo_loss
from ppo_cases import KINK, coverage, make_case
from test_gpu_fcnn import Twin, eng_pad_max, policy
from util import max_err_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("constant", "state_independent", "state_dependent")
OBS, NUM_OUTPUTS, K = 722, 108, 54
HEAD_SEEDS = {"constant": 3, "state_independent": 3, "state_dependent": 30}   # chosen so that the coverage assertions hold
IMITATION = dict(clip_param=0.2, kl_coeff=0.0, vf_clip_param=1000.0, lr=2e-5, sgd_minibatch_size=500, num_sgd_iter=20)
SECOND = dict(clip_param=0.2, kl_coeff=0.3, entropy_coeff=0.01, vf_clip_param=0.7, vf_loss_coeff=0.5, lr=1e-4,
              sgd_minibatch_size=500, num_sgd_iter=3)
# parameters after a few steps against the twin's, and Adam's moments (m, v): see test_one_step_and_five_steps_match_the_twin
PARAM_BOUND, MOMENT_BOUNDS = 2e-3, (2e-4, 4e-4)


# ---------------------------------------------------------------------------------------
# the head alone
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_head_matches_the_float64_restatement(kind):
    cur64, batch64, cfg = make_case(500, K, HEAD_SEEDS[kind], kind=kind, vf_clip_param=0.7, kl_coeff=0.3, entropy_coeff=0.01,
                                    vf_loss_coeff=0.5)
    # the kernel's inputs are float32: the oracle reads the same rounded values, in float64
    cur = {k: v.float() for k, v in cur64.items()}
    batch = {k: v.float() for k, v in batch64.items()}
    cov = coverage(cur, batch, cfg)
    print(kind, cov)
    assert cov["above"] >= 0.10 and cov["below"] >= 0.10 and cov["zero_grad_rows"] >= 0.10
    assert cov["vclip_active"] >= 0.10 and cov["kink"] > KINK
    params = P.PPOConfig(**{k: getattr(cfg, k) for k in ("clip_param", "vf_clip_param", "vf_loss_coeff", "kl_coeff",
                                                          "entropy_coeff")}).params(kind)
    dbatch = make_ppo_batch({k: v.to(DEV) for k, v in batch.items()}, DEV, K)
    gen = torch.Generator().manual_seed(5)
    for rows in (1, 5, 33, 500):
        for with_index in (False, True):
            idx = torch.randperm(500, generator=gen)[:rows] if with_index else torch.arange(rows)
            mean = cur["mean"][idx].double().requires_grad_(True)
            value = cur["value"][idx].double().requires_grad_(True)
            if kind == "state_dependent":
                leaf = cur["log_std"][idx].double().requires_grad_(True)
                ls64, ls_dev = leaf, cur["log_std"][idx].to(DEV)
            else:
                leaf = cur["log_std"][0].double().requires_grad_(True)
                ls64 = leaf.reshape(1, K).expand(rows, K)
                ls_dev = cur["log_std"][0].to(DEV).reshape(1, K).expand(rows, K)         # row stride 0
            total, stats = P.ppo_loss_torch(mean, ls64, value, cfg=cfg, **{k: v[idx].double() for k, v in batch.items()})
            total.backward()
            index = idx.to(DEV, torch.int32) if with_index else None
            args = (cur["mean"][idx].to(DEV), ls_dev, cur["value"][idx].to(DEV), dbatch, params, index)
            got = ppo_loss(*args)
            again = ppo_loss(*args)
            assert all(torch.equal(a, b) for a, b in zip(got, again))                   # fixed summation order
            g_stats, d_mean, d_ls, d_value = (t.cpu() for t in got)
            e = [max_err_scaled(g_stats, stats.detach()), max_err_scaled(d_mean, mean.grad), max_err_scaled(d_value, value.grad)]
            want_ls = leaf.grad if kind == "state_dependent" else leaf.grad
            got_ls = d_ls if kind == "state_dependent" else d_ls.double().sum(0)
            e.append(max_err_scaled(got_ls, want_ls))
            print(kind, rows, with_index, "stats %.3g d_mean %.3g d_value %.3g d_log_std %.3g" % tuple(e))
            assert e[0] < 1e-5 and e[1] < 1e-4 and e[2] < 1e-4 and e[3] < 1e-4
            check_stats(g_stats, stats.detach(), 1e-5, (kind, rows, with_index))
            assert bool(torch.isfinite(d_ls).all())


# ---------------------------------------------------------------------------------------
# the fused step against a torch twin
# ---------------------------------------------------------------------------------------
def make(kind, max_batch=512, seed=21):
    torch.manual_seed(seed)
    cmc = {"log_std_type": kind, "sample_std": 0.3}
    m = policy(cmc, obs=OBS, num_outputs=NUM_OUTPUTS, max_batch=max_batch)
    with torch.no_grad():                        # biases off zero
        for k, p in m.named_parameters():
            if k.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(3)).to(DEV))
    return m, cmc


def copy_of(m, cmc, max_batch=512):
    m2 = policy(cmc, obs=OBS, num_outputs=NUM_OUTPUTS, max_batch=max_batch)
    with torch.no_grad():
        m2.engine.params.copy_(m.engine.params)
        if cmc["log_std_type"] == "state_independent":
            m2._policy_fn._model[-1].log_std.copy_(m._policy_fn._model[-1].log_std)
    return m2


def sample_batch(twin, n, seed):
    """A train batch under RLlib's keys (CPU float32) around the twin's current outputs: log-ratios well past the clip
    range on both sides, advantages of both signs, vf_preds / value_targets about one unit from the value."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)                                    # noqa: E731
    obs = rn(n, OBS)
    with torch.no_grad():
        logits = twin(obs)
        value = twin.cur_value
    mean, ls = logits[:, :K], logits[:, K:]
    actions = mean + torch.exp(ls) * rn(n, K)
    logp = -0.5 * (((actions - mean) / torch.exp(ls)) ** 2).sum(1) - ls.sum(1) - 0.5 * K * math.log(2 * math.pi)
    return {"obs": obs, "actions": actions, "action_dist_inputs": torch.cat([mean + 0.02 * rn(n, K), ls + 0.05 * rn(n, K)], 1),
            "action_logp": logp - 0.35 * rn(n), "advantages": rn(n), "value_targets": value + rn(n), "vf_preds": value + rn(n)}


def twin_update(twin, opt, batch, idx, cfg):
    cols = {k: v[idx] for k, v in P.batch_columns(batch).items()}
    obs = cols.pop("obs")
    opt.zero_grad(set_to_none=True)
    logits = twin(obs)
    total, stats = P.ppo_loss_torch(logits[:, :K], logits[:, K:], twin.cur_value, cfg=cfg, **cols)
    total.backward()
    opt.step()
    return stats.detach()


def on_dev(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def hip_step(m, kind, cfg, dbatch, t, first=0, rows=500, index=None, mask=0):
    """One `pvae_fc_ppo_step` through the engine, as ppo_learn binds it."""
    eng = m.engine
    log_std = None if kind == "state_dependent" else m._policy_fn._model[-1].on_device(eng.device)
    eng.ppo_bind(log_std, kind == "state_independent")
    base = float(m._log_std_base) if kind == "state_dependent" else 0.0
    return eng.ppo_step(P.batch_columns(dbatch), cfg.params(kind, base, adam_t=t, train_mask=mask), first, rows, index)


def arena_pads(m, arena):
    live = torch.zeros_like(m.engine.params, dtype=torch.bool)
    for s in range(len(m.engine.stacks)):
        for w, b in m.engine.views(s, live):
            w.fill_(True)
            b.fill_(True)
    return arena[~live]


LS_KEY = "_policy_fn._model.3.log_std"


def arena_views(m, arena):
    """The stacks' weights and biases in a buffer of the arena's layout, under the module's parameter names."""
    views = {}
    for s, prefix in enumerate(("_policy_fn", "_value_fn", "_log_std_fn")[:len(m.engine.stacks)]):
        for i, (w, b) in enumerate(m.engine.views(s, arena)):
            views["%s._model.%d._model.0.weight" % (prefix, i)] = w
            views["%s._model.%d._model.0.bias" % (prefix, i)] = b
    return views


def ls_grad_from_moment(m, beta1=0.9):
    """After the FIRST step from zero moments m = (1 - beta1) g: the gradient `ppo_adam_kernel` formed for the vector."""
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))            # noqa: E731
    return m.engine.ppo_ls_m.double().cpu() / f32(1.0 - f32(beta1))      # (the factor as the library rounds it)


def ls_grad_from_partials(m, rows=500):
    """The head's column sums as it left them in the scratch buffer (include/pvae.h: one partial row per wave, a wave for
    every two padded rows, 8 floats of stats and then the k columns, k rounded up to 4), added here in float64."""
    waves = ((rows + 31) // 32 * 32 + 1) // 2
    waves = (waves + 3) // 4 * 4
    stride = 8 + (K + 3) // 4 * 4
    return m.engine.ppo_scratch[:waves * stride].view(waves, stride)[:, 8:8 + K].double().sum(0).cpu()


def check_stats(got, want, tol, what):
    """Every stat against its own size: |got - want| <= tol * max(|want|, floor).  The policy term is a mean of rows
    adv * ratio of both signs and of order 1, so its rounding error goes with the mean of |term| (floor 1), not with the
    small mean itself; the other four are sums of terms of one sign (floor 0: plain relative error) -- the total but
    for the same cancelling term, so it takes the floor too."""
    got, want = got.double().cpu(), want.double().cpu()
    floors = torch.tensor([1.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    err = (got - want).abs() / torch.maximum(want.abs(), floors).clamp_min(1e-30)
    print(what, "stats err per component", ["%.3g" % float(x) for x in err])
    assert bool((err < tol).all()), (what, err.tolist())


@pytest.mark.parametrize("hyper", ["imitation", "second"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_step_and_five_steps_match_the_twin(kind, hyper):
    cfg = P.PPOConfig(**(IMITATION if hyper == "imitation" else SECOND))
    m, cmc = make(kind)
    twin = Twin(m, cmc)
    batch = sample_batch(twin, 500, seed=7)
    dbatch = on_dev(batch)
    opt = torch.optim.Adam(twin.parameters(), lr=cfg.lr)
    idx = torch.arange(500)
    names = twin.named_like(m)
    mine = dict(m.named_parameters())
    assert set(names) == set(mine)
    for step in range(5):
        want = twin_update(twin, opt, batch, idx, cfg)
        got = hip_step(m, kind, cfg, dbatch, step + 1).cpu()
        print(kind, hyper, step, got.tolist(), want.tolist())
        assert float(got[0]) == pytest.approx(float(want[0]), rel=2e-4), step
        assert max_err_scaled(got, want) < 2e-4
        check_stats(got, want, 2e-4, (kind, hyper, step))
        if step == 0:            # the gradients of the first step, in the library's gradient arena
            for k, g in arena_views(m, m.engine.ppo_grad).items():
                e = max_err_scaled(g.cpu(), names[k].grad)
                assert e < 1e-4, (k, e)
            assert float(arena_pads(m, m.engine.ppo_grad).abs().max()) == 0.0
            if kind == "state_independent":          # the vector's gradient: the head's column sums, finished by the Adam launch
                want_g = names[LS_KEY].grad
                from_m, from_parts = ls_grad_from_moment(m), ls_grad_from_partials(m)
                e = (max_err_scaled(from_m, want_g), max_err_scaled(from_parts, want_g))
                print(kind, hyper, "log_std gradient: from m %.3g, from the partial rows %.3g" % e)
                assert e[0] < 1e-4 and e[1] < 1e-4
    for k, q in names.items():
        e = max_err_scaled(mine[k].detach().cpu(), q.detach())
        assert e < PARAM_BOUND, (k, e)
    # Adam's moments after the five steps against the twin optimizer's.  The parameters move by at most 5 lr here, far
    # inside their bound, so it is the moments that show whether every step's gradient was right.  Bounds: the gradient
    # bound 1e-4, doubled for the drift of the two parameter sets over five steps, for m; twice that for v, which
    # squares the gradient.
    moments = {k: (mm, vv) for (k, mm), vv in zip(arena_views(m, m.engine.ppo_m).items(), arena_views(m, m.engine.ppo_v).values())}
    if kind == "state_independent":
        moments[LS_KEY] = (m.engine.ppo_ls_m, m.engine.ppo_ls_v)
    assert set(moments) == set(names)
    for k, (mm, vv) in moments.items():
        state = opt.state[names[k]]
        e = (max_err_scaled(mm.cpu(), state["exp_avg"]), max_err_scaled(vv.cpu(), state["exp_avg_sq"]))
        print(kind, hyper, k, "m %.3g v %.3g" % e)
        assert e[0] < MOMENT_BOUNDS[0] and e[1] < MOMENT_BOUNDS[1], (k, e)
    if kind == "state_independent":
        ls = m._policy_fn._model[-1].log_std.detach().cpu()
        assert not torch.equal(ls, torch.full_like(ls, math.log(0.3)))               # it trained
    assert float(eng_pad_max(m)) == 0.0
    assert float(arena_pads(m, m.engine.ppo_m).abs().max()) == 0.0 and float(arena_pads(m, m.engine.ppo_v).abs().max()) == 0.0
    assert m.engine.ppo_launches() == 9


@pytest.mark.parametrize("kind", ["constant", "state_dependent"])
def test_sgd_loop_equals_the_steps_one_by_one_and_the_twin(kind):
    cfg = P.PPOConfig(**SECOND)
    m, cmc = make(kind)
    m1 = copy_of(m, cmc)
    twin = Twin(m, cmc)
    n = 1300
    batch = sample_batch(twin, n, seed=9)
    dbatch = on_dev(batch)
    perm = torch.stack([torch.randperm(n, generator=torch.Generator().manual_seed(40 + p)) for p in range(3)]).to(torch.int32)
    dperm = perm.to(DEV)
    stats = m.ppo_learn(dbatch, cfg, perm=dperm)
    assert stats.shape == (9, 5) and stats.device.type == "cuda"
    opt = torch.optim.Adam(twin.parameters(), lr=cfg.lr)
    t = 0
    for p in range(3):
        for first in (0, 500, 1000):
            rows = min(500, n - first)
            t += 1
            one = hip_step(m1, kind, cfg, dbatch, t, first, rows, dperm[p])
            assert torch.equal(one, stats[t - 1]), (p, first)
            want = twin_update(twin, opt, batch, perm[p, first: first + rows].long(), cfg)
            assert float(one[0]) == pytest.approx(float(want[0]), rel=2e-4), (p, first)
    assert torch.equal(m.engine.params, m1.engine.params)
    assert torch.equal(m.engine.ppo_m, m1.engine.ppo_m) and torch.equal(m.engine.ppo_v, m1.engine.ppo_v)
    mine = dict(m.named_parameters())
    for k, q in twin.named_like(m).items():
        assert max_err_scaled(mine[k].detach().cpu(), q.detach()) < 2e-3, k
    # a second call goes on from the optimizer state of the first; row order when no permutation is given
    more = m.ppo_learn(dbatch, P.PPOConfig(**dict(SECOND, num_sgd_iter=1)))
    assert more.shape == (3, 5) and m.__dict__["_ppo_t"] == 12
    one = hip_step(m1, kind, cfg, dbatch, 10, 0, 500, None)
    assert torch.equal(one, more[0])
    m.reset_ppo_optimizer()
    assert m.__dict__["_ppo_t"] == 0 and float(m.engine.ppo_m.abs().max()) == 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_fused_step_gradients_equal_forward_hip_loss_backward(kind):
    """forward + HipPPOLoss + backward() and the fused step run the same kernels on the same operands in the same order
    (the autograd path recomputes the forward and copies the head's output gradients through the seed launch): the stacks'
    parameter gradients are the same bits."""
    cfg = P.PPOConfig(**SECOND)
    m, cmc = make(kind)
    batch = sample_batch(Twin(m, cmc), 500, seed=13)
    dbatch = on_dev(batch)
    cols = P.batch_columns(dbatch)
    logits, _ = m.forward({"obs_flat": dbatch["obs"]}, [], None)
    base = float(m._log_std_base) if kind == "state_dependent" else 0.0
    total, stats = P.HipPPOLoss.apply(logits[:, :K], logits[:, K:], m.value_function(), cols, cfg.params(kind, base), None)
    (2.0 * total).backward()
    grads = {k: p.grad.clone() for k, p in m.named_parameters()}
    got = hip_step(m, kind, cfg, dbatch, 1)
    assert torch.equal(got, stats)
    eng = m.engine
    for s, fn in enumerate((m._policy_fn, m._value_fn, m._log_std_fn)[:len(eng.stacks)]):
        lins = [x._model[0] for x in fn._model if hasattr(x, "_model")]
        for lin, (w, b) in zip(lins, eng.views(s, eng.ppo_grad)):
            assert torch.equal(lin.weight.grad, 2.0 * w) and torch.equal(lin.bias.grad, 2.0 * b), s
    if kind == "state_independent":
        # the one gradient whose schedules differ (torch's reduction of the expanded vector there, the partial rows
        # here): to 1e-6, as formed by the Adam launch and as the head left it
        want_g = (grads[LS_KEY] / 2.0).double().cpu()
        assert float(want_g.abs().max()) > 0
        e = (max_err_scaled(ls_grad_from_moment(m), want_g), max_err_scaled(ls_grad_from_partials(m), want_g))
        print("log_std gradient against HipPPOLoss + backward(): from m %.3g, from the partial rows %.3g" % e)
        assert e[0] < 1e-6 and e[1] < 1e-6


def test_launch_count_does_not_grow_with_the_stacks():
    cfg = P.PPOConfig(**IMITATION)
    counts = {}
    for kind in ("constant", "state_dependent"):
        m, cmc = make(kind)
        dbatch = on_dev(sample_batch(Twin(m, cmc), 500, seed=3))
        hip_step(m, kind, cfg, dbatch, 1)
        counts[kind] = m.engine.ppo_launches()
        hip_step(m, kind, cfg, dbatch, 2, 0, 33)
        assert m.engine.ppo_launches() == 9
    assert counts == {"constant": 9, "state_dependent": 9}


@pytest.mark.parametrize("kind", KINDS)
def test_stale_buffers_reach_nothing(kind):
    cfg = P.PPOConfig(**SECOND)
    m, cmc = make(kind)
    m1 = copy_of(m, cmc)
    dbatch = on_dev(sample_batch(Twin(m, cmc), 600, seed=17))       # the steps below take rows [100, 100 + rows)
    for rows in (500, 37, 3):
        hip_step(m1, kind, cfg, dbatch, 1, 0, 1)               # (binds: the buffers exist)
        m1.reset_ppo_optimizer()
        with torch.no_grad():
            m1.engine.params.copy_(m.engine.params)
            if kind == "state_independent":
                m1._policy_fn._model[-1].log_std.copy_(m._policy_fn._model[-1].log_std)
        for buf in (m1.engine.workspace, m1.engine.ppo_scratch, m1.engine.ppo_grad):
            buf.fill_(float("nan"))
        m.reset_ppo_optimizer()
        dirty = hip_step(m1, kind, cfg, dbatch, 1, 100, rows)
        clean = hip_step(m, kind, cfg, dbatch, 1, 100, rows)
        assert bool(torch.isfinite(dirty).all()) and torch.equal(dirty, clean), rows
        assert torch.equal(m.engine.params, m1.engine.params) and bool(torch.isfinite(m1.engine.params).all())
        assert bool(torch.isfinite(m1.engine.ppo_grad).all()) and torch.equal(m.engine.ppo_grad, m1.engine.ppo_grad)
        assert torch.equal(m.engine.ppo_m, m1.engine.ppo_m) and torch.equal(m.engine.ppo_v, m1.engine.ppo_v)
        if kind == "state_independent":
            assert torch.equal(m._policy_fn._model[-1].log_std, m1._policy_fn._model[-1].log_std)


def test_frozen_value_stack_is_left_alone():
    cfg = P.PPOConfig(**dict(SECOND, num_sgd_iter=2))
    m, cmc = make("state_dependent")
    m1 = copy_of(m, cmc)
    dbatch = on_dev(sample_batch(Twin(m, cmc), 500, seed=19))
    m1._value_fn.requires_grad_(False)
    before = m1.engine.params.clone()
    full = m.ppo_learn(dbatch, cfg)
    part = m1.ppo_learn(dbatch, cfg)
    assert torch.equal(full[0], part[0])                                     # the first step sees the same policy and value
    assert torch.equal(full[:, [1, 3, 4]], part[:, [1, 3, 4]])               # and the policy's terms never see the value stack
    assert not torch.equal(full[-1, 2], part[-1, 2])
    for (w, b), (w0, b0), (wm, bm), (wv, bv) in zip(m1.engine.views(1), m1.engine.views(1, before),
                                                    m1.engine.views(1, m1.engine.ppo_m), m1.engine.views(1, m1.engine.ppo_v)):
        assert torch.equal(w, w0) and torch.equal(b, b0)
        assert float(wm.abs().max()) == 0.0 and float(bm.abs().max()) == 0.0 and float(wv.abs().max()) == 0.0 and float(bv.abs().max()) == 0.0
    for s in (0, 2):
        for (w, b), (w1, b1) in zip(m.engine.views(s), m1.engine.views(s)):
            assert torch.equal(w, w1) and torch.equal(b, b1)
    assert not torch.equal(m.engine.views(0)[0][0], m.engine.views(0, before)[0][0])      # the policy stack did move
    assert not torch.equal(m.engine.views(1)[0][0], m.engine.views(1, before)[0][0])      # and, unfrozen, so does the value stack
    next(iter(m1._policy_fn.parameters())).requires_grad_(False)
    with pytest.raises(NotImplementedError, match="_policy_fn is partially frozen"):
        m1.ppo_learn(dbatch, cfg)


@pytest.mark.parametrize("kind", KINDS)
def test_nothing_else_moved(kind):
    m, cmc = make(kind)
    dbatch = on_dev(sample_batch(Twin(m, cmc), 700, seed=23))
    x = dbatch["obs"][:300].contiguous()
    with torch.no_grad():
        l0, _ = m.forward({"obs_flat": x}, [], None)
        v0 = m.value_function().clone()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    stats = m.ppo_learn(dbatch, P.PPOConfig(**dict(IMITATION, lr=0.0, num_sgd_iter=2)))
    assert stats.shape == (4, 5) and bool(torch.isfinite(stats).all())
    assert torch.equal(stats[0], stats[2]) and torch.equal(stats[1], stats[3])           # lr 0: every pass sees the same policy
    with torch.no_grad():
        l1, _ = m.forward({"obs_flat": x}, [], None)
        v1 = m.value_function().clone()
    assert torch.equal(l0, l1) and torch.equal(v0, v1)
    sd1 = m.state_dict()
    assert list(sd0) == list(sd1) and all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    with pytest.raises(ValueError, match="max_batch"):
        m.ppo_learn(dbatch, P.PPOConfig(sgd_minibatch_size=513))
