"""Sweep of PhysicsVAE's PPO learner and evaluate pass (pvae_ppo.hip) against float64, through `PhysicsVAE` and `HipEngine`:
40 random and 20 directed models of tests/vae_ppo_cases.py -- stacks given layer by layer (a width and an activation per layer,
unequal depths), Db / Da / Z / widths that are multiples of no tile, Z = 1 and Da = 1, input subsets, both priors, noise on and
off, both log-std kinds, every train mask, 1 .. 130 rows, gathered minibatches, and the two grid caps of the kernels that are
PhysicsVAE's own.  Per case: (a) one step against the float64 twin -- stats, every gradient, pads, frozen nets, the launch
count; (b) three steps against torch.optim.Adam on the twin; (c) the structural zeros, exactly; (d) pvae_ppo_grad +
pvae_ppo_apply against the step, bit for bit; (e) on every fourth case `ppo_learn` against the steps one by one; (f) the
evaluate pass, and `ppo_prepare` straight into `ppo_learn`.  tests/test_vae_ppo_cases_cpu.py checks without a GPU that the
cases are what is claimed here and that the float32 twin of each stays within a quarter of these bounds.

Bounds, the suite's standing ones for the same quantities (tests/test_gpu_ppo_vae.py, tests/test_gpu_ppo_vae_prepare.py):
stats 2e-4 by `check_stats`; gradients 1e-4 by max_err_scaled, flat; moments 2e-4 / 4e-4 and parameters 2e-3 after three
steps; vf_preds, old_dist and last_value 1e-5 by max_err_scaled, old_logp 1e-5 by `logp_err`; the KL of the first step after
`ppo_prepare` below 2e-4.  The float32 twin's own distance from the float64 twin is printed beside every figure."""
import pytest
import torch

import fc_cases as F
import vae_ppo_cases as V
from physicsvae_amd import _lib
from physicsvae_amd import ppo as P
from test_gpu_gae import guarded, guards_intact, logp_err
from test_gpu_ppo import check_stats
from test_gpu_ppo_vae import all_pads, ls_grad_from_moment, mask_of
from test_gpu_ppo_vae_prepare import bind, want_launches
from util import max_err_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = P.PPOConfig(lr=V.LR, **F.LOSS)
KEY = "%s._model.%d._model.0.%s"


def launches(c):
    """`launches()` of tests/test_gpu_ppo_vae.py with the train mask: the decoder's backward goes out for its own gradient or
    to pass one on to a trained encoder, the sampler's and the encoder's backward for a trained encoder, the value stack's for
    a trained value branch."""
    te, md, vb = c.depths
    forward = 1 + (1 if c.rows <= 4 else 0) + (te + 1) + 1 + (md + 1) + (vb + 1) + 1
    backward = (md + 1 if c.mask & 3 else 0) + (1 + te + 1 if c.mask & 1 else 0) + (vb + 1 if c.mask & 4 else 0)
    return forward + backward + 1


def views_of(m, arena=None, value_arena=None):
    """The three nets' weights and biases in buffers of the two arenas' layouts (None: the parameters), under the module's names."""
    eng, ve = m.engine, m.__dict__["_value_engine"]
    views = {k: v for k, v in eng.named_views(arena).items() if k.split(".")[0] in V.NETS}
    for i, (w, b) in enumerate(ve.views(0, value_arena)):
        views[KEY % ("_value_branch", i, "weight")], views[KEY % ("_value_branch", i, "bias")] = w, b
    return views


def buffers(m, which):
    ve = m.__dict__["_value_engine"]
    return views_of(m, getattr(m.engine, "ppo_" + which), getattr(ve, "ppo_" + which))


def outside_window(m, arena):
    """max |value| of `arena` in the first-layer columns an input subset leaves out."""
    worst = 0.0
    for info in m.engine.layers:
        if info["index"] == 0 and info["net"] in (_lib.NET_TE, _lib.NET_MD):
            blk = arena[info["w_offset"]: info["w_offset"] + info["n_out_pad"] * info["ld"]].view(info["n_out_pad"], info["ld"])
            for part in (blk[:, : info["col0"]], blk[:, info["col0"] + info["n_in"]:]):
                if part.numel():
                    worst = max(worst, float(part.abs().max()))
    return worst


def params_of(c, m, t):
    train_ls = c.log_std_type == "state_independent"
    return CFG.params("state_independent" if train_ls else "constant", 0.0, adam_t=t, train_mask=mask_of(m))


def setup(c):
    m = V.module_for(c, DEV)
    assert m._ppo_train_mask() == c.mask
    eng = bind(m)
    ve = m.__dict__["_value_engine"]
    for buf in (eng.workspace, ve.workspace, eng.ppo_scratch):          # stale panel contents must reach nothing
        buf.fill_(float("nan"))
    return m, eng, ve


def state(m):
    """Everything a step may move, as clones."""
    eng, ve = m.engine, m.__dict__["_value_engine"]
    out = {"params": eng.params, "value params": ve.params, "m": eng.ppo_m, "v": eng.ppo_v, "value m": ve.ppo_m, "value v": ve.ppo_v,
           "log_std": m._als.log_std.detach()}
    if eng.ppo_ls_m is not None:
        out.update(ls_m=eng.ppo_ls_m, ls_v=eng.ppo_ls_v)
    return {k: v.clone() for k, v in out.items()}


def same_state(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


@pytest.mark.parametrize("name", V.CASE_IDS)
def test_learner_matches_the_float64_twin(name):
    c = V.case(name)
    train_ls = c.log_std_type == "state_independent"
    m, eng, ve = setup(c)
    cols = eng.ppo_batch({k: v.to(DEV) for k, v in c.batch.items()})
    index = c.index.to(DEV) if c.index is not None else None
    eps = c.eps.to(DEV)
    want, e32 = V.step_twin(c, steps=3), V.twin32_errors(name)
    before = {k: v.clone() for k, v in views_of(m).items()}
    trained = [net for bit, net in zip((1, 2, 4), V.NETS) if c.mask & bit]
    frozen = [net for net in V.NETS if net not in trained]
    print(name, "Db %d Da %d Z %d rows %d of %d" % (c.Db, c.Da, c.Z, c.rows, c.max_batch), c.te, c.md, c.vb, c.prior, "noise", c.noise,
          c.log_std_type, c.te_inputs, c.md_inputs, "mask", c.mask, "gathered" if c.gathered else "in order")

    # (a) one step
    stats = [eng.ppo_step(cols, params_of(c, m, 1), c.first, c.rows, index, eps=eps, noise=c.noise, offset=1).clone()]
    assert eng.ppo_launches() == launches(c), (eng.ppo_launches(), launches(c))
    check_stats(stats[0].cpu(), want.stats[0], V.STATS_BOUND, name)
    grad = buffers(m, "grad")
    e_grad = 0.0
    for net in trained:
        for i, pair in enumerate(want.grads[net]):
            for kind, g in zip(("weight", "bias"), pair):
                e = max_err_scaled(grad[KEY % (net, i, kind)].cpu(), g)      # (an all-zero gradient of the twin: exactly zero)
                e_grad = max(e_grad, e)
                assert e < V.GRAD_BOUND, (name, net, i, kind, e)
    if train_ls:
        e = max_err_scaled(ls_grad_from_moment(m), want.ls_grad)
        e_grad = max(e_grad, e)
        assert e < V.GRAD_BOUND, (name, "log_std", e)
    print(name, "gradients %.3g  float32 twin %.3g  bound %.3g" % (e_grad, e32["gradients"], V.GRAD_BOUND))
    for which in ("params", "grad", "m", "v"):
        assert float(all_pads(m, which).abs().max()) == 0.0, which

    # (b) three steps
    for t in (2, 3):
        stats.append(eng.ppo_step(cols, params_of(c, m, t), c.first, c.rows, index, eps=eps, noise=c.noise, offset=t).clone())
    assert bool(torch.isfinite(torch.stack(stats)).all())
    now, mom_m, mom_v = views_of(m), buffers(m, "m"), buffers(m, "v")
    e_p, e_m, e_v = [0.0], [0.0], [0.0]
    for net in trained:
        for i, pair in enumerate(want.params[net]):
            for kind, leaf in zip(("weight", "bias"), pair):
                k = KEY % (net, i, kind)
                wm, wv = V.state_of(want.opt, leaf)
                e_p.append(max_err_scaled(now[k].cpu(), leaf.detach()))
                e_m.append(max_err_scaled(mom_m[k].cpu(), wm))
                e_v.append(max_err_scaled(mom_v[k].cpu(), wv))
        if not V.structurally_zero(c, net):
            assert any(not torch.equal(now[k], before[k]) for k in now if k.startswith(net + ".")), (name, net, "did not move")
    if train_ls:
        wm, wv = V.state_of(want.opt, want.ls_vec)
        e_p.append(max_err_scaled(m._als.log_std.detach().cpu(), want.ls_vec.detach()))
        e_m.append(max_err_scaled(eng.ppo_ls_m.cpu(), wm))
        e_v.append(max_err_scaled(eng.ppo_ls_v.cpu(), wv))
        assert not torch.equal(m._als.log_std.detach().cpu(), c.ls_vec)
    else:
        assert torch.equal(m._als.log_std.detach().cpu(), c.ls_vec)
    print(name, "after three steps: parameters %.3g (float32 twin %.3g)  m %.3g (%.3g)  v %.3g (%.3g)"
          % (max(e_p), e32["parameters"], max(e_m), e32["m"], max(e_v), e32["v"]))
    assert max(e_p) < V.PARAM_BOUND and max(e_m) < V.MOMENT_BOUNDS[0] and max(e_v) < V.MOMENT_BOUNDS[1]
    for net in frozen:                                                   # a frozen net: parameters the bits they were, no moments
        for k in now:
            if k.startswith(net + "."):
                assert torch.equal(now[k], before[k]), k
                assert float(mom_m[k].abs().max()) == 0.0 and float(mom_v[k].abs().max()) == 0.0, k

    # (c) structural zeros, exactly
    for which in ("params", "grad", "m", "v"):
        assert float(all_pads(m, which).abs().max()) == 0.0, which
    for arena in (eng.params, eng.ppo_grad, eng.ppo_m, eng.ppo_v):
        assert outside_window(m, arena) == 0.0
        assert float(eng.segment(arena, [_lib.NET_WM]).abs().max()) == 0.0           # (the world model: nothing else moved)
    grad = buffers(m, "grad")
    if c.mask & 1 and V.structurally_zero(c, "_task_encoder"):
        for k in now:
            if k.startswith("_task_encoder."):
                assert float(grad[k].abs().max()) == 0.0 and float(mom_m[k].abs().max()) == 0.0 and float(mom_v[k].abs().max()) == 0.0, k
                assert torch.equal(now[k], before[k]), k
    if c.mask & 1 and c.prior and not c.noise:                           # noise off: the logvar half has no gradient
        last = len(c.te[0])
        for kind in ("weight", "bias"):
            assert float(grad[KEY % ("_task_encoder", last, kind)][c.Z:].abs().max()) == 0.0, kind

    # (d) pvae_ppo_grad + pvae_ppo_apply(grad_scale = 1) on a second module: the same bits
    m2, eng2, ve2 = setup(c)
    for t in (1, 2, 3):
        p = params_of(c, m2, t)
        one, ls_grad = eng2.ppo_grad_step(cols, p, c.first, c.rows, index, eps=eps, noise=c.noise, offset=t)
        eng2.ppo_apply(p, 1.0, ls_grad if train_ls else None)
        assert torch.equal(one, stats[t - 1]), (name, "grad + apply", t)
    assert not same_state(state(m), state(m2)), same_state(state(m), state(m2))

    # (e) ppo_learn against the steps one by one, continuing both modules from Adam's t = 3
    if V.CASE_IDS.index(name) % 4 == 0:
        g = torch.Generator().manual_seed(c.seed + 9)
        n, rows = 2 * c.rows + 3, c.rows
        pick = torch.randint(c.rows, (n,), generator=g)                  # rows of the used batch, with repeats: finite everywhere
        batch = {k: v[pick].to(DEV) for k, v in c.used.items()}
        per_pass = -(-n // rows)
        perm = torch.stack([torch.randperm(n, generator=g) for _ in range(2)]).to(torch.int32).to(DEV)
        leps = torch.randn(2 * per_pass, rows, c.Z, generator=g).to(DEV)
        rllib = {theirs: batch[ours] for theirs, ours in P.SAMPLE_BATCH_KEYS.items()}
        m.__dict__["_ppo_t"] = 3
        learned = m.ppo_learn(rllib, P.PPOConfig(lr=V.LR, sgd_minibatch_size=rows, num_sgd_iter=2, **F.LOSS), perm=perm, eps=leps)
        assert learned.shape == (2 * per_pass, 5) and bool(torch.isfinite(learned).all()) and m.__dict__["_ppo_t"] == 3 + 2 * per_pass
        cols2 = eng2.ppo_batch(batch)
        i = 0
        for p in range(2):
            for first in range(0, n, rows):
                r = min(rows, n - first)
                one = eng2.ppo_step(cols2, params_of(c, m2, 4 + i), first, r, perm[p].contiguous(), eps=leps[i, :r].contiguous(),
                                    noise=c.noise, offset=4 + i)
                assert torch.equal(one, learned[i]), (name, "ppo_learn", p, first)
                i += 1
        assert not same_state(state(m), state(m2)), same_state(state(m), state(m2))


@pytest.mark.parametrize("name", V.CASE_IDS)
def test_evaluate_pass_matches_the_float64_twin(name):
    c = V.case(name)
    m, eng, ve = setup(c)
    ro, eps, want = V.rollout(name)
    e32 = V.twin32_errors(name)
    n, s = ro["obs"].shape[0], ro["seg_done"].numel()
    deps = eps.to(DEV)
    dro = {"obs": ro["obs"].to(DEV), "actions": ro["actions"].to(DEV), "seg_done": ro["seg_done"].to(DEV),
           "boot_obs": ro["next_obs_last"].to(DEV)}
    bufs = {"vf_preds": guarded(n), "old_dist": guarded(n, 2 * c.Da), "old_logp": guarded(n), "last_value": guarded(s),
            "latent_eps": guarded(n, c.Z)}
    cfg = P.PPOConfig(clip_param=0.2, kl_coeff=0.3, entropy_coeff=0.01, vf_clip_param=10.0, lr=V.LR, sgd_minibatch_size=c.max_batch,
                      num_sgd_iter=1, gamma=V.GAMMA, lambda_=V.LAMBDA)
    got = eng.ppo_evaluate(dro, cfg.gae_params(c.log_std_type), eps=deps, noise=c.noise, out={k: v[1] for k, v in bufs.items()})
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b, _ in bufs.values())
    ev, rest = want_launches(m, n, s)
    assert eng.gae_launches() == (ev, rest - 2), (eng.gae_launches(), ev, rest - 2)
    e = {"vf_preds": max_err_scaled(got["vf_preds"].cpu(), want["vf_preds"]),
         "old_dist": max_err_scaled(got["old_dist"].cpu(), want["old_dist"]),
         "last_value": max_err_scaled(got["last_value"].cpu(), want["last_value"]),
         "old_logp": logp_err(got["old_logp"], want["old_logp"])}
    print(name, "Db %d Da %d Z %d rows %d in chunks of %d" % (c.Db, c.Da, c.Z, n, c.max_batch), c.prior, "noise", c.noise, c.te_inputs,
          c.md_inputs, "vf_preds %.3g last_value %.3g (float32 twin %.3g)  old_dist %.3g (%.3g)  old_logp %.3g (%.3g)  bound %.3g"
          % (e["vf_preds"], e["last_value"], e32["value"], e["old_dist"], e32["mean"], e["old_logp"], e32["action_logp"], V.EVAL_BOUND))
    assert all(v <= V.EVAL_BOUND for v in e.values()), (name, e)
    done = ro["seg_done"]
    assert bool((got["last_value"].cpu()[done] == 0.0).all())
    # the draws that were used come back: the supplied ones; zeros without a prior or with the noise off
    assert torch.equal(got["latent_eps"].cpu(), eps if (c.prior and c.noise) else torch.zeros_like(eps))
    # prepare straight into learn, the draws replayed row by row: the first step sees its own distribution
    batch = m.ppo_prepare({k: v.to(DEV) for k, v in ro.items()}, cfg, eps=deps)
    assert m.engine.gae_launches() == (ev, rest)
    assert all(torch.equal(batch[theirs], got[ours]) for theirs, ours in (("vf_preds", "vf_preds"), ("action_dist_inputs", "old_dist"),
                                                                          ("action_logp", "old_logp"), ("last_value", "last_value")))
    steps = -(-n // c.max_batch)
    leps = torch.zeros(steps * c.max_batch, c.Z, device=DEV)
    leps[:n] = deps
    stats = m.ppo_learn(batch, cfg, eps=leps.view(steps, c.max_batch, c.Z))
    assert stats.shape == (steps, 5) and bool(torch.isfinite(stats).all())
    print(name, "first step after prepare", stats[0].tolist())
    assert abs(float(stats[0, 3])) < 2e-4
