"""PhysicsVAE's fused PPO passes under the learned prior ("normal_state_mean_one_std") and the sphere prior
("hypersphere_uniform"), which a configuration opts into with "ppo_priors": the 24 random and 19 directed models of
tests/vae_ppo_prior_cases.py against their float64 twin, in the blocks of tests/test_gpu_ppo_vae_shapes.py (whose helpers
are used as they stand).  Per case: (a) one step from a NaN-filled workspace -- launch count, stats, every trained gradient,
pads; (b) three steps against torch.optim.Adam on the twin, frozen nets; (c) the structural zeros, exactly -- under the
learned prior also the prior stack's segment: parameters the bits they were, gradient and moments zero; (d) pvae_ppo_grad +
pvae_ppo_apply against the step, bit for bit; (e) on every fourth case `ppo_learn` against the steps one by one, on one case
per prior also with diagnostics and a clip that never bites; then the evaluate pass and `ppo_prepare` into `ppo_learn`,
`compute_actions` -> `ppo_prepare` -> `ppo_learn` through a `RolloutBuffer`, the fused step against forward + HipPPOLoss +
backward() under the sphere (the new backward kernel against the autograd path's), and the opt-in on the device.

Bounds: those of tests/test_gpu_ppo_vae_shapes.py (stats 2e-4, gradients 1e-4, moments 2e-4 / 4e-4, parameters 2e-3 after
three steps, evaluate columns 1e-5, the KL of a first step on its own distribution below 2e-4);
tests/test_vae_ppo_prior_cases_cpu.py holds the float32 twin of every case to a quarter of them.  `sphere_z1`: the
encoder's gradient is a rounding residue around an exact zero (z = sign(e)); its tensors are held to GRAD_BOUND times the
largest entry of the twin's decoder gradients and take no part in the relative measures."""
import numpy as np
import pytest
import torch

import fc_cases as F
import test_gpu_ppo_vae_shapes as TS
import vae_ppo_cases as V
import vae_ppo_prior_cases as W
from physicsvae_amd import _lib
from physicsvae_amd import ppo as P
from test_gpu_gae import guarded, guards_intact, logp_err
from test_gpu_ppo import check_stats
from test_gpu_ppo_vae import all_pads, ls_grad_from_moment
from test_gpu_ppo_vae_prepare import bind, want_launches
from util import max_err_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEY = TS.KEY
LEARN_TOO = (0, 5)                 # (e) runs on the cases whose index is one of these modulo 8: every fourth, both priors
WITH_DIAG_AND_CLIP = ("sphere_z64", "state_mean_noise_off")
NEVER = 1e30


def setup(c, opt_in=True):
    m = W.module_for(c, DEV, opt_in=opt_in)
    assert m._ppo_train_mask() == c.mask
    eng = bind(m)
    ve = m.__dict__["_value_engine"]
    for buf in (eng.workspace, ve.workspace, eng.ppo_scratch):          # stale panel contents must reach nothing
        buf.fill_(float("nan"))
    return m, eng, ve


def prior_segments(eng):
    """The prior stack's segment of the parameter arena and of the PPO step's gradient and moment arenas."""
    return [eng.segment(a, [_lib.NET_PR]) for a in (eng.params, eng.ppo_grad, eng.ppo_m, eng.ppo_v)]


def test_the_learn_and_diag_selections_meet_both_priors():
    learn = [W.case(name) for i, name in enumerate(W.CASE_IDS) if i % 8 in LEARN_TOO]
    assert 4 * len(learn) >= len(W.CASE_IDS) and {c.prior for c in learn} == {W.SPHERE, W.LEARNED}
    assert all(W.CASE_IDS.index(name) % 8 in LEARN_TOO and W.case(name).mask & 1 for name in WITH_DIAG_AND_CLIP)
    assert [W.case(name).prior for name in WITH_DIAG_AND_CLIP] == [W.SPHERE, W.LEARNED]


@pytest.mark.parametrize("name", W.CASE_IDS)
def test_learner_matches_the_float64_twin(name):
    c = W.case(name)
    train_ls = c.log_std_type == "state_independent"
    m, eng, ve = setup(c)
    cols = eng.ppo_batch({k: v.to(DEV) for k, v in c.batch.items()})
    index = c.index.to(DEV) if c.index is not None else None
    eps = c.eps.to(DEV)
    want, e32 = W.step_twin(c, steps=3), W.twin32_errors(name)
    before = {k: v.clone() for k, v in TS.views_of(m).items()}
    pr_before = prior_segments(eng)[0].clone() if c.prior == W.LEARNED else None
    trained = [net for bit, net in zip((1, 2, 4), V.NETS) if c.mask & bit]
    frozen = [net for net in V.NETS if net not in trained]
    print(name, "Db %d Da %d Z %d rows %d of %d" % (c.Db, c.Da, c.Z, c.rows, c.max_batch), c.te, c.md, c.vb, c.prior, c.pr, "noise", c.noise,
          c.log_std_type, c.te_inputs, c.md_inputs, "mask", c.mask, "gathered" if c.gathered else "in order")

    # (a) one step
    stats = [eng.ppo_step(cols, TS.params_of(c, m, 1), c.first, c.rows, index, eps=eps, noise=c.noise, offset=1).clone()]
    assert eng.ppo_launches() == TS.launches(c), (eng.ppo_launches(), TS.launches(c))
    check_stats(stats[0].cpu(), want.stats[0], V.STATS_BOUND, name)
    grad = TS.buffers(m, "grad")
    e_grad = 0.0
    for net in trained:
        if W.residue(c, net):
            _, md_scale = W.residue_scale(c, want.grads)
            worst = max(float(grad[k].abs().max()) for k in grad if k.startswith(net + "."))
            print(name, "the encoder's residue %.3g, bound %.3g" % (worst, V.GRAD_BOUND * md_scale))
            assert all(bool(torch.isfinite(grad[k]).all()) for k in grad if k.startswith(net + ".")) and worst <= V.GRAD_BOUND * md_scale
            continue
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
        stats.append(eng.ppo_step(cols, TS.params_of(c, m, t), c.first, c.rows, index, eps=eps, noise=c.noise, offset=t).clone())
    assert bool(torch.isfinite(torch.stack(stats)).all())
    now, mom_m, mom_v = TS.views_of(m), TS.buffers(m, "m"), TS.buffers(m, "v")
    e_p, e_m, e_v = [0.0], [0.0], [0.0]
    for net in trained:
        if W.residue(c, net):
            assert all(bool(torch.isfinite(now[k]).all()) for k in now if k.startswith(net + "."))
            continue
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
        assert TS.outside_window(m, arena) == 0.0
        assert float(eng.segment(arena, [_lib.NET_WM]).abs().max()) == 0.0           # (the world model: nothing else moved)
    if c.prior == W.LEARNED:                                             # the prior stack: never run, in no Adam segment
        pr = prior_segments(eng)
        assert pr[0].numel() > 0 and float(pr[0].abs().max()) > 0 and torch.equal(pr[0], pr_before)
        assert all(float(seg.abs().max()) == 0.0 for seg in pr[1:])
    grad = TS.buffers(m, "grad")
    if c.mask & 1 and V.structurally_zero(c, "_task_encoder"):
        for k in now:
            if k.startswith("_task_encoder."):
                assert float(grad[k].abs().max()) == 0.0 and float(mom_m[k].abs().max()) == 0.0 and float(mom_v[k].abs().max()) == 0.0, k
                assert torch.equal(now[k], before[k]), k
    if c.mask & 1 and c.prior == W.LEARNED and not c.noise:               # noise off: the logvar half has no gradient
        last = len(c.te[0])
        for kind in ("weight", "bias"):
            assert float(grad[KEY % ("_task_encoder", last, kind)][c.Z:].abs().max()) == 0.0, kind

    # (d) pvae_ppo_grad + pvae_ppo_apply(grad_scale = 1) on a second module: the same bits
    m2, eng2, ve2 = setup(c)
    for t in (1, 2, 3):
        p = TS.params_of(c, m2, t)
        one, ls_grad = eng2.ppo_grad_step(cols, p, c.first, c.rows, index, eps=eps, noise=c.noise, offset=t)
        eng2.ppo_apply(p, 1.0, ls_grad if train_ls else None)
        assert torch.equal(one, stats[t - 1]), (name, "grad + apply", t)
    assert not TS.same_state(TS.state(m), TS.state(m2)), TS.same_state(TS.state(m), TS.state(m2))

    # (e) ppo_learn against the steps one by one, continuing both modules from Adam's t = 3
    if W.CASE_IDS.index(name) % 8 in LEARN_TOO:
        g = torch.Generator().manual_seed(c.seed + 9)
        n, rows = 2 * c.rows + 3, c.rows
        pick = torch.randint(c.rows, (n,), generator=g)                  # rows of the used batch, with repeats: finite everywhere
        batch = {k: v[pick].to(DEV) for k, v in c.used.items()}
        per_pass = -(-n // rows)
        perm = torch.stack([torch.randperm(n, generator=g) for _ in range(2)]).to(torch.int32).to(DEV)
        leps = torch.randn(2 * per_pass, rows, c.Z, generator=g).to(DEV)
        rllib = {theirs: batch[ours] for theirs, ours in P.SAMPLE_BATCH_KEYS.items()}
        m.__dict__["_ppo_t"] = 3
        calls = m._st._rng_calls
        learned = m.ppo_learn(rllib, P.PPOConfig(lr=V.LR, sgd_minibatch_size=rows, num_sgd_iter=2, **F.LOSS), perm=perm, eps=leps)
        assert learned.shape == (2 * per_pass, 5) and bool(torch.isfinite(learned).all()) and m.__dict__["_ppo_t"] == 3 + 2 * per_pass
        assert m._st._rng_calls == calls + 2 * per_pass                  # one offset per step under every prior
        cols2 = eng2.ppo_batch(batch)
        i = 0
        for p in range(2):
            for first in range(0, n, rows):
                r = min(rows, n - first)
                one = eng2.ppo_step(cols2, TS.params_of(c, m2, 4 + i), first, r, perm[p].contiguous(), eps=leps[i, :r].contiguous(),
                                    noise=c.noise, offset=4 + i)
                assert torch.equal(one, learned[i]), (name, "ppo_learn", p, first)
                i += 1
        assert not TS.same_state(TS.state(m), TS.state(m2)), TS.same_state(TS.state(m), TS.state(m2))

    # diagnostics, and a clip that never bites: the first step of (a) through `ppo_learn`, on two fresh modules
    if name in WITH_DIAG_AND_CLIP:
        rllib = {theirs: c.used[ours].to(DEV) for theirs, ours in P.SAMPLE_BATCH_KEYS.items()}
        kw = dict(lr=V.LR, sgd_minibatch_size=c.rows, num_sgd_iter=1, **F.LOSS)
        (m3, _, _), (m4, _, _) = setup(c), setup(c)
        diag3, diag4 = (P.diag_buffer(c.rows, P.PPOConfig(**kw), DEV) for _ in range(2))
        plain = m3.ppo_learn(rllib, P.PPOConfig(**kw), eps=eps.view(1, c.rows, c.Z), diag_out=diag3)
        clipped = m4.ppo_learn(rllib, P.ClippedPPOConfig(grad_clip=NEVER, **kw), eps=eps.view(1, c.rows, c.Z), diag_out=diag4)
        assert torch.equal(plain[0], stats[0]) and torch.equal(clipped, plain)
        assert not TS.same_state(TS.state(m3), TS.state(m4)), TS.same_state(TS.state(m3), TS.state(m4))
        assert torch.equal(diag3[:, :5], diag4[:, :5]) and float(diag4[0, 6]) == 1.0
        twin = [t for net in trained for pair in want.grads[net] for t in pair] + ([want.ls_grad] if train_ls else [])
        norm = float(P.grad_gnorm_torch(twin))
        gn = P.DIAG.index("grad_gnorm")
        print(name, "grad_gnorm", float(diag3[0, gn]), "float64 twin", norm)
        assert abs(float(diag3[0, gn]) - norm) <= V.GRAD_BOUND * norm and abs(float(diag4[0, 5]) - norm) <= V.GRAD_BOUND * norm


@pytest.mark.parametrize("name", W.CASE_IDS)
def test_evaluate_pass_matches_the_float64_twin(name):
    c = W.case(name)
    m, eng, ve = setup(c)
    ro, eps, want = W.rollout(name)
    e32 = W.twin32_errors(name)
    n, s = ro["obs"].shape[0], ro["seg_done"].numel()
    deps = eps.to(DEV)
    dro = {"obs": ro["obs"].to(DEV), "actions": ro["actions"].to(DEV), "seg_done": ro["seg_done"].to(DEV),
           "boot_obs": ro["next_obs_last"].to(DEV)}
    bufs = {"vf_preds": guarded(n), "old_dist": guarded(n, 2 * c.Da), "old_logp": guarded(n), "last_value": guarded(s),
            "latent_eps": guarded(n, c.Z)}
    cfg = P.PPOConfig(clip_param=0.2, kl_coeff=0.3, entropy_coeff=0.01, vf_clip_param=10.0, lr=V.LR, sgd_minibatch_size=c.max_batch,
                      num_sgd_iter=1, gamma=V.GAMMA, lambda_=V.LAMBDA)
    params = cfg.gae_params(c.log_std_type)
    got = eng.ppo_evaluate(dro, params, eps=deps, noise=c.noise, out={k: v[1] for k, v in bufs.items()})
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
    # the draws that were used come back: the supplied ones under the learned prior, zeros with the noise off -- and
    # under the sphere, where nothing is drawn: other draws, no draws (Philox) and the noise switch change no bit
    drawn = c.prior == W.LEARNED and c.noise
    assert torch.equal(got["latent_eps"].cpu(), eps if drawn else torch.zeros_like(eps))
    if c.prior == W.SPHERE:
        kept = {k: v.clone() for k, v in got.items()}
        for kw in (dict(eps=deps.flip(0).contiguous(), noise=True), dict(eps=None, noise=True, seed=3, offset=7), dict(eps=deps, noise=False)):
            again = eng.ppo_evaluate(dro, params, **kw)
            assert all(torch.equal(again[k], kept[k]) for k in kept), kw
    # prepare straight into learn, the draws replayed row by row: the first step sees its own distribution
    calls = m._st._rng_calls
    batch = m.ppo_prepare({k: v.to(DEV) for k, v in ro.items()}, cfg, eps=deps)
    assert m.engine.gae_launches() == (ev, rest) and m._st._rng_calls == calls + 3        # three chunks, under every prior
    assert all(torch.equal(batch[theirs], got[ours]) for theirs, ours in (("vf_preds", "vf_preds"), ("action_dist_inputs", "old_dist"),
                                                                          ("action_logp", "old_logp"), ("last_value", "last_value")))
    assert torch.equal(batch["latent_eps"].cpu(), eps if drawn else torch.zeros_like(eps))
    steps = -(-n // c.max_batch)
    leps = torch.zeros(steps * c.max_batch, c.Z, device=DEV)
    leps[:n] = deps
    stats = m.ppo_learn(batch, cfg, eps=leps.view(steps, c.max_batch, c.Z))
    assert stats.shape == (steps, 5) and bool(torch.isfinite(stats).all())
    print(name, "first step after prepare", stats[0].tolist())
    assert abs(float(stats[0, 3])) < 2e-4


N_ENVS, T = 3, 8
DONES = np.zeros((N_ENVS, T), dtype=bool)
DONES[0, 2] = DONES[0, T - 1] = DONES[2, 5] = True


@pytest.mark.parametrize("name", ["sphere_z65", "state_mean_pr_layers"])
def test_compute_actions_into_prepare_into_learn(name):
    """The worker iteration of tests/test_gpu_ppo_act.py's whole-loop test from a configuration that sets "ppo_priors": the
    learner's first step runs on the distribution that drew the actions, so its KL stat is 0 and every ratio 1 -- to 2e-4, that
    test's bound on the KL; |ratio - 1| is the difference of two evaluations of logp, which EVAL_BOUND holds to 1e-5 of
    max(|logp|, 1), with |logp| below 20 at the 5 action dimensions and unit standard deviation of these cases."""
    c = W.case(name)
    m = W.module_for(c, DEV)
    assert c.Da == 5 and c.log_std_type == "constant" and N_ENVS * T <= c.max_batch
    g = torch.Generator().manual_seed(9)
    steps = [torch.randn(N_ENVS, 2 * c.Db, generator=g).to(DEV) for _ in range(T)]
    rewards, next_last = torch.rand(N_ENVS, T, generator=g), torch.randn(N_ENVS, 2 * c.Db, generator=g)
    buf = P.RolloutBuffer(N_ENVS, T, 2 * c.Db, c.Da, DEV, latent=c.Z)
    m.seed(5)
    calls = m._st._rng_calls
    for t, obs in enumerate(steps):
        res = m.compute_actions(obs, out=buf, step=t)
        assert res["actions"].data_ptr() == buf.step_view("actions", t).data_ptr()
    assert m._st._rng_calls == calls + T
    assert torch.equal(buf.columns["obs"].view(N_ENVS, T, -1), torch.stack(steps, 1))
    ro = buf.rollout(rewards, DONES, next_last)
    used = ro["latent_eps"]
    assert (float(used.abs().max()) == 0.0) == (c.prior == W.SPHERE)       # the sphere draws nothing
    cfg = P.PPOConfig(gamma=0.98, lambda_=0.95, clip_param=0.2, kl_coeff=0.3, entropy_coeff=0.01, vf_clip_param=10.0, lr=1e-4,
                      sgd_minibatch_size=N_ENVS * T, num_sgd_iter=1)
    batch = m.ppo_prepare(ro, cfg)
    assert m.engine.gae_launches()[0] == 0                                 # the sampler's columns are taken as given
    diag = P.diag_buffer(N_ENVS * T, cfg, DEV)
    stats = m.ppo_learn(batch, cfg, eps=used.view(1, N_ENVS * T, -1), diag_out=diag)
    dev = float(diag[0, P.DIAG.index("ratio_max_dev")])
    print(name, "first step", stats[0].tolist(), "ratio_max_dev", dev)
    assert stats.shape == (1, 5) and bool(torch.isfinite(stats).all())
    assert abs(float(stats[0, 3])) < 2e-4 and dev < 2e-4
    assert c.rows > 4 and m.engine.ppo_launches() == TS.launches(c) + 1    # the documented count, and the diagnostics launch


def test_fused_sphere_step_against_forward_hip_loss_backward():
    """`ppo_sphere_bwd_kernel` (the fused step) and `sampler_bwd_kernel` (`pvae_reparam_backward`, under autograd) share the
    row's arithmetic (`sphere_bwd_row`): the encoder's and the decoder's gradients of the two paths agree within GRAD_BOUND,
    and the encoder's, which only that function separates (the stacks' backward launches are the same in both paths, as
    tests/test_gpu_ppo_vae.py holds them under the default prior), are the same bits."""
    c = W.case("sphere_z65")
    assert c.rows == 33 and c.Z == 65 and c.mask == 7 and not c.gathered and c.log_std_type == "constant"
    m, eng, ve = setup(c)
    used = {k: v.to(DEV) for k, v in c.used.items()}
    logits, _ = m.forward({"obs_flat": used["obs"]}, [], None, eps=c.eps.to(DEV))
    total, stats = P.HipPPOLoss.apply(logits[:, :c.Da], logits[:, c.Da:], m.value_function(), used, TS.CFG.params("constant"), None)
    total.backward()
    auto = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    m, eng, ve = setup(c)
    got = eng.ppo_step(eng.ppo_batch(used), TS.params_of(c, m, 1), 0, c.rows, None, eps=c.eps.to(DEV), noise=c.noise, offset=1)
    assert max_err_scaled(got.cpu(), stats.cpu()) < 1e-5
    worst, same = 0.0, True
    for k, g in TS.buffers(m, "grad").items():
        if not k.startswith("_value_branch."):
            e = max_err_scaled(g.cpu(), auto[k].double().cpu())
            worst, same = max(worst, e), same and torch.equal(g, auto[k])
            assert float(auto[k].abs().max()) > 0 and e < V.GRAD_BOUND, (k, e)
            assert not k.startswith("_task_encoder.") or torch.equal(g, auto[k]), k
    print("fused against autograd under the sphere: worst %.3g, %s" % (worst, "the same bits" if same else "not the same bits"))


def test_a_module_that_did_not_opt_in_is_refused_and_launches_nothing():
    c = W.case("sphere_z65")
    m, eng, ve = setup(c, opt_in=False)
    cfg = P.PPOConfig(lr=V.LR, sgd_minibatch_size=c.rows, num_sgd_iter=1, **F.LOSS)
    rllib = {theirs: c.used[ours].to(DEV) for theirs, ours in P.SAMPLE_BATCH_KEYS.items()}
    with pytest.raises(NotImplementedError, match="hypersphere_uniform"):
        m.ppo_learn(rllib, cfg)
    cols = eng.ppo_batch({k: v.to(DEV) for k, v in c.batch.items()})
    before = TS.state(m)
    with pytest.raises(RuntimeError, match="supports the priors normal_zero_mean_one_std and False, got prior_kind 2"):
        eng.ppo_step(cols, TS.params_of(c, m, 1), 0, c.rows, None, eps=c.eps.to(DEV), offset=1)
    torch.cuda.synchronize()
    assert eng.ppo_launches() == 0 and not TS.same_state(before, TS.state(m))
    assert bool(torch.isnan(eng.workspace).all())                       # not one panel was written
    eng.set_ppo_priors(True)                                            # told: the same context runs
    eng.ppo_step(cols, TS.params_of(c, m, 1), 0, c.rows, None, eps=c.eps.to(DEV), offset=1)
    assert eng.ppo_launches() == TS.launches(c)
