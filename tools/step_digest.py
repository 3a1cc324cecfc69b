"""Digests of everything the PhysicsVAE training step, rollout and autograd entry points compute, for comparing two builds of
the library bit for bit -- the sibling of tools/ppo_digest.py for the supervised trainer's side of the ABI.  One process,
fixed seeds, small shapes that still take every host path: odd dims (Db 13, Da 5, Z 3), widths 17 / 64 / 129, depths 1-3,
rows 1 / 4 / 33 / 64 (the GEMV path, pad rows, two row tiles), both phases, lookahead 1 and 3, both losses, every prior kind,
a helper stack, fused Adam and store + Adam, the backward pass stage by stage, evaluation, the prefetch, direct and
data-parallel steps (the direct step needs Db >= 64, Z % 4 == 0 and first layers on 32-row tiles: Db 68, Z 4, 256 rows, 512
wide; `direct_active` in its scenarios says whether the library took that path), rollout at 1 - 8 rows, the per-stack
forward / backward, the sampler and its backward, one step at 1024 rows x 1024 wide, and the non-default backward schedules
(`schedules`: contexts created under PVAE_PAIR=0, PVAE_SAME_LAYER=0, PVAE_DEFER_ADAM=0 and the last two together, each with
what `pvae_backward_plan` returns beside the digests).  Prints one JSON line: scenario -> output tensor -> sha256 of its raw
bytes (`plan`: the stage list itself, [net, offset, count] per stage).  The library is the in-tree one, or the one PVAE_LIB_PATH names:

    python tools/step_digest.py > new.json;  PVAE_LIB_PATH=/path/to/other/libpvae_gfx950.so python tools/step_digest.py > old.json

The digests belong to one compiler and one pair of builds: they are compared, never pinned.
"""
import contextlib
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from physicsvae_amd import _lib                                  # noqa: E402
from physicsvae_amd import engine as E                           # noqa: E402
from synth_demo import synth_demo                                # noqa: E402

DEV = "cuda"
W, J = _lib.PHASE_WORLD, _lib.PHASE_JOINT
PRIORS = ("normal_zero_mean_one_std", "normal_state_mean_one_std", "hypersphere_uniform", False)


def digest(tensors):
    torch.cuda.synchronize()
    return {name: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
            for name, t in tensors.items() if t is not None}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def normal(rng, *shape):
    return dev(rng.standard_normal(shape).astype(np.float32))


def fill(eng, seed):
    """Weights N(0, 1 / n_in) and small biases into the live entries of the parameter arena; the other arenas zeroed."""
    rng = np.random.default_rng(seed)
    views = eng.named_views()
    with torch.no_grad():
        for a in (eng.params, eng.grads, eng.exp_avg, eng.exp_avg_sq):
            a.zero_()
        for name in sorted(k for k in views if k.endswith("weight")):
            w, b = views[name], views[name[:-len("weight")] + "bias"]
            w.copy_(dev((rng.standard_normal(tuple(w.shape)) / np.sqrt(w.shape[1])).astype(np.float32)))
            b.copy_(dev((0.1 * rng.standard_normal(tuple(b.shape))).astype(np.float32)))


def roomy(a):
    """16 readable bytes behind the last row (what the direct step asks of the demonstration set)."""
    buf = torch.zeros(a.size + 16, dtype=torch.float32, device=DEV)
    out = buf[: a.size].view(a.shape)
    out.copy_(torch.from_numpy(a))
    return out


def bind(eng, episodes):
    """Episodes of the given lengths, concatenated; the windows of an episode are its rows but the last `lookahead`, so the
    window list jumps where one episode ends."""
    e = synth_demo(7, 1, sum(episodes), eng.arch.Db, eng.arch.Da)["episodes"][0]
    starts = np.concatenate([[0], np.cumsum(episodes)[:-1]])
    rows = np.concatenate([np.arange(n - eng.lookahead) + s for s, n in zip(starts, episodes)]).astype(np.int32)
    eng.bind_dataset(roomy(np.stack(e["state_body"]).astype(np.float32)), roomy(np.stack(e["action"]).astype(np.float32)), dev(rows))


def make(Db=13, Da=5, Z=3, te=(17, 1), md=(64, 2), wm=(129, 3), prior=PRIORS[0], mh=None, max_batch=64, lookahead=1, direct=False,
         episodes=(40,) * 6):
    arch = E.Arch(Db, Da, Z, te=te, md=md, wm=wm, prior=prior, pr=(17, 2) if prior == PRIORS[1] else None, mh=mh)
    eng = E.HipEngine(arch, max_batch, device=DEV, lookahead=lookahead)
    if direct:
        eng.set_direct(True)
    bind(eng, episodes)
    return eng


def params_of(phase, loss="MSE", helper_t=1, t=1):
    adam_t = [t] * _lib.NUM_NETS
    adam_t[_lib.NET_MH] = helper_t * t
    world = phase == W
    return E.make_step_params(1e-3, adam_t=adam_t, a_rec=1.0, kl=0.5, s_rec=1.0 if world else 0.0, cyc=0.1, seed=11, offset=5,
                              loss=loss, weight_decay=0.01)


def state(eng, rows, loss=None):
    """The loss terms, the four arenas and every tensor pvae_read_tensor serves (of every unrolled step)."""
    out = {"loss": loss, "params": eng.params, "m": eng.exp_avg, "v": eng.exp_avg_sq, "grads": eng.grads}
    names = ["mu", "z", "a_hat", "s2_hat", "eps"]
    if eng.arch.prior in PRIORS[:2]:
        names.append("logvar")
    if eng.arch.prior == PRIORS[1]:
        names.append("prior_mu")
    for t in range(eng.lookahead):
        for n in names:
            out["%s[%d]" % (n, t)] = eng.read(n, rows, t)
    return digest(out)


def eps_for(eng, rows, seed=3):
    return normal(np.random.default_rng(seed), eng.lookahead, rows, eng.arch.Z)


def steps(out):
    for look in (1, 3):
        eng = make(lookahead=look)
        for rows in (1, 4, 33, 64):
            for phase in (W, J):
                for loss in ("MSE", "L1"):
                    for fused in (True, False):
                        fill(eng, 1)
                        eng.gather(9, rows)
                        l = eng.forward_backward(phase, rows, params_of(phase, loss), eps_for(eng, rows), fused_adam=fused,
                                                 loss_out=torch.zeros(5, device=DEV))
                        out["step look%d rows%d phase%d %s fused%d" % (look, rows, phase, loss, fused)] = state(eng, rows, l)
        for phase in (W, J):
            sp = params_of(phase)
            nets = [_lib.NET_WM] if phase == W else [_lib.NET_TE, _lib.NET_MD]
            # store + pvae_adam
            fill(eng, 2)
            eng.gather(0, 33)
            l = eng.forward_backward(phase, 33, sp, None, fused_adam=False, loss_out=torch.zeros(5, device=DEV))
            eng.adam(nets, sp)
            out["store+adam look%d phase%d" % (look, phase)] = state(eng, 33, l)
            # the backward pass stage by stage, pvae_adam_segment on each finished slice
            fill(eng, 2)
            eng.gather(0, 33)
            eng.forward_seed(phase, 33, sp, None)
            l, k, n = torch.zeros(5, device=DEV), 0, 1
            while k < n:
                seg, net, n = eng.backward_stage(phase, 33, sp, k, l)
                if seg is not None:
                    eng.adam_segment(net, seg[0], seg[1], sp)
                k += 1
            out["stages+adam_segment look%d phase%d" % (look, phase)] = dict(
                state(eng, 33, l), plan=hashlib.sha256(repr(eng.backward_plan(phase, sp)).encode()).hexdigest())
            # evaluation
            fill(eng, 2)
            eng.gather(5, 33)
            l = eng.forward_backward(phase, 33, sp, eps_for(eng, 33), backward=False, loss_out=torch.zeros(5, device=DEV))
            out["evaluate look%d phase%d" % (look, phase)] = state(eng, 33, l)
            # explicit batch
            fill(eng, 2)
            rng = np.random.default_rng(4)
            eng.set_batch(normal(rng, 33, look, 2 * eng.arch.Db), normal(rng, 33, look, eng.arch.Da))
            l = eng.forward_backward(phase, 33, sp, None, fused_adam=True, loss_out=torch.zeros(5, device=DEV))
            out["set_batch look%d phase%d" % (look, phase)] = state(eng, 33, l)


def priors_and_helper(out):
    for prior in PRIORS:
        eng = make(prior=prior)
        for fused in (True, False):
            fill(eng, 5)
            eng.gather(3, 33)
            l = eng.forward_backward(J, 33, params_of(J), eps_for(eng, 33), fused_adam=fused, loss_out=torch.zeros(5, device=DEV))
            out["prior_%s fused%d" % (prior, fused)] = state(eng, 33, l)
    for look in (1, 3):
        eng = make(mh=(17, 1), lookahead=look)
        for trained in (1, 0):
            for phase in (W, J):
                fill(eng, 6)
                eng.gather(3, 33)
                l = eng.forward_backward(phase, 33, params_of(phase, helper_t=trained), None, fused_adam=True,
                                         loss_out=torch.zeros(5, device=DEV))
                out["helper look%d trained%d phase%d" % (look, trained, phase)] = state(eng, 33, l)


def train_steps(out):
    """pvae_train_step / _prefetch / pvae_dp_train_step, staged (33 rows of 39-window episodes) and direct (256 rows of
    episodes with 299, 99 and 299 windows).  A minibatch with one episode jump inside it (windows 30 .. 62; 100 .. 355) can be
    read where it lies, one with two (30 .. 93; 250 .. 505) falls back to staging; consecutive minibatches `stride` apart."""
    for direct in (False, True):
        eng = make(Db=68, Z=4, te=(512, 1), md=(512, 2), wm=(512, 1), max_batch=256, direct=True, episodes=(300, 100, 300)) \
            if direct else make()
        tag = "direct" if direct else "staged"
        rows, stride, one_jump, two_jumps = (256, 100, 100, 250) if direct else (33, 33, 30, 30)
        for phase in (W, J):
            sp = params_of(phase)
            active = {"direct_active": int(eng.direct_active(phase, rows, sp))}
            for jumps, first, n in ((1, one_jump, rows), (2, two_jumps, rows if direct else 64)):
                fill(eng, 7)
                l = eng.train_step(phase, first, n, sp, eps_for(eng, n), loss_out=torch.zeros(5, device=DEV))
                out["train_step %s phase%d jumps%d" % (tag, phase, jumps)] = dict(state(eng, n, l), **active)
            fill(eng, 7)                    # three consecutive minibatches: the panels flip twice
            ls = []
            for k in range(3):
                ls.append(eng.train_step(phase, stride * k, rows, params_of(phase, t=k + 1), eps_for(eng, rows, k),
                                         loss_out=torch.zeros(5, device=DEV), next_span=(stride * (k + 1), rows)))
            out["prefetch %s phase%d" % (tag, phase)] = state(eng, rows, torch.cat(ls))
        eng.comm_init(0, 1, eng.comm_unique_id())
        for phase in (W, J):
            fill(eng, 8)
            ls = []
            for k, n in enumerate((rows, rows, 0, rows)):
                ls.append(eng.dp_train_step(phase, stride * k, n, params_of(phase, t=k + 1), eps_for(eng, rows, k) if n else None,
                                            loss_out=torch.zeros(5, device=DEV), next_span=(stride * (k + 1), rows)).clone())
            out["dp_train_step %s phase%d" % (tag, phase)] = state(eng, rows, torch.cat(ls))
        eng.comm_destroy()


def rollout(out):
    rng = np.random.default_rng(9)
    for fused in (1, 0):
        _lib.check(_lib.load().pvae_set_option(None, b"rollout_fused", fused), "rollout_fused")
        for mh in (None, (17, 1)):
            eng = make(mh=mh)
            fill(eng, 10)
            log_std = normal(rng, eng.arch.Da)
            for rows in (1, 2, 4, 8):
                obs, eps = normal(rng, rows, 2 * eng.arch.Db), normal(rng, rows, eng.arch.Z)
                for want_s2 in (False, True):
                    a, s2, z = eng.infer(obs, eps=eps, want_s2=want_s2)
                    lg, s2l, zl = eng.infer_logits(obs, log_std, noise=True, seed=3, offset=rows, want_s2=want_s2)
                    a0, _, z0 = eng.infer(obs, noise=False, want_s2=want_s2)
                    out["infer fused%d helper%d rows%d s2%d" % (fused, mh is not None, rows, want_s2)] = digest(
                        {"a_hat": a, "s2_hat": s2, "z": z, "logits": lg, "s2_hat_logits": s2l, "z_logits": zl, "a_hat_mean": a0,
                         "z_mean": z0, "mu": eng.read("mu", rows), "eps": eng.read("eps", rows)})
    eng = make()
    layers = [(normal(rng, 17, 26), normal(rng, 17)), (normal(rng, 64, 17), normal(rng, 64)), (normal(rng, 1, 64), normal(rng, 1))]
    for rows in (1, 5, 33):
        x = normal(rng, rows, 26)
        out["mlp_forward rows%d" % rows] = digest({"relu": eng.mlp_forward(x, layers), "tanh_out": eng.mlp_forward(x, layers, "tanh", "tanh")})


def autograd(out):
    rng = np.random.default_rng(12)
    eng = make(mh=(17, 1))
    fill(eng, 13)
    for net in (_lib.NET_TE, _lib.NET_MD, _lib.NET_WM, _lib.NET_MH):
        n_out = [l for l in eng.layers if l["net"] == net][-1]["n_out"]
        for rows in (3, 33):
            x, dy = normal(rng, rows, eng.net_in_width(net)), normal(rng, rows, n_out)
            res = {"y": eng.net_forward(net, x)}
            for want_dx in (False, True):
                grad = 0.5 * torch.ones(eng.segments[net][1], device=DEV)
                for accumulate in (False, True):
                    res["dx dx%d acc%d" % (want_dx, accumulate)] = eng.net_backward(net, x, dy, want_dx, grad, accumulate)
                    res["grad dx%d acc%d" % (want_dx, accumulate)] = grad.clone()
            res["dx only"] = eng.net_backward(net, x, dy, True)
            out["net net%d rows%d" % (net, rows)] = digest(res)
    for prior in PRIORS:
        eng = make(prior=prior)
        for rows in (3, 33):
            ml, eps, dz = normal(rng, rows, eng.arch.te_out), normal(rng, rows, eng.arch.Z), normal(rng, rows, eng.arch.Z)
            res = {"z_eps": eng.reparam(ml, eps=eps), "z_philox": eng.reparam(ml, seed=5, offset=2), "z_mean": eng.reparam(ml, noise=False)}
            res["eps_used"] = eng.read("eps", rows).clone()
            used = eps if prior in PRIORS[:2] else None
            res["d_ml"] = eng.reparam_backward(ml, used, dz)
            res["d_ml_mean"] = eng.reparam_backward(ml, None, dz, noise=False)
            out["reparam prior_%s rows%d" % (prior, rows)] = digest(res)


def wide(out):
    """1024 rows, two hidden layers of 1024: the 64-row tiles, and the deferred-Adam hand-over between narrow and wide launches."""
    eng = make(te=(1024, 2), md=(1024, 2), wm=(1024, 2), max_batch=1024)
    rng = np.random.default_rng(14)
    for phase in (W, J):
        fill(eng, 15)
        eng.set_batch(normal(rng, 1024, 1, 2 * eng.arch.Db), normal(rng, 1024, 1, eng.arch.Da))
        l = eng.forward_backward(phase, 1024, params_of(phase), None, fused_adam=True, loss_out=torch.zeros(5, device=DEV))
        out["wide phase%d" % phase] = state(eng, 1024, l)


SCHEDULES = (("pair0", {"PVAE_PAIR": "0"}), ("same_layer0", {"PVAE_SAME_LAYER": "0"}), ("defer_adam0", {"PVAE_DEFER_ADAM": "0"}),
             ("same_layer0+defer_adam0", {"PVAE_SAME_LAYER": "0", "PVAE_DEFER_ADAM": "0"}))
# hidden layers per stack, every stack once at every depth.  One hidden layer is the shallowest stack a context accepts
# (two layers: with no input gradient its two weight gradients share the last launch), two make the three-layer stack whose
# last layer is a narrow launch in front of a hidden-layer pair, three add a second pair.
DEPTHS = ({"te": (17, 1), "md": (64, 2), "wm": (129, 3)}, {"te": (17, 3), "md": (64, 1), "wm": (129, 2)},
          {"te": (17, 2), "md": (64, 3), "wm": (129, 1)})


@contextlib.contextmanager
def context_env(env):
    """The per-context switches as `_lib.apply_context_options` reads them: a context created inside keeps them."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def schedules(out):
    """The three non-default schedules of plan_backward_net (unpaired, one behind with and without a gradient arena's
    deferral) and what they make of the unroll, at the small shapes: both phases, lookahead 1 and 3, fused Adam and store,
    33 and 64 rows, every stack at every depth, a helper stack trained and frozen, a learned prior (a stack without input
    gradient ahead of the encoder), the zero-mean prior of the default model (the seeded first-layer input gradients and,
    one behind, the weight gradient carried from the decoder's plan into the encoder's), and the direct step wherever
    the schedule admits it (`direct_active`)."""
    def step(eng, tag, phase, rows, fused, seed, **kw):
        sp = params_of(phase, **kw)
        fill(eng, seed)
        eng.gather(3, rows)
        l = eng.forward_backward(phase, rows, sp, eps_for(eng, rows), fused_adam=fused, loss_out=torch.zeros(5, device=DEV))
        out[tag] = dict(state(eng, rows, l), plan=[list(s) for s in eng.backward_plan(phase, sp)])

    for name, env in SCHEDULES:
        with context_env(env):
            for look in (1, 3):
                for d, depths in enumerate(DEPTHS):
                    eng = make(lookahead=look, **depths)
                    for rows in (33, 64):
                        for phase in (W, J):
                            for fused in (True, False):
                                step(eng, "schedule %s look%d depths%d rows%d phase%d fused%d" % (name, look, d, rows, phase, fused),
                                     phase, rows, fused, 16)
                eng = make(mh=(17, 1), lookahead=look)
                for trained in (1, 0):
                    for phase in (W, J):
                        for fused in (True, False):
                            step(eng, "schedule %s look%d helper trained%d phase%d fused%d" % (name, look, trained, phase, fused),
                                 phase, 33, fused, 17, helper_t=trained)
            eng = make(prior=PRIORS[1])
            for fused in (True, False):
                step(eng, "schedule %s learned_prior fused%d" % (name, fused), J, 33, fused, 18)
            # the direct step (train_steps' shapes): taken where the schedule pairs same-layer and, fused, can defer Adam
            eng = make(Db=68, Z=4, te=(512, 1), md=(512, 2), wm=(512, 1), max_batch=256, direct=True, episodes=(300, 100, 300))
            for phase in (W, J):
                sp = params_of(phase)
                fill(eng, 19)
                l = eng.train_step(phase, 100, 256, sp, eps_for(eng, 256), loss_out=torch.zeros(5, device=DEV))
                out["schedule %s direct train_step phase%d" % (name, phase)] = dict(
                    state(eng, 256, l), plan=[list(s) for s in eng.backward_plan(phase, sp)],
                    direct_active=int(eng.direct_active(phase, 256, sp)), direct_active_store=int(eng.direct_active(phase, 256, sp, fused=False)))
            if eng.direct_active(W, 256, params_of(W), fused=False):      # (the data-parallel step stores its gradients)
                eng.comm_init(0, 1, eng.comm_unique_id())
                for phase in (W, J):
                    fill(eng, 19)
                    l = eng.dp_train_step(phase, 100, 256, params_of(phase), eps_for(eng, 256), loss_out=torch.zeros(5, device=DEV),
                                          next_span=(200, 256)).clone()
                    out["schedule %s direct dp_train_step phase%d" % (name, phase)] = state(eng, 256, l)
                eng.comm_destroy()


def main():
    assert torch.cuda.is_available(), "the digests are of what the GPU computes: there is nothing to report without one"
    out = {}
    sys.stdout.flush()
    stdout = os.dup(1)                      # (RCCL greets on the C level's stdout: only the JSON line goes there)
    os.dup2(2, 1)
    try:
        for scenario in (steps, priors_and_helper, train_steps, rollout, autograd, wide, schedules):
            scenario(out)
    finally:
        os.dup2(stdout, 1)
        os.close(stdout)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
