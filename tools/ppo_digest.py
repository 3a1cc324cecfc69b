"""Digests of everything the on-device PPO learner computes, for comparing two builds of the library bit for bit: in one
process, with fixed seeds, every entry point that runs the learner's kernels (the fused steps of the stack set and of
PhysicsVAE -- the whole learn, single steps, and gradient + apply --, `pvae_ppo_loss`, `pvae_gae`, evaluate, prepare and
the action sampling of both models) at the smallest shapes that still take every path -- k 5 (a padded column-sum stride),
70 rows in minibatches of 33 (a two-tile step with pad rows and a 4-row step on the GEMV / zero-rows path), segments of 1,
63, 64, 65 and 130 rows (a piece boundary and a carry), 70 rows in 40 segments at max_batch 32 (more than one chunk in the
rows pass and in the bootstrap pass, the last one short; the action sampling scatters its 70 rows over 80).  Only the
engines' public methods are called, so the same file runs in an older tree.  Prints one JSON line:
scenario -> output tensor -> sha256 of its raw bytes.  The library is the in-tree one, or the one PVAE_LIB_PATH names:

    python tools/ppo_digest.py > new.json;  PVAE_LIB_PATH=/path/to/other/libpvae_gfx950.so python tools/ppo_digest.py > old.json

Two builds that launch the same kernels in the same order with the same arithmetic print the same line.  The digests belong
to one compiler and one pair of builds: they are compared, never pinned.

`--diag` binds a learner-diagnostics buffer (`ppo_diag`) on every engine of the learner scenarios and adds its rows to
their digests under "diag": every other digest must then be the one printed without the flag.

`--order none` (the default) leaves every scenario on its hand-made `perm` (numpy permutations from the scenario's seed):
the line is the one printed without the flag.  `--order philox` draws every `perm` of the sgd and step scenarios on the
device instead (`ppo_order` at seed 11, offset 5; a library without `pvae_ppo_order` cannot run it) and adds the scenario
"order": the order itself at 70, 8192, 8193 and 20000 rows -- one workgroup in LDS, and tiles with one and two merge
launches.

`--grad-clip X` adds the learner scenarios (the sgd loops, the single steps and gradient + apply of both models) once more
with global-norm gradient clipping bound at max_norm X (`ppo_grad_clip`), under names that start with "clip": every other
digest is the one printed without the flag.  A library without `pvae_fc_ppo_grad_clip` cannot run it.

`--priors` adds PhysicsVAE's scenarios (the sgd loop, the single steps, gradient + apply, evaluate, prepare and the action
sampling) once more under the learned prior ("normal_state_mean_one_std") and the sphere prior ("hypersphere_uniform") on
engines that opted in (`set_ppo_priors`), under names that start with "prior_": every other digest is the one printed
without the flag.  A library without the option "ppo_priors" cannot run it.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physicsvae_amd import engine as E                           # noqa: E402
from physicsvae_amd import ppo as P                              # noqa: E402

DEV = "cuda"
K = 5
CFG = P.PPOConfig(clip_param=0.2, kl_coeff=0.3, entropy_coeff=0.01, vf_clip_param=0.7, vf_loss_coeff=0.5, lr=1e-3,
                  gamma=0.98, lambda_=0.95)
DIAG = False                                                     # set by main() from `--diag`
ORDER = "none"                                                   # set by main() from `--order`
CLIP = None                                                      # set by main() for the scenarios `--grad-clip` adds
OLD_PRIORS, NEW_PRIORS = ("normal_zero_mean_one_std", False), ("normal_state_mean_one_std", "hypersphere_uniform")
PRIORS = OLD_PRIORS                                              # set by main() for the scenarios `--priors` adds


def bind_diag(eng):
    """`--diag`: eight zeroed diagnostics rows bound to the engine and kept on it (more than any scenario's steps)."""
    eng.diag_rows = None
    if DIAG:
        eng.diag_rows = torch.zeros(8, P.PPO_DIAG, dtype=torch.float32, device=DEV)
        eng.ppo_diag(eng.diag_rows)
    if CLIP is not None:
        eng.ppo_grad_clip(CLIP)


def digest(tensors):
    torch.cuda.synchronize()
    return {name: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
            for name, t in tensors.items() if t is not None}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def fill(views, rng):
    """Weights N(0, 1 / n_in) and small biases into the live entries of an arena (its pads stay zero)."""
    with torch.no_grad():
        for w, b in views:
            w.copy_(dev((rng.standard_normal(tuple(w.shape)) / np.sqrt(w.shape[1])).astype(np.float32)))
            b.copy_(dev((0.1 * rng.standard_normal(tuple(b.shape))).astype(np.float32)))


def pairs(named):
    names = sorted(k[:-len("weight")] for k in named if k.endswith("weight"))
    return [(named[n + "weight"], named[n + "bias"]) for n in names]


def batch(rng, n, n_in):
    f = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    b = {"obs": f(n, n_in), "actions": f(n, K), "old_dist": np.concatenate([0.3 * f(n, K), -0.5 + 0.1 * f(n, K)], 1),
         "old_logp": -6.0 + f(n), "advantages": f(n), "value_targets": f(n), "vf_preds": f(n)}
    return {k: dev(v) for k, v in b.items()}


def perms(rng, passes, n):
    made = dev(np.stack([rng.permutation(n) for _ in range(passes)]).astype(np.int32))       # (drawn either way: the rng moves alike)
    return E.ppo_order(n, passes, 11, 5, DEV) if ORDER == "philox" else made


def order(out):
    for n, passes in ((70, 2), (8192, 3), (8193, 3), (20000, 2)):
        out["order n%d passes%d" % (n, passes)] = digest({"perm": E.ppo_order(n, passes, 11, 5, DEV),
                                                         "high_words": E.ppo_order(n, passes, 11 << 32, 5 << 32, DEV)})


def rollout(rng, n_in):
    """70 rows in 40 segments (30 of two rows, 10 of one), every fifth segment done."""
    lens = [2] * 30 + [1] * 10
    n, s = sum(lens), len(lens)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)    # noqa: E731
    ro = {"obs": dev(f(n, n_in)), "actions": dev(f(n, K)), "rewards": dev(rng.random(n, dtype=np.float32)),
          "seg_start": torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)),
          "seg_done": dev((np.arange(s) % 5 == 2).astype(np.uint8)), "boot_obs": dev(f(s, n_in))}
    sampler = {"vf_preds": dev(f(n)), "old_dist": dev(np.concatenate([0.3 * f(n, K), -0.5 + 0.1 * f(n, K)], 1)),
               "old_logp": dev(-6.0 + f(n))}
    return ro, sampler


def log_std_vector(rng):
    return dev((-0.5 + 0.1 * rng.standard_normal(K)).astype(np.float32))


def fc_engine(kind, max_batch, rng):
    stacks = [(E.Stack.of((32, 2)), K), (E.Stack.of((16, 2)), 1)] + ([(E.Stack.of((32, 2)), K)] if kind == 2 else [])
    eng = E.StackSetEngine(7, stacks, max_batch, device=DEV)
    for s in range(len(stacks)):
        fill(eng.views(s), rng)
    ls = None if kind == 2 else log_std_vector(rng)
    eng.ppo_bind(ls, kind == 1)
    bind_diag(eng)
    return eng, ls


def fc_sgd(out):
    for kind in (0, 1, 2):
        for with_perm in (False, True):
            for frozen in (False, True):
                rng = np.random.default_rng(100 + kind)
                eng, ls = fc_engine(kind, 64, rng)
                b = batch(rng, 70, 7)
                mask = 0 if not frozen else (5 if kind == 2 else 1)             # frozen: every stack but the value stack (1)
                stats = eng.ppo_sgd(b, CFG.params(kind, -0.5 if kind == 2 else 0.0, adam_t=1, train_mask=mask), 33, 2,
                                    perms(rng, 2, 70) if with_perm else None)
                out["fc_sgd kind%d perm%d value_frozen%d" % (kind, with_perm, frozen)] = digest(
                    {"stats": stats, "params": eng.params, "m": eng.ppo_m, "v": eng.ppo_v, "log_std": ls,
                     "log_std_m": eng.ppo_ls_m, "log_std_v": eng.ppo_ls_v, "diag": eng.diag_rows})


def state(eng, ls, ve=None):
    d = {"params": eng.params, "m": eng.ppo_m, "v": eng.ppo_v, "log_std": ls, "log_std_m": eng.ppo_ls_m, "log_std_v": eng.ppo_ls_v,
         "diag": eng.diag_rows}
    if ve is not None:
        d.update({"value_params": ve.params, "value_m": ve.ppo_m, "value_v": ve.ppo_v})
    return d


def steps(out, name, eng, ls, b, params_at, index, train_ls, ve=None, draws=lambda rows: {}):
    """Single steps (a two-tile one, then the 4-row tail) and, from the state they leave, gradient + apply at half scale."""
    stats = [eng.ppo_step(b, params_at(1), 0, 33, index, **draws(33)), eng.ppo_step(b, params_at(2), 66, 4, index, **draws(4))]
    out["%s_step %s" % name] = digest(dict(state(eng, ls, ve), stats=torch.stack(stats)))
    one, ls_grad = eng.ppo_grad_step(b, params_at(3), 33, 33, index, **draws(33))
    grads = {"grad%d" % i: g.clone() for i, g in enumerate(eng.ppo_grad_arenas())}
    eng.ppo_apply(params_at(3), 0.5, ls_grad if train_ls else None)
    out["%s_grad_apply %s" % name] = digest(dict(state(eng, ls, ve), stats=one, ls_grad=ls_grad, **grads))


def fc_steps(out):
    for kind in (0, 1, 2):
        for with_index in (False, True):
            rng = np.random.default_rng(700 + kind)
            eng, ls = fc_engine(kind, 64, rng)
            b = batch(rng, 70, 7)
            params_at = lambda t: CFG.params(kind, -0.5 if kind == 2 else 0.0, adam_t=t)      # noqa: E731
            steps(out, ("fc", "kind%d index%d" % (kind, with_index)), eng, ls, b, params_at,
                  perms(rng, 1, 70)[0].contiguous() if with_index else None, kind == 1)


def act_columns(n_dst, n_in, latent=None):
    """Zeroed destination columns of `ppo_act` (the rows no input row is scattered to stay as they are)."""
    widths = {"actions": K, "env_actions": K, "old_dist": 2 * K, "old_logp": None, "vf_preds": None, "action_noise": K, "obs": n_in}
    if latent is not None:
        widths["latent_eps"] = latent
    return {name: torch.zeros((n_dst,) if w is None else (n_dst, w), dtype=torch.float32, device=DEV) for name, w in widths.items()}


def act(out, name, eng, gp, rng, n_in, latent=None):
    """70 rows at max_batch 32: three chunks.  Philox and supplied noise; in row order and scattered over 80 rows."""
    obs = dev(rng.standard_normal((70, n_in)).astype(np.float32))
    noise = dev(rng.standard_normal((70, K)).astype(np.float32))
    rows = dev((rng.permutation(76)[:70] + 2).astype(np.int32))
    for supplied in (False, True):
        kw = {"noise": noise if supplied else None}
        if latent is not None:
            kw["eps"] = dev(rng.standard_normal((70, latent)).astype(np.float32)) if supplied else None
        out["%s_act %s supplied%d" % (name[0], name[1], supplied)] = digest(
            eng.ppo_act(obs, gp, clip=(-0.5, 0.5), seed=11, offset=5, **kw))
        out["%s_act %s supplied%d scatter" % (name[0], name[1], supplied)] = digest(
            eng.ppo_act(obs, gp, clip=(-0.5, 0.5), seed=11, offset=5, out=act_columns(80, n_in, latent), out_row=rows, **kw))
    out["%s_act %s greedy" % name] = digest(eng.ppo_act(obs, gp, explore=False, seed=11, offset=5))


def fc_act(out):
    for kind in (0, 2):
        rng = np.random.default_rng(800 + kind)
        eng, _ = fc_engine(kind, 32, rng)
        act(out, ("fc", "kind%d" % kind), eng, CFG.gae_params(kind, -0.5 if kind == 2 else 0.0), rng, 7)


def loss(out):
    rng = np.random.default_rng(200)
    b = batch(rng, 40, 7)
    del b["obs"]
    for rows in (3, 33):
        mean, value = dev(0.3 * rng.standard_normal((rows, K)).astype(np.float32)), dev(rng.standard_normal(rows).astype(np.float32))
        per_row, vec = dev((-0.5 + 0.1 * rng.standard_normal((rows, K))).astype(np.float32)), log_std_vector(rng)
        index = dev(rng.integers(0, 40, rows).astype(np.int32))
        for with_index in (False, True):
            for broadcast in (False, True):
                ls = vec.expand(rows, K) if broadcast else per_row
                stats, d_mean, d_ls, d_value = E.ppo_loss(mean, ls, value, b, CFG.params(0), index if with_index else None)
                out["loss rows%d index%d broadcast%d" % (rows, with_index, broadcast)] = digest(
                    {"stats": stats, "d_mean": d_mean, "d_log_std": d_ls, "d_value": d_value})


def gae(out):
    rng = np.random.default_rng(300)
    lens = [1, 63, 64, 65, 130]
    n = sum(lens)
    seg = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
    rewards, vf = dev(rng.random(n, dtype=np.float32)), dev(rng.standard_normal(n).astype(np.float32))
    last, done = dev(rng.standard_normal(len(lens)).astype(np.float32)), dev(np.array([0, 1, 0, 0, 1], dtype=np.uint8))
    for with_done in (False, True):
        for standardize in (False, True):
            adv, vt = E.gae(rewards, vf, last, seg, CFG.gamma, CFG.lambda_, standardize, done if with_done else None)
            out["gae done%d standardize%d" % (with_done, standardize)] = digest({"advantages": adv, "value_targets": vt})


def fc_prepare(out):
    for kind in (0, 2):
        rng = np.random.default_rng(400 + kind)
        eng, _ = fc_engine(kind, 32, rng)
        ro, sampler = rollout(rng, 7)
        gp = CFG.gae_params(kind, -0.5 if kind == 2 else 0.0)
        out["fc_evaluate kind%d" % kind] = digest(eng.ppo_evaluate(ro, gp))
        out["fc_prepare kind%d" % kind] = digest(eng.ppo_prepare(ro, gp))
        out["fc_prepare_given kind%d" % kind] = digest(eng.ppo_prepare(dict(ro, **sampler), gp))


def vae_engine(prior, kind, max_batch, rng):
    arch = E.Arch(6, K, 4, te=(32, 2), md=(32, 2), wm=(16, 1), prior=prior)
    eng = E.HipEngine(arch, max_batch, device=DEV)
    if prior in NEW_PRIORS:
        eng.set_ppo_priors(True)
    fill(pairs(eng.named_views()), rng)
    ve = E.StackSetEngine(12, [(E.Stack.of((16, 2)), 1)], max_batch, device=DEV)
    fill(ve.views(0), rng)
    ls = log_std_vector(rng)
    eng.ppo_bind(ve, ls, kind == 1)
    bind_diag(eng)
    return eng, ve, ls


def vae_sgd(out):
    for prior in PRIORS:
        for kind in (0, 1):
            for with_eps in (False, True):
                for mask in (7, 3, 4):
                    rng = np.random.default_rng(500 + kind)
                    eng, ve, ls = vae_engine(prior, kind, 64, rng)
                    b = batch(rng, 70, 12)
                    eps = dev(rng.standard_normal((6, 33, 4)).astype(np.float32)) if with_eps else None
                    stats = eng.ppo_sgd(b, CFG.params(kind, 0.0, adam_t=1, train_mask=mask), 33, 2, perms(rng, 2, 70), eps=eps,
                                        noise=True, seed=11, offset=5)
                    out["vae_sgd prior_%s kind%d eps%d mask%d" % (prior, kind, with_eps, mask)] = digest(
                        {"stats": stats, "params": eng.params, "m": eng.ppo_m, "v": eng.ppo_v, "value_params": ve.params,
                         "value_m": ve.ppo_m, "value_v": ve.ppo_v, "log_std": ls, "log_std_m": eng.ppo_ls_m,
                         "log_std_v": eng.ppo_ls_v, "diag": eng.diag_rows})


def vae_prepare(out):
    for prior in PRIORS:
        rng = np.random.default_rng(600)
        eng, _, _ = vae_engine(prior, 0, 32, rng)
        ro, sampler = rollout(rng, 12)
        gp = CFG.gae_params(0)
        eps = dev(rng.standard_normal((70, 4)).astype(np.float32))
        out["vae_evaluate prior_%s" % prior] = digest(eng.ppo_evaluate(ro, gp, noise=True, seed=11, offset=5))
        out["vae_prepare prior_%s" % prior] = digest(eng.ppo_prepare(ro, gp, eps=eps))
        out["vae_prepare_given prior_%s" % prior] = digest(eng.ppo_prepare(dict(ro, **sampler), gp))


def vae_steps(out):
    for prior in PRIORS:
        for kind in (0, 1):
            for with_eps in (False, True):
                rng = np.random.default_rng(900 + kind)
                eng, ve, ls = vae_engine(prior, kind, 64, rng)
                b = batch(rng, 70, 12)
                eps = dev(rng.standard_normal((33, 4)).astype(np.float32))
                draws = lambda rows: dict(eps=eps[:rows].contiguous() if with_eps else None, noise=True, seed=11, offset=5)   # noqa: E731
                steps(out, ("vae", "prior_%s kind%d eps%d" % (prior, kind, with_eps)), eng, ls, b,
                      lambda t: CFG.params(kind, 0.0, adam_t=t), perms(rng, 1, 70)[0].contiguous(), kind == 1, ve, draws)


def vae_act(out):
    for prior in PRIORS:
        rng = np.random.default_rng(1000)
        eng, _, _ = vae_engine(prior, 0, 32, rng)
        act(out, ("vae", "prior_%s" % prior), eng, CFG.gae_params(0), rng, 12, latent=4)


def main():
    global DIAG, ORDER, CLIP, PRIORS
    ap = argparse.ArgumentParser()
    ap.add_argument("--diag", action="store_true")
    ap.add_argument("--order", choices=("philox", "none"), default="none")
    ap.add_argument("--grad-clip", type=float, default=None)
    ap.add_argument("--priors", action="store_true")
    a = ap.parse_args()
    DIAG, ORDER = a.diag, a.order
    assert torch.cuda.is_available(), "the digests are of what the GPU computes: there is nothing to report without one"
    out = {}
    for scenario in (fc_sgd, fc_steps, fc_act, loss, gae, fc_prepare, vae_sgd, vae_steps, vae_act, vae_prepare) + (
            (order,) if ORDER == "philox" else ()):
        scenario(out)
    if a.grad_clip is not None:
        CLIP, clipped = a.grad_clip, {}
        for scenario in (fc_sgd, fc_steps, vae_sgd, vae_steps):
            scenario(clipped)
        out.update({"clip%g %s" % (CLIP, name): d for name, d in clipped.items()})
    if a.priors:
        CLIP, PRIORS, opted = None, NEW_PRIORS, {}
        for scenario in (vae_sgd, vae_steps, vae_act, vae_prepare):
            scenario(opted)
        out.update({"prior_" + name: d for name, d in opted.items()})
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
