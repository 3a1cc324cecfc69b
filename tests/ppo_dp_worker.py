"""Gradient exchange between workers inside the fused PPO learners, several processes on one GPU
(tests/test_gpu_ppo_dp.py): the cases, what every process builds from seeds alone -- the model, every rank's train batch
(seed 100 + rank) and, for PhysicsVAE, every rank's explicit latent draws (seed 200 + rank) --, the one-process emulation of
a run (`emulate`: per step `*_ppo_grad` on every rank's minibatch, `ppo.dp_mean_torch`, `*_ppo_apply`), and, run as a
script, one worker of a run:

    python ppo_dp_worker.py <repository root> <output prefix> <case> <mode>      (RANK / WORLD_SIZE / MASTER_* in the environment)
"""
import math
import os
import sys
import time

import torch

DEV = "cuda"
FC_OBS, FC_OUT, FC_K = 22, 10, 5
HYPER = dict(clip_param=0.2, kl_coeff=0.3, entropy_coeff=0.01, vf_clip_param=0.7, vf_loss_coeff=0.5, lr=1e-3)
# (131, 185) rows at minibatch 64: three steps a pass on both ranks, the last minibatches 3 rows (the GEMV path) and 57 rows
CASES = {
    "fc2": dict(model="fcnn", kind="state_independent", n_rows=(131, 185), minibatch=64, passes=2),
    "fc3": dict(model="fcnn", kind="state_dependent", n_rows=(150, 150, 150), minibatch=64, passes=1),
    "vae2": dict(model="vae", kind="state_independent", n_rows=(131, 131), minibatch=64, passes=1),
    "vae3": dict(model="vae", kind="constant", n_rows=(150, 150, 150), minibatch=64, passes=1, freeze="_task_encoder"),
}


def config(case):
    from physicsvae_amd import ppo as P
    return P.PPOConfig(**dict(HYPER, sgd_minibatch_size=case["minibatch"], num_sgd_iter=case["passes"]))


def steps_of(case):
    from physicsvae_amd import ppo as P
    return P.dp_steps(case["n_rows"][0], case["minibatch"], case["passes"])


def fc_cmc(kind):
    return {"log_std_type": kind, "sample_std": 0.3}


def make_model(case, seed=21):
    """The same module in every process (the weights come from `seed` alone)."""
    if case["model"] == "fcnn":
        from test_gpu_fcnn import policy
        torch.manual_seed(seed)
        m = policy(fc_cmc(case["kind"]), obs=FC_OBS, num_outputs=FC_OUT, max_batch=64)
        with torch.no_grad():                        # biases off zero
            for k, p in m.named_parameters():
                if k.endswith("bias"):
                    p.copy_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(3)).to(DEV))
        return m
    from test_gpu_ppo_vae import build
    m = build(max_batch=64, log_std_type=case["kind"], seed=seed - 20)
    if case.get("freeze"):
        getattr(m, case["freeze"]).requires_grad_(False)
    return m


def fc_batch(twin, n, seed):
    """A train batch under RLlib's keys (CPU float32) around the twin's current outputs (tests/test_gpu_ppo.py sample_batch)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)                                    # noqa: E731
    obs = rn(n, FC_OBS)
    with torch.no_grad():
        logits = twin(obs)
        value = twin.cur_value
    mean, ls = logits[:, :FC_K], logits[:, FC_K:]
    actions = mean + torch.exp(ls) * rn(n, FC_K)
    logp = -0.5 * (((actions - mean) / torch.exp(ls)) ** 2).sum(1) - ls.sum(1) - 0.5 * FC_K * math.log(2 * math.pi)
    return {"obs": obs, "actions": actions, "action_dist_inputs": torch.cat([mean + 0.02 * rn(n, FC_K), ls + 0.05 * rn(n, FC_K)], 1),
            "action_logp": logp - 0.35 * rn(n), "advantages": rn(n), "value_targets": value + rn(n), "vf_preds": value + rn(n)}


def make_batches(case, m, learns=1):
    """([rank r's train batch], [rank r's draws [learns, steps, minibatch, Z] or None]) -- from the seeds 100 + r, 200 + r and
    the module as `make_model` left it, so every process and the emulation hold the same."""
    n_rows = case["n_rows"]
    if case["model"] == "fcnn":
        from test_gpu_fcnn import Twin
        twin = Twin(m, fc_cmc(case["kind"]))
        return [fc_batch(twin, n, 100 + r) for r, n in enumerate(n_rows)], [None] * len(n_rows)
    from test_gpu_ppo_vae import Twin, sample_batch
    twin = Twin(m)                                   # (float64, as tests/test_gpu_ppo_vae.py samples its batches)
    Db, Da, Z = m.dim_state_body, m.dim_action, m._task_encoder_output_dim
    batches = [sample_batch(twin, n, 100 + r, Db, Da, Z)[0] for r, n in enumerate(n_rows)]
    eps = [torch.randn(learns, steps_of(case), case["minibatch"], Z, generator=torch.Generator().manual_seed(200 + r))
           for r in range(len(n_rows))]
    return batches, eps


def on_dev(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def log_std_vector(m):
    if hasattr(m, "_als"):
        return m._als.log_std
    return m._policy_fn._model[-1].log_std if m._log_std_fn is None else None


def state(m):
    """Everything a step may move, as CPU copies: parameters, Adam's moments, the log-std vector and its moments."""
    eng = m.engine
    out = {"params": eng.params, "m": eng.ppo_m, "v": eng.ppo_v, "log_std": log_std_vector(m),
           "ls_m": eng.ppo_ls_m, "ls_v": eng.ppo_ls_v}
    ve = m.__dict__.get("_value_engine")
    if ve is not None:
        out.update(value_params=ve.params, value_m=ve.ppo_m, value_v=ve.ppo_v)
    return {k: v.detach().cpu().clone() for k, v in out.items() if v is not None}


def same_state(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def learner(m, cfg):
    """(params_at(adam_t), train_ls, draws) as `ppo_learn` forms them; binds the PPO buffers."""
    m._ppo_dp_state()
    if hasattr(m, "_als"):
        train_ls = m._als.type == "state_independent" and m._als.log_std.requires_grad
        mask = m._ppo_train_mask()
        kind, base, tm = ("state_independent" if train_ls else "constant"), 0.0, (0 if mask == 7 else mask)
        draws = dict(noise=bool(m.latent_prior_noise), seed=m._rng_seed, offset=0)
    else:
        kind, base, _, train_ls = m._ppo_log_std()
        mask = m._ppo_train_mask()
        tm = 0 if mask == (1 << len(m.engine.stacks)) - 1 else mask
        draws = {}
    return (lambda t: cfg.params(kind, base, adam_t=t, train_mask=tm)), train_ls, draws


def emulate(case, m, batches, eps, learns=1):
    """A run of the case's workers in ONE process on the module `m`: per step, `ppo_grad_step` on every rank's minibatch
    (the replicas are identical, so one module serves), the gradients averaged with `ppo.dp_mean_torch`, `ppo_apply(1.0)`.
    Returns [rank r's stats [learns * steps, 5]]."""
    from physicsvae_amd import ppo as P
    cfg, eng, mb = config(case), m.engine, case["minibatch"]
    params_at, train_ls, draws = learner(m, cfg)
    arenas = eng.ppo_grad_arenas()
    cols = [eng.ppo_batch(P.batch_columns(on_dev(b))) for b in batches]
    world, per_pass = len(batches), steps_of(case) // case["passes"]
    stats = [[] for _ in range(world)]
    t = m.__dict__.get("_ppo_t", 0)
    for learn in range(learns):
        for i in range(steps_of(case)):
            first = (i % per_pass) * mb
            prm = params_at(t + 1)
            grads, ls_grads = [], []
            for r in range(world):
                rows = min(mb, case["n_rows"][r] - first)
                kw = dict(draws, eps=eps[r][learn, i, :rows].to(DEV)) if draws else {}
                st, lg = eng.ppo_grad_step(cols[r], prm, first, rows, **kw)
                stats[r].append(st.clone())
                grads.append([a.clone() for a in arenas])
                ls_grads.append(lg.clone())
            for j, a in enumerate(arenas):
                a.copy_(P.dp_mean_torch([g[j] for g in grads]))
            eng.ppo_apply(prm, 1.0, P.dp_mean_torch(ls_grads) if train_ls else None)
            t += 1
    m.__dict__["_ppo_t"] = t
    torch.cuda.synchronize()
    return [torch.stack(s).cpu() for s in stats]


def main():
    root, out, name, mode = sys.argv[1:5]
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    from physicsvae_amd import parallel
    rank, world, _ = parallel.init_from_env(backend="gloo")
    import torch.distributed as dist
    case = CASES[name]
    assert world == len(case["n_rows"])
    learns = 2 if mode == "reattach" else 1
    cfg = config(case)
    m = make_model(case)
    batches, eps = make_batches(case, m, learns)
    if rank > 0:                                     # what attach must put right: rank 0's weights and step counter
        with torch.no_grad():
            m.engine.params.mul_(1.0 + 0.05 * rank)
        m.__dict__["_ppo_t"] = 3
    dp = parallel.PPODataParallel(rank, world, transport=os.environ.get("PPO_DP_TRANSPORT", "p2p"))
    dp.attach(m)
    p2p = dp.transport == "p2p"
    if p2p:
        assert m.engine.ppo_peer_status()[:2] == (rank, world)
    if mode == "timeout":
        # rank 0 enters a step its peer never joins: the wait gives up (PVAE_P2P_TIMEOUT_MS), nothing moves, no hang
        dist.barrier()
        before = state(m)
        if rank == 0:
            from physicsvae_amd import ppo as P
            params_at, _, _ = learner(m, cfg)
            m.engine.ppo_step(P.batch_columns(on_dev(batches[0])), params_at(1), 0, case["minibatch"])
            torch.cuda.synchronize()
        res = {"timeouts": dp.timeouts(m), "unmoved": same_state(state(m), before)}
    else:
        dbatch = on_dev(batches[rank])
        stats = []
        for learn in range(learns):
            if learn > 0:
                dp.detach(m)
                if p2p:
                    assert m.engine.ppo_peer_status()[:2] == (0, 0)
                dp.attach(m)
            time.sleep(0.05 * rank)                  # the ranks arrive at different times
            kw = {"eps": eps[rank][learn]} if eps[rank] is not None else {}
            stats.append(m.ppo_learn(dbatch, cfg, dp=dp, **kw))
        torch.cuda.synchronize()
        res = {"state": state(m), "stats": torch.cat(stats).cpu(), "timeouts": dp.timeouts(m) if p2p else 0,
               "t": m.__dict__["_ppo_t"], "launches": m.engine.ppo_launches()}
    if p2p:
        dp.detach(m)
    torch.save(res, out + ".%d" % rank)
    dist.barrier()
    print("DONE", rank)


if __name__ == "__main__":
    main()
