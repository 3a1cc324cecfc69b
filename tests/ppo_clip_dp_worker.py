"""Gradient clipping under the workers' gradient exchange, several processes on one GPU (tests/test_gpu_ppo_clip_dp.py): the
cases -- three steps of `ppo_learn(ClippedPPOConfig(...), dp=, diag_out=)` on a stack set and on PhysicsVAE, built from seeds
alone as tests/ppo_dp_worker.py builds them, every rank on rows of its own --, the one-process probes and emulation of a run
(`raw_norms`, `emulate`), and, run as a script, one worker:

    python ppo_clip_dp_worker.py <repository root> <output prefix> <case> <max_norm>     (RANK / WORLD_SIZE / MASTER_* in the environment)
"""
import os
import sys

import torch

import ppo_dp_worker as W

# minibatches of 16 rows, one pass: three steps on every rank, the last minibatch of rank 1 short (9 rows)
CASES = {
    "fc2": dict(model="fcnn", kind="state_independent", n_rows=(48, 41), minibatch=16, passes=1),
    "fc3": dict(model="fcnn", kind="state_dependent", n_rows=(48, 41, 35), minibatch=16, passes=1),
    "vae2": dict(model="vae", kind="state_independent", n_rows=(48, 41), minibatch=16, passes=1),
}


def config(case, max_norm):
    from physicsvae_amd import ppo as P
    return P.ClippedPPOConfig(**dict(W.HYPER, sgd_minibatch_size=case["minibatch"], num_sgd_iter=case["passes"], grad_clip=max_norm))


def make_batches(case, m):
    """tests/ppo_dp_worker.py `make_batches` with rank r's advantages times 1 + r / 2: gradients of clearly different norms,
    so that a threshold between them separates the workers by far more than any rounding."""
    batches, eps = W.make_batches(case, m)
    for r, b in enumerate(batches):
        b["advantages"] = b["advantages"] * (1.0 + 0.5 * r)
    return batches, eps


def _grad_step(case, eng, cols, eps, draws, prm, r, i):
    mb = case["minibatch"]
    first = i * mb
    rows = min(mb, case["n_rows"][r] - first)
    kw = dict(draws, eps=eps[r][0, i, :rows].to(W.DEV)) if draws else {}
    return eng.ppo_grad_step(cols[r], prm, first, rows, **kw)


def _setup(case):
    from physicsvae_amd import ppo as P
    m = W.make_model(case)
    batches, eps = make_batches(case, m)
    params_at, train_ls, draws = W.learner(m, W.config(case))
    cols = [m.engine.ppo_batch(P.batch_columns(W.on_dev(b))) for b in batches]
    return m, cols, eps, params_at, train_ls, draws


def raw_norms(case):
    """[rank r's float64 norm of its own unclipped gradient at step 0], from `*_ppo_grad` on one module: what the test picks
    the threshold between."""
    from physicsvae_amd import ppo as P
    m, cols, eps, params_at, train_ls, draws = _setup(case)
    eng, norms = m.engine, []
    for r in range(len(cols)):
        _, lg = _grad_step(case, eng, cols, eps, draws, params_at(1), r, 0)
        norms.append(float(P.grad_gnorm_torch(eng.ppo_grad_arenas() + ([lg] if train_ls else []))))
    return norms


def emulate(case, coefs):
    """A run of the case's workers in ONE process: per step `*_ppo_grad` with NO clip bound on every rank's minibatch, each
    rank's gradient times its coefficient `coefs[r][i]` (the device's own entry 6 of that worker's run) in float32, the
    rank-ordered float32 mean (`ppo.dp_mean_torch`), `*_ppo_apply(1.0)`.  Returns the state, and [rank r's float64 norm
    of its unclipped gradient per step]."""
    from physicsvae_amd import ppo as P
    m, cols, eps, params_at, train_ls, draws = _setup(case)
    eng = m.engine
    arenas = eng.ppo_grad_arenas()
    world = len(cols)
    raws = [[] for _ in range(world)]
    for i in range(W.steps_of(case)):
        prm = params_at(i + 1)
        grads, ls_grads = [], []
        for r in range(world):
            _, lg = _grad_step(case, eng, cols, eps, draws, prm, r, i)
            raws[r].append(float(P.grad_gnorm_torch(arenas + ([lg] if train_ls else []))))
            c = coefs[r][i].to(W.DEV, torch.float32)
            grads.append([a * c for a in arenas])
            ls_grads.append(lg * c)
        for j, a in enumerate(arenas):
            a.copy_(P.dp_mean_torch([g[j] for g in grads]))
        eng.ppo_apply(prm, 1.0, P.dp_mean_torch(ls_grads) if train_ls else None)
    torch.cuda.synchronize()
    return W.state(m), raws


def main():
    root, out, name, max_norm = sys.argv[1:5]
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    from physicsvae_amd import parallel
    from physicsvae_amd import ppo as P
    rank, world, _ = parallel.init_from_env(backend="gloo")
    import torch.distributed as dist
    case = CASES[name]
    assert world == len(case["n_rows"])
    cfg = config(case, float(max_norm))
    m = W.make_model(case)
    batches, eps = make_batches(case, m)
    dp = parallel.PPODataParallel(rank, world, transport=os.environ.get("PPO_DP_TRANSPORT", "p2p"))
    dp.attach(m)
    dbatch = W.on_dev(batches[rank])
    diag = P.diag_buffer(case["n_rows"][rank], cfg, W.DEV)
    kw = {"eps": eps[rank][0]} if eps[rank] is not None else {}
    stats = m.ppo_learn(dbatch, cfg, dp=dp, diag_out=diag, **kw)
    torch.cuda.synchronize()
    res = {"diag": diag.cpu(), "stats": stats.cpu(), "state": W.state(m), "launches": m.engine.ppo_launches(),
           "timeouts": dp.timeouts(m) if dp.transport == "p2p" else 0, "bound": m.engine.ppo_grad_clip_bound()}
    if dp.transport == "p2p":
        dp.detach(m)
    torch.save(res, out + ".%d" % rank)
    dist.barrier()
    print("DONE", rank)


if __name__ == "__main__":
    main()
