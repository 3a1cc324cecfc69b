"""The gradient exchange between workers inside the fused PPO learners (include/pvae.h "Gradient exchange between workers"),
timed at the specs' shapes: FullyConnectedPolicy (observation 722, 54 actions, 256x2 stacks; tools/ppo_bench.py) and
PhysicsVAE (2 x 197, 45 actions, latent 32, 256x2 / 512x3 / 256x2; tools/vae_ppo_bench.py), `--rows` rows a minibatch.

  world 1   on one GPU, in one process: `*_ppo_sgd` with a world-1 exchange open (the exchanged Adam launch) against the
            plain loop, blocks of `--steps` steps alternating within the session; per way the median, min and max of the
            per-round means in microseconds per step, and the difference of the medians beside the plain loop's own
            run-to-run range.  Not a production path: informative only.
  world 2, 4   `--worlds`: that many PROCESSES on the GPUs there are (one each while they last, else they share cuda:0) over
            gloo, each on its own batch, `ppo_learn(dp=PPODataParallel(transport="p2p"))` and, for comparison, "torch";
            microseconds per step (the slowest rank), replicas checked bit-identical, waits that gave up.  With the
            processes on ONE GPU the figure is labelled "functional, says nothing about links": every "link" is the
            device's own memory, and the workers' launches share its CUs.  On a multi-GPU node the same command measures
            the links; none has been available to this project.

    python tools/ppo_dp_bench.py [--rows 500] [--steps 100] [--rounds 5] [--warmup 20] [--worlds 2,4] [--out profiles/ppo_dp_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from physicsvae_amd import parallel                                # noqa: E402
from physicsvae_amd import ppo as P                              # noqa: E402


def build(model, rows, seed=0):
    """(module, make_batch(n)) at the spec's shapes, weights from `seed`."""
    torch.manual_seed(seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    mb = max(rows, 32)
    if model == "fcnn":
        import ppo_bench as B
        m = B.make_policy("state_independent", mb)
        return m, lambda n: B.make_batch(m, n, g)
    import vae_ppo_bench as B
    m = B.make_model(mb)
    return m, lambda n: B.make_batch(m, n, g, mb)


def config(rows):
    return P.PPOConfig(clip_param=0.2, kl_coeff=0.0, vf_clip_param=1000.0, lr=1e-6, sgd_minibatch_size=rows, num_sgd_iter=1)


def summary(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def world_one(model, a):
    cfg = config(a.rows)
    plain, _ = build(model, a.rows)
    opened, make_batch = build(model, a.rows)
    batch = make_batch(a.rows * a.steps)
    dp = parallel.PPODataParallel(0, 1, transport="p2p")
    dp.attach(opened)
    ways = (("plain", plain, None), ("exchanged_world_1", opened, dp))
    for _, m, d in ways:
        m.ppo_learn(make_batch(a.rows * a.warmup), cfg, dp=d)
    means = {name: [] for name, _, _ in ways}
    for _ in range(a.rounds):                        # the ways alternate within the session
        for name, m, d in ways:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.ppo_learn(batch, cfg, dp=d)
            torch.cuda.synchronize()
            means[name].append((time.perf_counter() - t0) / a.steps * 1e6)
    res = {name: summary(v) for name, v in means.items()}
    res["exchanged_minus_plain_us"] = round(res["exchanged_world_1"]["median"] - res["plain"]["median"], 1)
    res["plain_run_to_run_range_us"] = round(res["plain"]["max"] - res["plain"]["min"], 1)
    res["launches_per_step"] = [plain.engine.ppo_launches(), opened.engine.ppo_launches()]
    res["waits_that_gave_up"] = dp.timeouts(opened)
    dp.detach(opened)
    return res


def worker(a):
    """One rank of a multi-process run (started by `several`)."""
    rank, world, local = parallel.init_from_env(backend=os.environ.get("PVAE_DIST_BACKEND") or "gloo")
    import torch.distributed as dist
    cfg = config(a.rows)
    m, make_batch = build(a.model, a.rows)
    _, make_own = build(a.model, a.rows, seed=100 + rank)     # this worker's own rows
    dp = parallel.PPODataParallel(rank, world, transport=a.transport)
    dp.attach(m)
    m.ppo_learn(make_own(a.rows * a.warmup), cfg, dp=dp)
    batch = make_own(a.rows * a.steps)
    means = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        m.ppo_learn(batch, cfg, dp=dp)
        torch.cuda.synchronize()
        means.append((time.perf_counter() - t0) / a.steps * 1e6)
    t = torch.tensor(means, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    h = m.engine.params.view(torch.int32).to(torch.int64).sum().reshape(1).cpu()
    hi, lo = h.clone(), h.clone()
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    bad = torch.tensor([dp.timeouts(m) if a.transport == "p2p" else 0], dtype=torch.int64)
    dist.all_reduce(bad, op=dist.ReduceOp.MAX)
    if a.transport == "p2p":
        dp.detach(m)
    if rank == 0:
        res = summary(t.tolist())
        res.update(replicas_identical=int(hi.item()) == int(lo.item()), waits_that_gave_up=int(bad.item()))
        with open(a.worker, "w") as f:
            json.dump(res, f)
    dist.barrier()


def several(model, world, transport, a, port):
    shared = torch.cuda.device_count() < world
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "res.json")
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", PVAE_DIST_BACKEND="gloo")
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", out, "--model", model, "--transport", transport,
               "--rows", str(a.rows), "--steps", str(a.steps), "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
        procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(0 if shared else r)), stdout=subprocess.PIPE,
                                  stderr=subprocess.STDOUT, text=True) for r in range(world)]
        outs = [p.communicate(timeout=900)[0] for p in procs]
        for p, o in zip(procs, outs):
            if p.returncode != 0:
                return {"error": o[-800:]}
        with open(out) as f:
            res = json.load(f)
    res["what"] = "functional, says nothing about links (the processes share one GPU)" if shared else "one GPU per worker"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--worlds", default="2,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_dp_bench.json"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--model", default="fcnn", help=argparse.SUPPRESS)
    ap.add_argument("--transport", default="p2p", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a)
        return
    assert torch.cuda.is_available(), "the exchange runs on a GPU: there is nothing to time without one"
    out = {"rows": a.rows, "steps": a.steps, "rounds": a.rounds, "gpus": torch.cuda.device_count(),
           "link_cost": "not measured: no multi-GPU node has been available; run this tool there"}
    port = 29650
    for model in ("fcnn", "physics_vae"):
        res = {"world_1": world_one(model, a)}
        for world in [int(w) for w in a.worlds.split(",") if w]:
            for transport in ("p2p", "torch"):
                port += 1
                res["world_%d_%s" % (world, transport)] = several(model, world, transport, a, port)
        out[model] = res
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
