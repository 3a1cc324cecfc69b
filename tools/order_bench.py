"""The `--order` mode of tools/ppo_bench.py and tools/vae_ppo_bench.py: what the minibatch order of a `ppo_learn` call costs.

  order alone   `engine_ppo.ppo_order` (pvae_ppo_order: one launch up to 8192 rows, 1 + ceil(log2(tiles)) above) against what it
                replaces, torch.stack([torch.randperm(n, device=dev) for _ in range(passes)]).to(torch.int32), at (6250 rows,
                20 passes) -- a worker's train batch -- and (50000, 20) -- a single learner's
  whole call    `ppo_learn` on a train batch of `--learn-rows` rows, sgd_minibatch_size 500, 20 passes, with the order made each of
                the ways named by `--order` (philox: perm="philox"; torch: the expression above, made inside the timed call;
                none: perm=None, row order)

The ways alternate within the session, round by round.  A timed sample is as many back-to-back calls as fill `--window-ms`
(counted per way after the warm-up, at least 3), ending in ONE device synchronise (tools/act_bench.py's pattern): a learner
does not read the order, so nothing else drains the stream.  Reported per way: median, min and max over the rounds, in
microseconds per call."""
import math
import statistics
import time

import torch

ORDERS = ("philox", "torch", "none")
SIZES = ((6250, 20), (50000, 20))


def torch_order(n, passes, dev="cuda"):
    return torch.stack([torch.randperm(n, device=dev) for _ in range(passes)]).to(torch.int32)


def add_arguments(ap):
    ap.add_argument("--order", nargs="+", choices=ORDERS, default=None,
                    help="time the minibatch order instead: alone (philox against torch) and the whole ppo_learn call with the "
                         "order made each of these ways, alternating")
    ap.add_argument("--learn-rows", type=int, default=6250, help="--order: rows of the train batch of the whole call")
    ap.add_argument("--window-ms", type=float, default=100.0, help="--order: length of a timed sample")
    ap.add_argument("--out", default=None, help="--order: also write the JSON line to this file")


def timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / inner


def alternate(ways, rounds, window_ms, warmup=3):
    """{name: {median, min, max, calls_per_sample}} of the callables `ways` = [(name, fn)], alternating round by round."""
    inner = {}
    for name, fn in ways:
        for _ in range(warmup):
            fn()
        inner[name] = max(3, math.ceil(window_ms * 1e3 / timed(fn, 3)))
    samples = {name: [] for name, _ in ways}
    for _ in range(rounds):
        for name, fn in ways:
            samples[name].append(timed(fn, inner[name]))
    return {name: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2),
                   "calls_per_sample": inner[name]} for name, v in samples.items()}


def run(model, batch, config, a):
    """The `--order` measurement on `model` (seeded here) and the device train batch `batch` of `a.learn_rows` rows."""
    from physicsvae_amd import engine_ppo
    assert a.rounds >= 5, "report the median of at least 5 rounds"
    dev = model.engine.device
    model.seed(1234)
    out = {"unit": "us per call", "rounds": a.rounds, "window_ms": a.window_ms, "order_alone": {}, "launches": {}}
    for n, passes in SIZES:
        buf = torch.empty(passes, n, dtype=torch.int32, device=dev)
        info = {}
        ways = [("philox", lambda: engine_ppo.ppo_order(n, passes, 1234, 1, dev, out=buf, info=info)),
                ("torch", lambda: torch_order(n, passes, dev))]
        res = alternate(ways, a.rounds, a.window_ms)
        res["philox_over_torch"] = round(res["philox"]["median"] / res["torch"]["median"], 4)
        out["order_alone"]["%dx%d" % (n, passes)] = res
        out["launches"]["%dx%d" % (n, passes)] = info["launches"]
    n = int(batch["actions"].shape[0])
    perm_of = {"philox": lambda: "philox", "torch": lambda: torch_order(n, config.num_sgd_iter, dev), "none": lambda: None}
    ways = [(o, (lambda o=o: model.ppo_learn(batch, config, perm=perm_of[o]()))) for o in a.order]
    res = alternate(ways, a.rounds, a.window_ms, warmup=2)
    for o in a.order:
        res[o]["spread"] = round(res[o]["max"] - res[o]["min"], 2)
    if "philox" in res and "torch" in res:
        res["philox_minus_torch"] = round(res["philox"]["median"] - res["torch"]["median"], 2)
    out["ppo_learn"] = dict(res, rows=n, sgd_minibatch_size=config.sgd_minibatch_size, num_sgd_iter=config.num_sgd_iter)
    return out
