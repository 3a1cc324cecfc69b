"""The step between rollout and SGD of a PPO learner iteration -- bootstrap values, GAE, value targets, standardised
advantages -- timed four ways on the same GPU in one session, at the imitation spec's shapes (train_batch_size 100000 in
fragments of 100, observation 722, 54 actions, the default 256x2 stacks, gamma 0.98, lambda 0.95):
  a  host         RLlib's way: per fragment the numpy recurrence on the host (the sampler's vf_preds and bootstrap values
                  given), standardisation, then the upload of the seven train-batch columns
  b  torch        ppo.gae_torch + ppo.standardize_torch on device tensors (one vectorised step per time offset)
  c  prepare      FullyConnectedPolicy.ppo_prepare with the evaluate pass over the rows (pvae_fc_ppo_prepare)
  d  prepare_given  ppo_prepare with the sampler's vf_preds / action_dist_inputs / action_logp given: bootstrap + GAE +
                  standardisation only
The ways alternate round by round within the session; reported per way: median, min and max over the rounds, in
milliseconds, and the launch counts of (c) and (d).  Prints one JSON line.

    python tools/gae_bench.py [--rows 100000] [--fragment 100] [--rounds 7] [--warmup 2] [--kind constant]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physicsvae_amd import FullyConnectedPolicy                  # noqa: E402
from physicsvae_amd import ppo as P                              # noqa: E402
from physicsvae_amd.spaces import Box                            # noqa: E402

OBS, NUM_OUTPUTS = 722, 108
K = NUM_OUTPUTS // 2


def make_policy(kind, max_batch):
    cmc = {"log_std_type": kind, "device": "cuda", "max_batch": max_batch, "sample_std": 0.3}
    return FullyConnectedPolicy(Box(np.zeros(OBS), np.zeros(OBS)), Box(np.zeros(K), np.zeros(K)), NUM_OUTPUTS,
                                {"custom_model_config": cmc}, "fcnn")


def host_gae(rewards, vf_preds, last_values, seg_start, gamma, lambda_):
    """compute_advantages fragment by fragment, as RLlib's postprocessing does it (numpy; the discounted sum as a reverse
    loop over the fragment's rows), then the standardisation over the batch."""
    adv = np.empty_like(rewards)
    c = gamma * lambda_
    for s in range(len(last_values)):
        a, b = int(seg_start[s]), int(seg_start[s + 1])
        v = np.append(vf_preds[a:b], last_values[s])
        delta = rewards[a:b] + gamma * v[1:] - v[:-1]
        acc = 0.0
        out = np.empty(b - a, dtype=np.float64)
        for t in range(b - a - 1, -1, -1):
            acc = delta[t] + c * acc
            out[t] = acc
        adv[a:b] = out
    vt = adv + vf_preds
    return ((adv - adv.mean()) / max(1e-4, adv.std())).astype(np.float32), vt.astype(np.float32)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--fragment", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-batch", type=int, default=512)
    ap.add_argument("--kind", default="constant", choices=("constant", "state_independent", "state_dependent"))
    a = ap.parse_args()
    assert a.rounds >= 5, "report the median of at least 5 rounds"
    n, frag = a.rows, a.fragment
    cfg = P.PPOConfig(gamma=0.98, lambda_=0.95)
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    m = make_policy(a.kind, a.max_batch)
    # a rollout on the host, as the sampler leaves it: fragments of `frag` rows, every ninth one ends its episode
    host = {"obs": rng.standard_normal((n, OBS), dtype=np.float32), "actions": rng.standard_normal((n, K), dtype=np.float32),
            "rewards": rng.random(n, dtype=np.float32), "vf_preds": rng.standard_normal(n, dtype=np.float32),
            "action_dist_inputs": rng.standard_normal((n, 2 * K), dtype=np.float32) * 0.1,
            "action_logp": rng.standard_normal(n, dtype=np.float32)}
    eps_id = np.arange(n) // frag
    dones = np.zeros(n, dtype=bool)
    dones[frag * 9 - 1::frag * 9] = True
    seg_start, seg_done, next_obs_last = P.segment_table(eps_id, dones, rng.standard_normal((n, OBS), dtype=np.float32))
    last_values = rng.standard_normal(len(seg_done), dtype=np.float32) * (1 - seg_done)
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    table = {"seg_start": torch.from_numpy(seg_start).cuda(), "seg_done": torch.from_numpy(seg_done).cuda(),
             "next_obs_last": torch.from_numpy(next_obs_last).cuda()}
    d_last = torch.from_numpy(last_values).cuda()
    ro_eval = dict({k: dev[k] for k in ("obs", "actions", "rewards")}, **table)
    ro_given = dict(dev, **table)

    def way_a():
        adv, vt = host_gae(host["rewards"], host["vf_preds"], last_values, seg_start, cfg.gamma, cfg.lambda_)
        cols = dict(host, advantages=adv, value_targets=vt)
        return {k: torch.from_numpy(cols[k]).cuda() for k in P.SAMPLE_BATCH_KEYS}

    def way_b():
        adv, vt = P.gae_torch(dev["rewards"], dev["vf_preds"], d_last, table["seg_start"], cfg.gamma, cfg.lambda_)
        return P.standardize_torch(adv), vt

    launches = {}

    def way_c():
        out = m.ppo_prepare(ro_eval, cfg)
        launches["c_prepare"] = m.engine.gae_launches()
        return out

    def way_d():
        out = m.ppo_prepare(ro_given, cfg)
        launches["d_prepare_given"] = m.engine.gae_launches()
        return out

    ways = (("a_host", way_a), ("b_torch", way_b), ("c_prepare", way_c), ("d_prepare_given", way_d))
    for _, fn in ways:
        for _ in range(a.warmup):
            fn()
    times = {name: [] for name, _ in ways}
    for _ in range(a.rounds):                        # the ways alternate within the session
        for name, fn in ways:
            times[name].append(timed(fn))
    # the ways agree on what they compute (d against b: the same inputs but for the bootstrap values)
    b_adv, _ = way_b()
    a_cols = way_a()
    agree = float((a_cols["advantages"] - b_adv).abs().max() / b_adv.abs().max())
    out = {"rows": n, "fragment": frag, "segments": int(len(seg_done)), "obs": OBS, "k": K, "kind": a.kind,
           "max_batch": a.max_batch, "rounds": a.rounds, "a_vs_b_max_err_scaled": agree}
    for name, v in times.items():
        out[name] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
    for name, (ev, rest) in launches.items():
        out[name]["launches"] = {"evaluate": ev, "rest": rest}
    out["d_beats_b"] = out["d_prepare_given"]["median_ms"] < out["b_torch"]["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
