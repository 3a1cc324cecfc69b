"""FullyConnectedPolicy ("fcnn", rmt:323-457) timed three ways on the same GPU in one session:
  grouped    the HIP policy, one launch per layer depth for all stacks (the default schedule)
  per_stack  the HIP policy with pvae_set_option(NULL, "fc_per_stack", 1): one launch per layer per stack
  torch      a plain torch twin (nn.Linear stacks holding the same weights: hipBLAS GEMMs)
on (a) one 500-row PPO-shaped update -- forward, clipped-ratio diagonal-Gaussian log-likelihood + value loss, backward(),
torch.optim.Adam.step() --, (b) one B = 1 `forward` + `value_function` without a graph (the rollout call), and (c) "calls":
the forward and the backward of the stacks alone at 500 rows (the two library calls; the twin: forward + autograd
backward from the same output gradients) -- the part of (a) the schedule can change, without the loss and the optimizer.

Shapes: observation 722, num_outputs 108, the default 256x2 policy / value stacks (+ the 64x2 log-std stack with
--log-std-type state_dependent).  722 is the RUNTIME spec's observation width (data/spec/loco/loco_runtime_physics_vae.yaml);
the imitation spec's own observation width is assembled by its PyBullet environment and cannot be derived without it.

The three ways alternate block by block within the session (`--rounds` rounds of `--steps` calls each), so clock and
thermal drift hit all of them alike; reported per way: median, min and max of the per-round means, in microseconds.
Prints one JSON line.

    python tools/fcnn_bench.py [--rows 500] [--steps 200] [--rounds 7] [--warmup 30] [--log-std-type constant]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physicsvae_amd import FullyConnectedPolicy                  # noqa: E402
from physicsvae_amd.engine import set_fc_per_stack               # noqa: E402
from physicsvae_amd.spaces import Box                            # noqa: E402

OBS, NUM_OUTPUTS = 722, 108


class Twin(nn.Module):
    def __init__(self, m, kind):
        super().__init__()
        sd = m.state_dict()

        def stack(prefix):
            mods, i = [], 0
            while "%s._model.%d._model.0.weight" % (prefix, i) in sd:
                w = sd["%s._model.%d._model.0.weight" % (prefix, i)]
                lin = nn.Linear(w.shape[1], w.shape[0], device="cuda")
                with torch.no_grad():
                    lin.weight.copy_(w)
                    lin.bias.copy_(sd["%s._model.%d._model.0.bias" % (prefix, i)])
                mods += [lin, nn.ReLU()]
                i += 1
            return nn.Sequential(*mods[:-1])
        self.pol, self.val = stack("_policy_fn"), stack("_value_fn")
        self.ls = stack("_log_std_fn") if kind == "state_dependent" else None
        self.log_std = torch.zeros(NUM_OUTPUTS // 2, device="cuda")

    def forward(self, obs):
        mean = self.pol(obs)
        self.cur_value = self.val(obs).squeeze(1)
        ls = self.ls(obs) if self.ls is not None else self.log_std.reshape(1, -1).expand(obs.shape[0], -1)
        return torch.cat([mean, ls], dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--log-std-type", default="constant", choices=["constant", "state_independent", "state_dependent"])
    a = ap.parse_args()
    Da = NUM_OUTPUTS // 2
    torch.manual_seed(0)
    cmc = {"log_std_type": a.log_std_type, "device": "cuda", "max_batch": max(a.rows, 32)}
    m = FullyConnectedPolicy(Box(np.zeros(OBS), np.zeros(OBS)), Box(np.zeros(Da), np.zeros(Da)), NUM_OUTPUTS,
                             {"custom_model_config": cmc}, "fcnn")
    twin = Twin(m, a.log_std_type)
    g = torch.Generator(device="cuda").manual_seed(0)
    obs = torch.randn(a.rows, OBS, device="cuda", generator=g)
    obs1 = obs[:1].contiguous()
    act = 0.1 * torch.randn(a.rows, Da, device="cuda", generator=g)
    adv = torch.randn(a.rows, device="cuda", generator=g)
    ret = torch.randn(a.rows, device="cuda", generator=g)
    with torch.no_grad():
        lg, _ = m.forward({"obs_flat": obs}, [], None)
    old_logp = (-0.5 * (((act - lg[:, :Da]) / torch.exp(lg[:, Da:])) ** 2).sum(1) - lg[:, Da:].sum(1)
                - 0.5 * Da * math.log(2 * math.pi)).detach()
    opt = torch.optim.Adam(m.parameters(), lr=1e-6)
    topt = torch.optim.Adam(twin.parameters(), lr=1e-6)

    def loss_of(logits, value):
        mean, log_std = logits[:, :Da], logits[:, Da:]
        logp = -0.5 * (((act - mean) / torch.exp(log_std)) ** 2).sum(1) - log_std.sum(1) - 0.5 * Da * math.log(2 * math.pi)
        ratio = torch.exp(logp - old_logp)
        return -torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv).mean() + 0.5 * ((value - ret) ** 2).mean()

    def update_hip():
        opt.zero_grad(set_to_none=True)
        logits, _ = m.forward({"obs_flat": obs}, [], None)
        loss_of(logits, m.value_function()).backward()
        opt.step()

    def update_torch():
        topt.zero_grad(set_to_none=True)
        logits = twin(obs)
        loss_of(logits, twin.cur_value).backward()
        topt.step()

    def rollout_hip():
        with torch.no_grad():
            m.forward({"obs_flat": obs1}, [], None)
            return m.value_function()

    def rollout_torch():
        with torch.no_grad():
            twin(obs1)
            return twin.cur_value

    eng = m.engine
    dys = [torch.randn(a.rows, n, device="cuda", generator=g) for n in eng.n_outs]
    gbuf = torch.empty(eng.arena_floats, device="cuda")
    mask = (1 << len(eng.n_outs)) - 1

    def calls_hip():                             # the two library calls of an update alone: no loss, no optimizer, no graph
        eng.forward(obs)
        eng.backward(obs, dys, False, gbuf, mask)

    def calls_torch():
        for p in twin.parameters():
            p.grad = None
        logits = twin(obs)
        torch.autograd.backward([logits[:, :Da], twin.cur_value] + ([logits[:, Da:]] if twin.ls is not None else []),
                                [dys[0], dys[1][:, 0]] + ([dys[2]] if twin.ls is not None else []))

    def grouped(fn):
        def run():
            set_fc_per_stack(False)
            fn()
        return run

    def per_stack(fn):
        def run():
            set_fc_per_stack(True)
            fn()
        return run

    out = {"rows": a.rows, "steps": a.steps, "rounds": a.rounds, "log_std_type": a.log_std_type, "obs": OBS}
    for what, ways in (("calls", (("grouped", grouped(calls_hip)), ("per_stack", per_stack(calls_hip)), ("torch", calls_torch))),
                       ("update", (("grouped", grouped(update_hip)), ("per_stack", per_stack(update_hip)), ("torch", update_torch))),
                       ("rollout_b1", (("grouped", grouped(rollout_hip)), ("per_stack", per_stack(rollout_hip)), ("torch", rollout_torch)))):
        means = {name: [] for name, _ in ways}
        for name, fn in ways:
            for _ in range(a.warmup):
                fn()
        for _ in range(a.rounds):                # the ways alternate within the session
            for name, fn in ways:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                means[name].append((time.perf_counter() - t0) / a.steps * 1e6)
        for name, v in means.items():
            out["%s_%s_us" % (what, name)] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
    set_fc_per_stack(False)
    with torch.no_grad():
        m.forward({"obs_flat": obs}, [], None)
    out["launches_forward"] = m.engine.launches()[0]
    update_hip()
    out["launches_backward"] = m.engine.launches()[1]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
