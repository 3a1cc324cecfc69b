"""One PPO-shaped update of PhysicsVAE at the runtime spec's shapes (data/spec/loco/loco_runtime_physics_vae.yaml:
sgd_minibatch_size 500; Db 361, Da 54, Z 32, TE 256x2, MD 512x3, WM 1024x2, rmt:462-510): forward, clipped-ratio Gaussian
log-likelihood + value loss, backward(), torch.optim.Adam.step(), timed two ways on the same GPU:
  (a) hip    PhysicsVAE.forward under autograd: the arena stacks on the HIP kernels (physicsvae_amd/autograd.py)
  (b) torch  the same module's torch sub-modules called directly (m._task_encoder(x), ...: hipBLAS GEMMs)
and the kernel launches per update of each (torch.profiler).  Prints one JSON line.

    python tools/autograd_bench.py [--rows 500] [--steps 50] [--warmup 10]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import refpath as R                      # noqa: E402
from physicsvae_amd.model import PhysicsVAE          # noqa: E402
from physicsvae_amd.spaces import Box                # noqa: E402


def build(rows):
    Db, Da, Z = 361, 54, 32
    arch = R.make_arch(Db, Da, latent=Z, te=(256, 2), md=(512, 3), wm=(1024, 2))
    cmc = dict(observation_space=Box(np.zeros(2 * Db), np.zeros(2 * Db)), observation_space_body=Box(np.zeros(Db), np.zeros(Db)),
               observation_space_task=Box(np.zeros(Db), np.zeros(Db)), action_space=Box(np.zeros(Da), np.zeros(Da)),
               task_encoder_layers=R.fc_layer_list(arch["te"]), motor_decoder_layers=R.fc_layer_list(arch["md"]),
               world_model_layers=R.fc_layer_list(arch["wm"]), task_encoder_output_dim=Z, device="cuda", max_batch=rows)
    m = PhysicsVAE(cmc["observation_space"], cmc["action_space"], 2 * Da, {"custom_model_config": cmc}, "physics_vae")
    m.load_state_dict(R.perturb_biases(R.init_state_dict(arch, seed=1), seed=3))
    return m, Db, Da, Z


def torch_forward(m, obs, eps, Db, Z):
    """The module's forward through its torch sub-modules (rmt:742-771 as upstream runs it)."""
    h = m._task_encoder(obs)
    z = h[:, :Z] + eps * torch.exp(0.5 * h[:, Z:])
    a = m._motor_decoder._model[:-1](torch.cat([obs[:, :Db], z], dim=1))
    logits = m._motor_decoder._model[-1](a)
    s2 = m._world_model(torch.cat([obs[:, :Db], a], dim=1))
    return logits, m._value_branch(obs).squeeze(1), s2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    m, Db, Da, Z = build(a.rows)
    g = torch.Generator(device="cuda").manual_seed(0)
    obs = torch.randn(a.rows, 2 * Db, device="cuda", generator=g)
    eps = torch.randn(a.rows, Z, device="cuda", generator=g)
    act = 0.1 * torch.randn(a.rows, Da, device="cuda", generator=g)
    adv = torch.randn(a.rows, device="cuda", generator=g)
    ret = torch.randn(a.rows, device="cuda", generator=g)
    with torch.no_grad():
        lg, _ = m.forward({"obs_flat": obs}, [], None, eps=eps)
    old_logp = -0.5 * (((act - lg[:, :Da]) / 0.1) ** 2).sum(1)
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-5)

    def loss_of(logits, value):
        mean, log_std = logits[:, :Da], logits[:, Da:]
        logp = -0.5 * (((act - mean) / torch.exp(log_std)) ** 2).sum(1) - log_std.sum(1) - 0.5 * Da * math.log(2 * math.pi)
        ratio = torch.exp(logp - old_logp)
        return -torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv).mean() + 0.5 * ((value - ret) ** 2).mean()

    def update_hip():
        opt.zero_grad(set_to_none=True)
        logits, _ = m.forward({"obs_flat": obs}, [], None, eps=eps)
        loss_of(logits, m.value_function()).backward()
        opt.step()

    def update_torch():
        opt.zero_grad(set_to_none=True)
        logits, value, _ = torch_forward(m, obs, eps, Db, Z)
        loss_of(logits, value).backward()
        opt.step()

    out = {"rows": a.rows, "steps": a.steps, "warmup": a.warmup}
    for name, fn in (("hip", update_hip), ("torch", update_torch)):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        out[name + "_us_per_update"] = round((time.perf_counter() - t0) / a.steps * 1e6, 1)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kern = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        out[name + "_launches_per_update"] = len(kern)
        out[name + "_gemm_ops"] = sum(1 for e in prof.events() if e.name in ("aten::mm", "aten::addmm"))
    out["hip_over_torch"] = round(out["hip_us_per_update"] / out["torch_us_per_update"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
