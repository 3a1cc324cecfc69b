"""One PPO minibatch update of PhysicsVAE timed four ways on the same GPU in one session:
  a  update       forward + the loss in torch + backward() + torch.optim.Adam   (the HIP forward / backward kernels under autograd)
  b  hip_loss     as (a) with ppo.HipPPOLoss (one launch) in place of the torch loss
  c  ppo_step     the fused step, pvae_ppo_step, called per minibatch from Python
  d  ppo_sgd      pvae_ppo_sgd: `--steps` steps enqueued in ONE call, one synchronisation at the end, per step
At the runtime spec's shapes (loco_runtime_physics_vae.yaml): observation 2 x 197, 45 actions, latent 32, encoder 256x2,
decoder 512x3, value branch 256x2, `--rows` rows (500: the spec's sgd_minibatch_size).  The loss of (a) is
ppo.ppo_loss_torch -- the full specification, which is what an RLlib learner evaluates.

The ways alternate block by block within the session (`--rounds` rounds of `--steps` updates each), so clock and thermal
drift hit all of them alike; reported per way: median, min and max of the per-round means, in microseconds, and for (c)
and (d) the acceptance figure: (b.median - x.median) / (b.max - b.min), which must exceed 3.  Prints one JSON line.

    python tools/vae_ppo_bench.py [--rows 500] [--steps 200] [--rounds 7] [--warmup 30] [--one-step] [--diag]
    python tools/vae_ppo_bench.py --order philox torch [none] [--rounds 7] [--learn-rows 6250] [--out FILE]
`--order`: time the minibatch order instead (tools/order_bench.py): `pvae_ppo_order` against the torch.randperm stack it
replaces, and the whole `ppo_learn` call (sgd_minibatch_size `--rows`, 20 passes) with the order made each of the ways named.
`--diag`: ways c and d run with a learner-diagnostics buffer bound (`ppo_diag`; one small launch more per step).
`--grad-clip X`: global-norm gradient clipping at max_norm X -- ways a and b get `clip_grad_norm_` between backward() and
the optimizer step, and a fifth way is timed in the same rounds, alternating with (d): e  ppo_sgd_clip, (d) with the clip
bound (`ppo_grad_clip`: one launch more per step); (c) and (d) stay unbound.  Reported beside it: e.median - d.median.
`--one-step`: run a single fused step and exit (for a kernel trace of one step).
`--prior {zero_mean,state_mean,sphere}`: the model's latent_prior_type (default zero_mean, whose output is the one printed
without the flag); the other two run the fused ways on a module that opted in ("ppo_priors") and ways a and b under that
prior -- the path the fused step replaces for such a model.
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import order_bench                                               # noqa: E402
from physicsvae_amd import ppo as P                              # noqa: E402
from physicsvae_amd.engine import make_ppo_batch                 # noqa: E402
from physicsvae_amd.model import PhysicsVAE, fc_spec             # noqa: E402
from physicsvae_amd.spaces import Box                            # noqa: E402

DB, DA, Z = 197, 45, 32
PRIORS = {"zero_mean": "normal_zero_mean_one_std", "state_mean": "normal_state_mean_one_std", "sphere": "hypersphere_uniform"}


def make_model(max_batch, prior="zero_mean"):
    cmc = dict(observation_space=Box(np.zeros(2 * DB), np.zeros(2 * DB)), observation_space_body=Box(np.zeros(DB), np.zeros(DB)),
               observation_space_task=Box(np.zeros(DB), np.zeros(DB)), action_space=Box(np.zeros(DA), np.zeros(DA)),
               task_encoder_layers=fc_spec(256, 2), motor_decoder_layers=fc_spec(512, 3), value_fn_layers=fc_spec(256, 2),
               task_encoder_output_dim=Z, device="cuda", max_batch=max_batch, sample_std=0.3)
    if prior != "zero_mean":
        cmc.update(latent_prior_type=PRIORS[prior], ppo_priors=True)
    return PhysicsVAE(cmc["observation_space"], cmc["action_space"], 2 * DA, {"custom_model_config": cmc}, "physics_vae")


def make_batch(m, n, g, max_batch):
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)          # noqa: E731
    obs = rn(n, 2 * DB)
    with torch.no_grad():
        logits = torch.cat([m.forward({"obs_flat": obs[lo: lo + max_batch]}, [], None)[0] for lo in range(0, n, max_batch)])
    mean, ls = logits[:, :DA], logits[:, DA:]
    actions = mean + torch.exp(ls) * rn(n, DA)
    logp = -0.5 * (((actions - mean) / torch.exp(ls)) ** 2).sum(1) - ls.sum(1) - 0.5 * DA * math.log(2 * math.pi)
    return {"obs": obs, "actions": actions, "action_dist_inputs": torch.cat([mean + 0.02 * rn(n, DA), ls + 0.05 * rn(n, DA)], 1),
            "action_logp": logp - 0.35 * rn(n), "advantages": rn(n), "value_targets": rn(n), "vf_preds": rn(n)}


def order_mode(a):
    """`--order`: the runtime spec's learner call -- a worker's train batch, sgd_minibatch_size `--rows`, num_sgd_iter 20."""
    cfg = P.PPOConfig(clip_param=0.2, kl_coeff=0.0, vf_clip_param=1000.0, lr=1e-6, sgd_minibatch_size=a.rows, num_sgd_iter=20)
    torch.manual_seed(0)
    mb = max(a.rows, 32)
    m = make_model(mb)
    batch = make_batch(m, a.learn_rows, torch.Generator(device="cuda").manual_seed(0), mb)
    out = dict(order_bench.run(m, batch, cfg, a), model="physics_vae", obs=2 * DB)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--one-step", action="store_true")
    ap.add_argument("--diag", action="store_true",
                    help="ways c and d with a learner-diagnostics buffer bound (ppo.DIAG): one small launch more per step")
    ap.add_argument("--grad-clip", type=float, default=None,
                    help="max_norm: ways a and b with clip_grad_norm_, and way e = way d with the clip bound")
    ap.add_argument("--prior", choices=tuple(PRIORS), default="zero_mean", help="the model's latent_prior_type")
    order_bench.add_arguments(ap)
    a = ap.parse_args()
    if a.order:
        return order_mode(a)
    cfg = P.PPOConfig(clip_param=0.2, kl_coeff=0.0, vf_clip_param=1000.0, lr=1e-6, sgd_minibatch_size=a.rows, num_sgd_iter=1)
    out = {"rows": a.rows, "steps": a.steps, "rounds": a.rounds, "obs": 2 * DB}
    torch.manual_seed(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    mb = max(a.rows, 32)
    if a.prior != "zero_mean":
        out["prior"] = PRIORS[a.prior]
    m = make_model(mb, a.prior)         # ways a, b: torch.optim.Adam
    f = make_model(mb, a.prior)         # ways c, d: the fused step (its own weights and Adam state)
    f.load_state_dict(m.state_dict())
    m._world_model.requires_grad_(False)         # (the learner's loss never reaches the world model)
    mini = make_batch(m, a.rows, g, mb)
    big = make_batch(m, a.rows * a.steps, g, mb)        # (d): `steps` minibatches of one pass
    cols = P.batch_columns(mini)
    obs = mini["obs"]
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=cfg.lr)
    eng = f.engine
    eng.ppo_bind(f._ppo_value_engine(), f._als.on_device(eng.device), False)
    out["diag"] = bool(a.diag)
    out["grad_clip"] = a.grad_clip
    if a.diag:
        eng.ppo_diag(torch.zeros(a.steps, P.PPO_DIAG, dtype=torch.float32, device="cuda"))       # one row per step of way d
    fb, fbig = eng.ppo_batch(cols), eng.ppo_batch(P.batch_columns(big))
    loss_params = cfg.params("constant")
    loss_cols = {k: v for k, v in cols.items() if k != "obs"}
    hip_cols = make_ppo_batch(loss_cols, "cuda", DA)
    t = [0]
    clipped = list([p for p in m.parameters() if p.requires_grad])

    def clip_twin():
        if a.grad_clip is not None:
            torch.nn.utils.clip_grad_norm_(clipped, a.grad_clip)

    def update_torch_loss():
        opt.zero_grad(set_to_none=True)
        logits, _ = m.forward({"obs_flat": obs}, [], None)
        total, _ = P.ppo_loss_torch(logits[:, :DA], logits[:, DA:], m.value_function(), cfg=cfg, **loss_cols)
        total.backward()
        clip_twin()
        opt.step()

    def update_hip_loss():
        opt.zero_grad(set_to_none=True)
        logits, _ = m.forward({"obs_flat": obs}, [], None)
        total, _ = P.HipPPOLoss.apply(logits[:, :DA], logits[:, DA:], m.value_function(), hip_cols, loss_params, None)
        total.backward()
        clip_twin()
        opt.step()

    stats = torch.empty(5, device="cuda")

    def step_once():
        t[0] += 1
        eng.ppo_step(fb, cfg.params("constant", adam_t=t[0]), 0, a.rows, None, offset=t[0], stats_out=stats)

    if a.one_step:
        step_once()
        torch.cuda.synchronize()
        out["launches_per_step"] = eng.ppo_launches()
        print(json.dumps(out))
        return

    def sgd_block():
        eng.ppo_sgd(fbig, cfg.params("constant", adam_t=t[0] + 1), a.rows, 1, offset=t[0] + 1)
        t[0] += a.steps

    def sgd_clip_block():
        eng.ppo_grad_clip(a.grad_clip)
        try:
            sgd_block()
            return eng.ppo_launches()
        finally:
            eng.ppo_grad_clip(None)

    per_call = (("a_update", update_torch_loss), ("b_hip_loss", update_hip_loss), ("c_ppo_step", step_once))
    for _, fn in per_call:
        for _ in range(a.warmup):
            fn()
    sgd_block()
    means = {name: [] for name, _ in per_call}
    means["d_ppo_sgd"] = []
    if a.grad_clip is not None:
        clip_launches = sgd_clip_block()
        means["e_ppo_sgd_clip"] = []
    for _ in range(a.rounds):                    # the ways alternate within the session
        for name, fn in per_call:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            means[name].append((time.perf_counter() - t0) / a.steps * 1e6)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sgd_block()
        torch.cuda.synchronize()
        means["d_ppo_sgd"].append((time.perf_counter() - t0) / a.steps * 1e6)
        if a.grad_clip is not None:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sgd_clip_block()
            torch.cuda.synchronize()
            means["e_ppo_sgd_clip"].append((time.perf_counter() - t0) / a.steps * 1e6)
    res = {name: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
           for name, v in means.items()}
    spread = res["b_hip_loss"]["max"] - res["b_hip_loss"]["min"]
    for name in ("c_ppo_step", "d_ppo_sgd"):
        res[name]["gain_over_b_in_spreads_of_b"] = round((res["b_hip_loss"]["median"] - res[name]["median"]) / max(spread, 1e-9), 1)
    if a.grad_clip is not None:
        res["e_ppo_sgd_clip"]["over_d_us"] = round(res["e_ppo_sgd_clip"]["median"] - res["d_ppo_sgd"]["median"], 1)
        res["e_ppo_sgd_clip"]["launches_per_step"] = clip_launches
        sgd_block()                              # (the counter below is the unbound step's)
    res["launches_per_step"] = eng.ppo_launches()
    out["constant"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
