"""Time optimizer steps of the multi-step unroll (lookahead L, tpv:367-428) at the benchmark
sizes (B=256, TE/MD/WM 4x1024, Db=197, Da=45) and compare with L independent lookahead-1 steps.
`--s-rec C` runs the joint phase with world_model_s_rec_coeff = C (the demonstrated-action pass of the frozen world model,
tpv:411-414); the line then also carries the number of stages of each joint backward plan.
Usage (GPU box): python tools/lookahead_bench.py [--lookahead 2] [--steps 200] [--s-rec 0.5]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lookahead", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--s-rec", type=float, default=None, help="world_model_s_rec_coeff of the joint phase (default: the trainer's, 0)")
    a = ap.parse_args()
    from synth_demo import make_trainer, synth_demo
    data = synth_demo(0, 10, 1000, 197, 45)
    out = {}
    for L in (1, a.lookahead):
        with contextlib.redirect_stdout(io.StringIO()):
            tr = make_trainer(data, a.batch, "cuda", extra={"lookahead": L})
        eng = tr.engine
        ds = tr.train_loader.dataset
        eng.bind_dataset(*ds.device_arrays(eng.device))
        full = len(ds) // a.batch
        loss = torch.zeros(5, device="cuda")
        for name in ("world", "joint"):
            w = name == "world"
            tr.model.set_learnable_task_encoder(not w)
            tr.model.set_learnable_motor_decoder(not w)
            tr.model.set_learnable_world_model(w)
            tr.read_loss_fn_coeff(world=w)
            if not w and a.s_rec is not None:
                tr.s_rec_coeff = a.s_rec
                eng.set_joint_s_rec(a.s_rec != 0)
            phase, nets = tr.phase()
            if not w:
                out["L%d_joint_s_rec_coeff" % L] = tr.s_rec_coeff
                out["L%d_joint_backward_stages" % L] = len(eng.backward_plan(phase, tr.step_params(nets, a.batch, False)))

            def run(n, start):
                for i in range(n):
                    g = (start + i) % full
                    sp = tr.step_params(nets, a.batch, True)
                    sp.rng_seed, sp.rng_offset = 7, (start + i) * 65536
                    eng.train_step(phase, g * a.batch, a.batch, sp, loss_out=loss)
            run(20, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(a.steps, 20)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.steps
            out["L%d_%s_us_per_step" % (L, name)] = dt * 1e6
            out["L%d_%s_loss" % (L, name)] = float(loss[0])
            if not w:
                out["L%d_joint_loss_s" % L] = float(loss[3])
        if a.s_rec is not None and L == 1:
            # what the term is priced against: the world model's forward alone, and forward + input-gradient chain
            # (pvae_net_backward without a gradient buffer recomputes the forward, then runs the dgrad launches only)
            from physicsvae_amd import _lib
            x = torch.randn(a.batch, eng.net_in_width(_lib.NET_WM), device="cuda")
            dy = torch.randn(a.batch, 197, device="cuda")
            for key, fn in (("wm_forward_us", lambda: eng.net_forward(_lib.NET_WM, x)),
                            ("wm_forward_dgrad_us", lambda: eng.net_backward(_lib.NET_WM, x, dy, True))):
                for _ in range(20):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                out[key] = (time.perf_counter() - t0) / a.steps * 1e6
    print(json.dumps(out))


if __name__ == "__main__":
    main()
