"""Imagined rollouts timed on one GPU at the runtime spec's shapes (observation 722 = 2 x 361, 54 actions, the DEFAULT
architecture: latent 32, encoder 256x2, decoder 512x3, world model 1024x2), 512 rows, H = 30 steps, the three modes:
  loop      what a caller writes without `imagine`: the module's stage-by-stage calls under no_grad, per step
            forward_encoder + forward_decoder + forward_world ("track"), torch.randn + forward_decoder + forward_world
            ("prior"), forward_world ("replay"), the prediction fed back with torch.cat -- code this library version did not
            touch, so it stands for the parent commit's path
  imagine   `PhysicsVAE.imagine(...)`: one library call (pvae_imagine)
Both paths run in the same process and session, alternating, each sample one whole unroll ending in a device synchronise;
reported: median, min and max of `--rounds` (7) rounds in microseconds per unroll, and the launches one `imagine` call
enqueued (the count `pvae_imagine` returns) with pvae_imagine_launches' per-step figure, next to the library calls of the
loop.  Prints one JSON line and, with --out, writes it to a file.

    python tools/imagine_bench.py [--rounds 7] [--out profiles/imagine_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OBS, K, Z, ROWS, H = 722, 54, 32, 512, 30
MODES = ("replay", "track", "prior")
LOOP_CALLS = {"replay": 1, "track": 4, "prior": 2}          # library calls per step of the loop (net_forward x3 + reparam)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from physicsvae_amd.model import PhysicsVAE
    from physicsvae_amd.spaces import Box
    assert torch.cuda.is_available(), "this benchmark measures the GPU: there is nothing to report without one"
    assert a.rounds >= 7, "report the median of at least 7 rounds"
    box = lambda n: Box(np.zeros(n), np.zeros(n))                # noqa: E731
    torch.manual_seed(0)
    Db = OBS // 2
    cmc = dict(observation_space=box(OBS), observation_space_body=box(Db), observation_space_task=box(Db), action_space=box(K),
               device="cuda", max_batch=ROWS, sample_std=0.3)
    m = PhysicsVAE(cmc["observation_space"], cmc["action_space"], 2 * K, {"custom_model_config": cmc}, "physics_vae")
    assert m._task_encoder_output_dim == Z
    dev = "cuda"
    s0 = torch.randn(ROWS, Db, device=dev)
    goals, actions = torch.randn(H, ROWS, Db, device=dev), torch.randn(H, ROWS, K, device=dev)

    def loop(mode):
        with torch.no_grad():
            s, out = s0, []
            for t in range(H):
                if mode == "replay":
                    logits = actions[t]
                else:
                    if mode == "track":
                        _, z, _ = m.forward_encoder(torch.cat([s, goals[t]], 1))
                    else:
                        z = torch.randn(ROWS, Z, device=dev)
                    logits, _ = m.forward_decoder(s, z)
                s = m.forward_world(s, logits)
                out.append(s)
            return out

    def fused(mode):
        return m.imagine(mode, s0, H, goals=goals if mode == "track" else None, actions=actions if mode == "replay" else None,
                         want=("states",))

    def timed(fn, mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(mode)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    ways = (("loop", loop), ("imagine", fused))
    for mode in MODES:
        for _, fn in ways:
            for _ in range(a.warmup):
                fn(mode)
    samples = {}
    for _ in range(a.rounds):                                    # the two paths alternate within the session
        for mode in MODES:
            for way, fn in ways:
                samples.setdefault("%s/%s" % (mode, way), []).append(timed(fn, mode))
    out = {"obs": OBS, "k": K, "latent": Z, "rows": ROWS, "horizon": H, "rounds": a.rounds, "unit": "us per unroll of H steps",
           "device": torch.cuda.get_device_name(0), "launches": {}, "times": {}}
    for mode in MODES:
        per_step, per_call = m.engine.imagine_launches(mode)
        fused(mode)
        out["launches"][mode] = {"imagine_per_step": per_step, "imagine_per_call_at_most": per_call,
                                 "imagine_this_call": int(m.engine.imagine_launched),         # what pvae_imagine returned
                                 "loop_library_calls_per_step": LOOP_CALLS[mode]}
    for key, us in sorted(samples.items()):
        out["times"][key] = {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1)}
    for mode in MODES:
        t = out["times"]
        out["times"]["%s/imagine_over_loop" % mode] = round(t["%s/imagine" % mode]["median"] / t["%s/loop" % mode]["median"], 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
