"""Gradient clipping under the workers' gradient exchange (include/pvae.h "Gradient clipping inside the PPO learners": every
worker clips its own gradient first, then the clipped gradients are averaged), two or three processes that share cuda:0
(tests/ppo_clip_dp_worker.py; fresh children, each under its own time limit).  Every worker has rows of its own and hence a
coefficient of its own; the threshold lies between the workers' raw norms of the first step, so one of them clips there and
another does not.  The replicas must be bit-identical across ranks, across the two transports (two workers: a two-term sum is
commutative) and to the one-process emulation -- `*_ppo_grad` unclipped per rank, times the coefficient the device itself
reported in entry 6, the rank-ordered float32 mean, `*_ppo_apply`; no wait may give up."""
import math
import os
import subprocess
import sys

import pytest
import torch

import ppo_clip_cases as CC
import ppo_clip_dp_worker as CW
import ppo_diag_cases as D
import ppo_dp_worker as W
from physicsvae_amd import ppo as P
from physicsvae_amd.parallel import PPODataParallel
from ppo_clip_cases import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = D.GNORM_RTOL


def run_workers(tmp_path, name, tag, port, max_norm, **extra_env):
    world = len(CW.CASES[name]["n_rows"])
    out = str(tmp_path / tag)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world),
               HSA_ENABLE_IPC_MODE_LEGACY="0", **extra_env)
    procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "ppo_clip_dp_worker.py"),
                               ROOT, out, name, repr(float(max_norm))], env=dict(env, RANK=str(r), LOCAL_RANK="0"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = [p.communicate()[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [torch.load(out + ".%d" % r) for r in range(world)]


@pytest.mark.parametrize("model", ["fcnn", "vae"])
def test_world_one_exchange_gives_the_plain_clipped_step(model):
    case = dict(model=model, kind="state_independent", n_rows=(41,), minibatch=16, passes=1)
    max_norm = 0.5 * CW.raw_norms(case)[0]
    cfg = CW.config(case, max_norm)
    a, b, c = W.make_model(case), W.make_model(case), W.make_model(case)
    (batch,), (eps,) = CW.make_batches(case, a)
    dbatch = W.on_dev(batch)
    kw = {"eps": eps[0]} if eps is not None else {}
    da, db, dc = (P.diag_buffer(41, cfg, DEV) for _ in range(3))
    want = a.ppo_learn(dbatch, cfg, diag_out=da, **kw)
    dp = PPODataParallel(0, 1, transport="p2p")
    dp.attach(b)
    got = b.ppo_learn(dbatch, cfg, dp=dp, diag_out=db, **kw)
    assert same_bits(got, want) and same_bits(da, db) and W.same_state(W.state(a), W.state(b))
    assert dp.timeouts(b) == 0 and float(da[0, 6]) < 1.0 and a.engine.ppo_launches() == b.engine.ppo_launches()
    dp.detach(b)
    got = c.ppo_learn(dbatch, cfg, dp=PPODataParallel(0, 1, transport="torch"), diag_out=dc, **kw)
    assert same_bits(got, want) and same_bits(dc, da) and W.same_state(W.state(a), W.state(c))
    for i in range(3):
        CC.check_row(da[i].cpu(), max_norm, RTOL, (model, i))
    # and the clip did something: the unclipped learner ends elsewhere
    d = W.make_model(case)
    d.ppo_learn(dbatch, W.config(case), **kw)
    assert not W.same_state(W.state(a), W.state(d))


@pytest.mark.parametrize("name,port,transports", [("fc2", 29641, ("p2p", "torch")), ("vae2", 29644, ("p2p", "torch")),
                                                  ("fc3", 29647, ("p2p",))])
def test_workers_clip_their_own_gradient_then_average(tmp_path, name, port, transports):
    case = CW.CASES[name]
    world, steps = len(case["n_rows"]), W.steps_of(case)
    first = CW.raw_norms(case)
    assert max(first) > 1.02 * min(first), first                                     # different rows, different norms
    max_norm = math.sqrt(min(first) * max(first))                                    # between them: one clips, one does not
    runs = {t: run_workers(tmp_path, name, "%s_%s" % (name, t), port + i, max_norm, PPO_DP_TRANSPORT=t) for i, t in enumerate(transports)}
    p2p = runs["p2p"]
    coefs = [p2p[r]["diag"][:, 6] for r in range(world)]
    want_state, raws = CW.emulate(case, coefs)
    for t, res in runs.items():
        for r in range(world):
            got = res[r]
            assert got["timeouts"] == 0 and got["bound"] is None and tuple(got["diag"].shape) == (steps, P.PPO_DIAG)
            assert W.same_state(got["state"], res[0]["state"]), (t, "replica %d differs from replica 0" % r)
            assert W.same_state(got["state"], want_state), (t, "replica %d differs from the one-process emulation" % r)
            assert same_bits(got["diag"][:, 4], res[0]["diag"][:, 4])                # what Adam consumed: the same on every rank
            assert same_bits(got["diag"], p2p[r]["diag"]) and same_bits(got["stats"], p2p[r]["stats"]), (t, r)
            assert bool(torch.isfinite(got["diag"]).all()) and bool(torch.isfinite(got["stats"]).all())
    for r in range(world):
        for i in range(steps):
            raw, coef = float(p2p[r]["diag"][i, 5]), float(p2p[r]["diag"][i, 6])
            want = float(P.clip_coef_torch([torch.tensor([raws[r][i]], dtype=torch.float64)], max_norm)[1])
            print(name, "rank", r, "step", i, "raw", raw, "float64", raws[r][i], "coef", coef, "want", want, "grad_gnorm", float(p2p[r]["diag"][i, 4]))
            assert abs(raw - raws[r][i]) <= RTOL * raws[r][i] and abs(coef - want) <= RTOL * want
    step0 = [float(c[0]) for c in coefs]
    assert min(step0) < 1.0 and max(step0) == 1.0, step0                             # one worker clips, one does not
    assert not same_bits(p2p[0]["diag"][:, 5], p2p[1]["diag"][:, 5])
    assert not same_bits(p2p[0]["stats"], p2p[1]["stats"])
    # the averaged gradient's norm is at most the mean of the clipped norms
    for i in range(steps):
        bound = sum(float(coefs[r][i]) * raws[r][i] for r in range(world)) / world
        assert float(p2p[0]["diag"][i, 4]) <= bound * (1 + 1e-5)
