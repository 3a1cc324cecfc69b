"""Imagined rollouts on the device (include/pvae.h pvae_imagine; HipEngine.imagine, PhysicsVAE.imagine,
TrainModel.evaluate_rollout) on the eight models of tests/imagine_cases.py at 1, 5 and 33 rows (max_batch 64), H = 1 and 3.

  1 same bits     every step's a_t, z_t, s_{t+1} equal, bit for bit, what the existing entry points compute from the call's
                  own s_t: `infer` (with s2_hat) wherever it takes the staged path (more than 4 rows, or a helper model), the
                  net_forward / reparam chain otherwise; supplied draws and Philox
  2 float64       each step of `imagine_torch` in float64 from the device's s_t: outputs within ROLLOUT_BOUND (2e-5 scaled),
                  err within FORWARD_BOUND (1e-5 relative) of the float64 mean over the device's own states
  3 in place      (dataset tensor, row_index) sources give the bits of the same values passed dense
  4 guards        outputs and scratch inside guard bands; outputs not asked for are not written
  5 determinism   two calls agree in every byte
  6 training      K training steps with an imagine call between two of them give the parameters of K steps without it
  7 launches      the kernels a profiler lists for a call equal pvae_imagine_launches' per_step * H + per_call.  Counted
                  in a child process (tests/imagine_launch_child.py), so that the tracer stays out of the suite's process,
                  from the profiler's device records; records whose name holds "memcpy" or "memset" are filtered out by
                  name (they are no kernels).  Test 8 holds the call's own return value to the same figure
  8 refusals      every refusal answers -1 and leaves the outputs alone
  9 trainer       evaluate_rollout equals imagine_torch over the same windows"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import guards as G
import imagine_cases as IC
import infer_cases as I
from oracle import refpath as R
from physicsvae_amd import _lib
from physicsvae_amd.engine import Arch, HipEngine, make_step_params
from physicsvae_amd.imagine import imagine_torch
from util import make_trainer, max_err_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = IC.H
SEED, OFFSET = 11, 5
_MODELS = {}


def model(name):
    if name not in _MODELS:
        _MODELS[name] = I.module_for(IC.case(name), DEV)
    return _MODELS[name]


def dev(x):
    return None if x is None else x.to(DEV)


def call(name, mode, rows, horizon=H, philox=False, supplied_z=True, **kw):
    """eng.imagine on the first `rows` rows of the case's pool; track mode under the pool's draws unless `philox`."""
    c, eng = IC.case(name), model(name).engine
    d = IC.drives(c, mode, rows, horizon, supplied_z=supplied_z)
    d.pop("n", None)
    if philox:
        d.pop("eps", None)
    return eng.imagine(mode, dev(c.s0[:rows]), horizon, seed=SEED, offset=OFFSET, **{k: dev(v) for k, v in d.items()}, **kw)


def drawn(eng, rows, t):
    """n_t of the rule: what pvae_reparam forms from a zero [mu | logvar] at (seed, offset + t)."""
    return eng.reparam(torch.zeros(rows, 2 * eng.arch.Z, device=DEV), seed=SEED, offset=OFFSET + t)


# ---- 1. the same bits as the staged path, step by step -------------------------------------------------------------
@pytest.mark.parametrize("rows", IC.ROWS)
@pytest.mark.parametrize("name", IC.CASE_IDS)
def test_track_steps_are_the_staged_path_bit_for_bit(name, rows):
    c, eng = IC.case(name), model(name).engine
    for philox, horizon in ((False, H), (True, H), (False, 1), (True, 1)):     # (H = 1: the hand-over with no next step is its only one)
        out = call(name, "track", rows, horizon, philox=philox)
        assert tuple(out["states"].shape) == (horizon, rows, c.Db)
        for t in range(horizon):
            s = dev(c.s0[:rows]) if t == 0 else out["states"][t - 1]
            obs = torch.cat([s, dev(c.goals[t, :rows])], 1).contiguous()
            eps = None if philox else dev(c.eps[t, :rows])
            if rows > 4 or c.mh is not None:
                a, s2, z = eng.infer(obs, eps=eps, noise=True, seed=SEED, offset=OFFSET + t, want_s2=True)
            else:
                z = eng.reparam(eng.net_forward(_lib.NET_TE, obs), eps=eps, noise=True, seed=SEED, offset=OFFSET + t)
                a = eng.net_forward(_lib.NET_MD, torch.cat([s, z], 1).contiguous())
                s2 = eng.net_forward(_lib.NET_WM, torch.cat([s, a], 1).contiguous())
            assert torch.equal(out["z"][t], z), (philox, t, "z")
            assert torch.equal(out["actions"][t], a), (philox, t, "a")
            assert torch.equal(out["states"][t], s2), (philox, t, "s")


@pytest.mark.parametrize("rows", IC.ROWS)
@pytest.mark.parametrize("name", IC.CASE_IDS)
def test_replay_and_prior_steps_are_the_stage_calls_bit_for_bit(name, rows):
    c, eng = IC.case(name), model(name).engine
    for horizon in IC.HORIZONS:
        _replay_and_prior_steps(c, eng, name, rows, horizon)


def _replay_and_prior_steps(c, eng, name, rows, H):
    out = call(name, "replay", rows, H)
    assert "z" not in out and tuple(out["states"].shape) == (H, rows, c.Db)
    for t in range(H):
        s = dev(c.s0[:rows]) if t == 0 else out["states"][t - 1]
        assert torch.equal(out["actions"][t], dev(c.actions[t, :rows]))
        assert torch.equal(out["states"][t], eng.net_forward(_lib.NET_WM, torch.cat([s, dev(c.actions[t, :rows])], 1).contiguous()))
    for supplied in ((True, False) if IC.draws_prior(c) else (True,)):
        out = call(name, "prior", rows, H, supplied_z=supplied)
        for t in range(H):
            s = dev(c.s0[:rows]) if t == 0 else out["states"][t - 1]
            if supplied:
                z = dev(c.z[t, :rows])
            else:
                z = drawn(eng, rows, t)
                if c.prior == I.STATE_MEAN:
                    z = eng.net_forward(_lib.NET_PR, s.contiguous()) + z
            assert torch.equal(out["z"][t], z), (supplied, t, "z")
            if c.mh is None:                   # (with the helper the action is decoder + range * helper in one fma: test 2 holds it)
                assert torch.equal(out["actions"][t], eng.net_forward(_lib.NET_MD, torch.cat([s, z], 1).contiguous())), (supplied, t)
            assert torch.equal(out["states"][t], eng.net_forward(_lib.NET_WM, torch.cat([s, out["actions"][t]], 1).contiguous()))


# ---- 2. against float64, teacher-forced -----------------------------------------------------------------------------
@pytest.mark.parametrize("rows", IC.ROWS)
@pytest.mark.parametrize("name", IC.CASE_IDS)
def test_steps_against_float64_from_the_devices_states(name, rows):
    c, eng = IC.case(name), model(name).engine
    for mode in IC.MODES:
        for supplied in ((True, False) if mode == "prior" and IC.draws_prior(c) else (True,)):
            for horizon in IC.HORIZONS:
                out = call(name, mode, rows, horizon, supplied_z=supplied)
                got = {k: v.cpu() for k, v in out.items()}
                d = IC.drives(c, mode, rows, horizon, torch.float64, supplied)
                if "n" in d:
                    d["n"] = torch.stack([drawn(eng, rows, t) for t in range(horizon)]).cpu().double()
                want = imagine_torch(c.A, c.sd, mode, c.s0[:rows].double(), horizon, teacher=got["states"].double(), **d)
                for q in ("states", "actions", "z"):
                    if want[q] is not None:
                        e = max_err_scaled(got[q], want[q])
                        print(name, mode, supplied, rows, horizon, q, e)
                        assert e <= IC.ROLLOUT_BOUND, (mode, supplied, horizon, q, e)
                diff = got["states"].double() - c.targets[:horizon, :rows].double()
                ref = (diff * diff).mean(dim=(1, 2))
                e = float(((got["err"].double() - ref).abs() / ref).max())
                print(name, mode, supplied, rows, horizon, "err", e)
                assert e <= IC.FORWARD_BOUND, (mode, supplied, horizon, e)


# ---- 3. in-place sources ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("zero_mean", "db1", "helper"))
def test_in_place_sources_give_the_dense_bits(name):
    c, eng = IC.case(name), model(name).engine
    g = torch.Generator().manual_seed(3)
    N, rows = 200, 33
    states, actions = torch.randn(N, c.Db, generator=g).to(DEV), torch.randn(N, c.Da, generator=g).to(DEV)
    idx = torch.randint(0, N - H - 1, (rows,), generator=g).to(torch.int32).to(DEV)
    li = idx.long()
    run = lambda off: torch.stack([states[li + off + t] for t in range(H)])          # noqa: E731
    dense = eng.imagine("track", states[li], H, goals=run(1), targets=run(1), eps=dev(c.eps[:, :rows]))
    there = eng.imagine("track", (states, idx), H, goals=(states, idx, 1), targets=(states, idx, 1), eps=dev(c.eps[:, :rows]))
    for k in ("states", "actions", "z", "err"):
        assert torch.equal(dense[k], there[k]), k
    dense = eng.imagine("replay", states[li], H, actions=torch.stack([actions[li + t] for t in range(H)]), targets=run(1))
    there = eng.imagine("replay", (states, idx), H, actions=(actions, idx), targets=(states, idx, 1))
    for k in ("states", "actions", "err"):
        assert torch.equal(dense[k], there[k]), k
    codes = torch.randn(N, c.Z, generator=g).to(DEV)
    dense = eng.imagine("prior", states[li], H, z=torch.stack([codes[li + t] for t in range(H)]), targets=run(1))
    there = eng.imagine("prior", (states, idx), H, z=(codes, idx), targets=(states, idx, 1))
    for k in ("states", "actions", "z", "err"):
        assert torch.equal(dense[k], there[k]), k


# ---- 4. guard bands, 5. determinism ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("state_mean", "task_body", "db1"))
def test_outputs_and_scratch_stay_inside_their_guards(name):
    c, eng = IC.case(name), model(name).engine
    rows = 33
    bufs = {k: G.guarded((H, rows, w), fill=None, device=DEV) for k, w in (("states", c.Db), ("actions", c.Da), ("z", c.Z))}
    bufs["err"] = G.guarded((H,), fill=None, device=DEV)
    need = int(eng.lib.pvae_imagine_scratch_bytes(eng.ctx, H))
    assert need > 0 and need % 16 == 0
    sbuf, sview = G.guarded(need // 4, fill=None, device=DEV)
    keep = getattr(eng, "_imagine_scratch", None)
    eng._imagine_scratch = sview.view(torch.float64)
    try:
        for mode in IC.MODES:
            for b, v in bufs.values():
                v.copy_(G.poison(v.numel(), DEV).view(v.shape))
            out = call(name, mode, rows, out={k: v for k, (b, v) in bufs.items()})
            torch.cuda.synchronize()
            for k, (b, v) in bufs.items():
                assert G.guards_intact(b, v), (mode, k)
                written = (v.view(torch.int32) != G.POISON_BITS)
                if k == "z" and mode == "replay":
                    assert not bool(written.any())
                else:
                    assert out[k].data_ptr() == v.data_ptr() and bool(written.all()), (mode, k)
            assert G.guards_intact(sbuf, sview), mode
        # outputs not asked for are not written
        for b, v in bufs.values():
            v.copy_(G.poison(v.numel(), DEV).view(v.shape))
        out = call(name, "track", rows, want=("states",), out={k: v for k, (b, v) in bufs.items()})
        torch.cuda.synchronize()
        assert set(out) == {"states", "err"}
        for k in ("actions", "z"):
            assert not bool((bufs[k][1].view(torch.int32) != G.POISON_BITS).any()), k
    finally:
        eng._imagine_scratch = keep


@pytest.mark.parametrize("name", ("zero_mean", "state_mean", "helper"))
def test_two_calls_agree_in_every_byte(name):
    c = IC.case(name)
    for mode in IC.MODES:
        kw = dict(philox=True) if mode == "track" else dict(supplied_z=not IC.draws_prior(c))
        a = {k: v.clone() for k, v in call(name, mode, 33, **kw).items()}
        model(name).engine.infer(torch.randn(7, 2 * c.Db, device=DEV))        # (another call in between)
        b = call(name, mode, 33, **kw)
        for k in a:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (mode, k)


def test_chunked_call_through_the_module():
    name = "zero_mean"
    c, m = IC.case(name), model(name)
    eng, rows = m.engine, IC.POOL
    assert rows > eng.max_batch
    m.seed(SEED)
    m._rng_calls = OFFSET - 1
    out = m.imagine("track", dev(c.s0), H, goals=dev(c.goals), targets=dev(c.targets))
    assert m._rng_calls == OFFSET - 1 + 2 * H
    spans = [(0, 64), (64, 70)]
    parts = [eng.imagine("track", dev(c.s0[lo:hi]), H, goals=dev(c.goals[:, lo:hi]), targets=dev(c.targets[:, lo:hi]), seed=SEED,
                         offset=OFFSET + i * H) for i, (lo, hi) in enumerate(spans)]
    for k in ("states", "actions", "z"):
        assert tuple(out[k].shape)[:2] == (H, rows) and torch.equal(out[k], torch.cat([p[k] for p in parts], 1)), k
    d = out["states"].double().cpu() - c.targets.double()
    ref = (d * d).mean(dim=(1, 2))
    assert float(((out["err"].double().cpu() - ref).abs() / ref).max()) <= IC.FORWARD_BOUND
    m._rng_calls = OFFSET - 1
    m.imagine("replay", dev(c.s0), H, actions=dev(c.actions))
    assert m._rng_calls == OFFSET - 1 + 2 * H            # (advances in every mode, drawn or not)


# ---- 6. training is not disturbed -------------------------------------------------------------------------------------
# "staged": pvae_train_step, which gathers every minibatch; "prefetch": the gather of minibatch k + 1 rides in step k's last
# launch; "direct": pvae_set_direct, the first layers read the set where it lies (shapes that path admits: dim_body >= 64,
# first layers wide enough for the 32x32 tiles at 256 rows, Z % 4 == 0) -- the state pvae_imagine edits (dx.on, staged_rows)
TRAIN = {"staged": dict(Db=23, Da=7, Z=5, nets=dict(te=(40, 2), md=(31, 2), wm=(50, 2)), B=32, direct=False, prefetch=False),
         "prefetch": dict(Db=23, Da=7, Z=5, nets=dict(te=(40, 2), md=(31, 2), wm=(50, 2)), B=32, direct=False, prefetch=True),
         "direct": dict(Db=68, Da=7, Z=4, nets=dict(te=(512, 2), md=(512, 2), wm=(512, 2)), B=256, direct=True, prefetch=True)}
TRAIN_STEPS = 4


@functools.lru_cache(maxsize=None)
def _train_inputs(kind):
    """Weights and a packed set of two episodes, long enough for TRAIN_STEPS + 1 minibatches."""
    t = TRAIN[kind]
    arch = R.make_arch(t["Db"], t["Da"], latent=t["Z"], **t["nets"])
    g = torch.Generator().manual_seed(21)
    T = (TRAIN_STEPS + 1) * t["B"] // 2 + 8
    states, actions = torch.randn(2 * T, t["Db"], generator=g), torch.randn(2 * T, t["Da"], generator=g).clamp_(-3, 3)
    window_row = torch.cat([torch.arange(T - 1), T + torch.arange(T - 1)]).to(torch.int32)
    return arch, R.perturb_biases(R.init_state_dict(arch, seed=8), seed=9), states, actions, window_row


def _train_engine(kind):
    t = TRAIN[kind]
    arch, sd, states, actions, window_row = _train_inputs(kind)
    eng = HipEngine(Arch(t["Db"], t["Da"], t["Z"], t["nets"]["te"], t["nets"]["md"], t["nets"]["wm"]), t["B"], DEV)
    for k, v in eng.named_views().items():
        v.copy_(sd[k])
    return eng


def _train(kind, world, imagine_after):
    t = TRAIN[kind]
    arch, sd, states, actions, window_row = _train_inputs(kind)
    eng = _train_engine(kind)
    pad = lambda a: torch.cat([a, torch.zeros(16, a.shape[1])]).to(DEV)[: a.shape[0]]   # noqa: E731  (slack behind the last row: direct steps)
    st, ac = pad(states), pad(actions)
    if t["direct"]:
        eng.set_direct(True)
    eng.bind_dataset(st, ac, window_row.to(DEV))
    co = R.phase_coeffs(world)
    phase = _lib.PHASE_WORLD if world else _lib.PHASE_JOINT
    B, active = t["B"], []
    for k in range(TRAIN_STEPS):
        sp = make_step_params(lr=5e-4, adam_t=(k + 1,) * 3, a_rec=co["a_rec_coeff"], kl=co["vae_kl_coeff"], s_rec=co["s_rec_coeff"],
                              cyc=co["vae_cycle_coeff"], global_rows=B)
        sp.rng_seed, sp.rng_offset = 3, 100 * k
        active.append(eng.direct_active(phase, B, sp))
        eng.train_step(phase, k * B, B, sp, next_span=((k + 1) * B, B) if t["prefetch"] else None)
        if k == imagine_after:
            idx = window_row[:20].to(DEV)
            eng.imagine("track", (st, idx), 2, goals=(st, idx, 1), targets=(st, idx, 1), seed=1, offset=2)
            eng.imagine("replay", (st, idx), 2, actions=(ac, idx))
            active.append(eng.direct_active(phase, B, sp))
    torch.cuda.synchronize()
    assert all(a == t["direct"] for a in active), (kind, active)       # (the steps around the call took the path the case names)
    return eng.params.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone()


@pytest.mark.parametrize("world", (True, False))
@pytest.mark.parametrize("kind", tuple(TRAIN))
def test_training_steps_are_not_disturbed(kind, world):
    without, with_call = _train(kind, world, None), _train(kind, world, 1)
    for a, b in zip(without, with_call):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(without[0], _train_engine(kind).params)     # (the steps did train)


# ---- 7. launch count --------------------------------------------------------------------------------------------------
def _layers(eng, net):
    return sum(1 for l in eng.layers if l["net"] == net)


def _raw(eng, args):
    return eng.lib.pvae_imagine(eng.ctx, C.byref(args), None)


@functools.lru_cache(maxsize=None)
def _counted():
    """{case/mode/horizon/rows: device kernels of one call}, counted in a child process (tests/imagine_launch_child.py): the
    tracer that lists a process's kernels stays out of the process that runs the suite."""
    import json
    import os
    import subprocess
    import sys
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "imagine_launch_child.py")
    res = subprocess.run([sys.executable, child, *LAUNCH_CASES], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    line = next(l for l in res.stdout.splitlines() if l.startswith("IMAGINE_LAUNCHES "))
    return json.loads(line[len("IMAGINE_LAUNCHES "):])


LAUNCH_CASES = ("zero_mean", "state_mean", "helper")


@pytest.mark.parametrize("name", LAUNCH_CASES)
def test_launch_count_is_what_the_library_states(name):
    c, eng = IC.case(name), model(name).engine
    for mode in IC.MODES:
        per_step, per_call = eng.imagine_launches(mode)
        n = {k: _layers(eng, v) for k, v in (("te", _lib.NET_TE), ("md", _lib.NET_MD), ("wm", _lib.NET_WM), ("pr", _lib.NET_PR),
                                             ("mh", _lib.NET_MH))}
        layers = n["wm"] + (0 if mode == "replay" else n["md"] + n["mh"]) + (n["te"] if mode == "track" else 0) + \
            (n["pr"] if mode == "prior" else 0)
        extra = (1 if mode == "track" or (mode == "prior" and n["pr"]) else 0) + (1 if n["mh"] and mode != "replay" else 0)
        assert per_step == layers + extra + 1 and per_call == 2      # one launch per step beyond layers, sampler, helper's add
        for horizon, rows in ((1, 5), (3, 33)):
            counted = _counted()["%s/%s/%d/%d" % (name, mode, horizon, rows)]
            print(name, mode, horizon, rows, "launches", counted, per_step * horizon + per_call)
            assert counted == per_step * horizon + per_call, (mode, horizon, rows, counted)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------
def _args(eng, c, mode, rows, horizon, outs, scratch):
    a = _lib.ImagineArgs()
    a.mode, a.rows, a.horizon, a.noise = _lib.IMAGINE_MODES[mode], rows, horizon, 1
    keep = []
    a.s0 = eng._imagine_src(dev(c.s0[:rows]), c.Db, None, rows, "s0", keep)
    hs = max(horizon, 1)
    a.goals = eng._imagine_src(dev(c.goals[:hs, :rows]), c.Db, hs, rows, "goals", keep)
    a.actions = eng._imagine_src(dev(c.actions[:hs, :rows]), c.Da, hs, rows, "actions", keep)
    a.z = eng._imagine_src(dev(c.z[:hs, :rows]), c.Z, hs, rows, "z", keep)
    a.targets = eng._imagine_src(dev(c.targets[:hs, :rows]), c.Db, hs, rows, "targets", keep)
    a.states_out, a.actions_out, a.z_out, a.err = (outs[k][1].data_ptr() for k in ("states", "actions", "z", "err"))
    a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel() * 4
    return a, keep


@pytest.mark.parametrize("name", ("zero_mean", "sphere", "none"))
def test_refusals_answer_minus_one_and_write_nothing(name):
    c, eng = IC.case(name), model(name).engine
    rows = 5
    outs = {k: G.guarded((H, 64, w), fill=None, device=DEV) for k, w in (("states", c.Db), ("actions", c.Da), ("z", c.Z))}
    outs["err"] = G.guarded((H,), fill=None, device=DEV)
    scratch = torch.zeros(int(eng.lib.pvae_imagine_scratch_bytes(eng.ctx, H)) // 4, device=DEV)
    null = _lib.ImagineSrc()

    def refused(edit, mode="track", rows=rows, horizon=H, word=b""):
        a, keep = _args(eng, c, mode, max(rows, 1) if rows <= 64 else 64, horizon, outs, scratch)
        a.rows = rows
        edit(a)
        rc = _raw(eng, a)
        torch.cuda.synchronize()
        assert rc == -1 and word in eng.lib.pvae_last_error(), (rc, eng.lib.pvae_last_error())
        for k, (b, v) in outs.items():
            assert not bool((b.view(torch.int32) != G.POISON_BITS).any()), k

    refused(lambda a: setattr(a, "s0", null), word=b"s0")
    refused(lambda a: None, rows=0, word=b"rows")
    refused(lambda a: None, rows=65, word=b"rows")
    refused(lambda a: None, horizon=0, word=b"horizon")
    refused(lambda a: setattr(a, "goals", null), mode="track", word=b"goals")
    refused(lambda a: setattr(a, "actions", null), mode="replay", word=b"actions")
    refused(lambda a: setattr(a, "mode", 7), word=b"mode")
    refused(lambda a: setattr(a, "targets", null), word=b"targets")
    refused(lambda a: setattr(a, "scratch_bytes", 8), word=b"scratch")
    if c.prior in (I.SPHERE, False):
        refused(lambda a: setattr(a, "z", null), mode="prior", word=b"needs z")
        with pytest.raises(ValueError, match="needs z"):
            eng.imagine("prior", dev(c.s0[:rows]), H)
    assert eng.lib.pvae_imagine(eng.ctx, None, None) == -1
    # and the accepted call still runs
    a, keep = _args(eng, c, "track", rows, H, outs, scratch)
    assert _raw(eng, a) == eng.imagine_launches("track")[0] * H + 2


# ---- 9. the trainer's hook -------------------------------------------------------------------------------------------
def test_evaluate_rollout_is_imagine_torch_over_the_same_windows():
    from physicsvae_amd import torch_models
    arch = R.make_arch(7, 3, latent=4, te=(16, 2), md=(24, 2), wm=(32, 2))
    data = R.synth_demo(seed=0, n_episodes=3, n_steps=15, dim_body=7, dim_action=3, kind="dynamics")
    tr = make_trainer(arch, data, 8, device=DEV)
    tr.model.load_state_dict(R.perturb_biases(R.init_state_dict(arch, 1), 3))       # (seeded: the same model whatever ran before)
    tr.model.latent_prior_noise = False
    ds = tr.train_loader.dataset
    sd = {k: v.detach().cpu() for k, v in tr.model.state_dict().items()}
    before = tr.engine.params.clone()
    for mode in ("track", "replay"):
        for horizon, cap in ((1, None), (4, None), (4, 5)):
            got = tr.evaluate_rollout(horizon, mode=mode, max_windows=cap)["horizon_mse"]
            starts = torch.from_numpy(torch_models.rollout_windows(ds, horizon, cap)).long()
            assert len(got) == horizon and len(starts) == (5 if cap else 3 * (15 - horizon)) and int(starts.max()) + horizon < len(ds.states)
            st, ac = torch.from_numpy(ds.states).double(), torch.from_numpy(ds.actions).double()
            nxt = torch.stack([st[starts + 1 + t] for t in range(horizon)])
            want = imagine_torch(tr.engine.arch, sd, mode, st[starts], horizon, goals=nxt if mode == "track" else None,
                                 actions=torch.stack([ac[starts + t] for t in range(horizon)]) if mode == "replay" else None,
                                 targets=nxt, noise=False)
            d = want["states"] - nxt
            ref = (d * d).mean(dim=(1, 2))
            e = float(((torch.tensor(got, dtype=torch.float64) - ref).abs() / ref).max())
            print(mode, horizon, cap, "horizon_mse", got, e)
            assert e <= IC.FORWARD_BOUND, (mode, horizon, e)
    # noise on: chunk i, step t draws at ROLLOUT_RNG_OFFSET + i * horizon + t of the trainer's seed
    tr.model.latent_prior_noise = True
    eng, horizon = tr.engine, 4
    assert torch.equal(before, eng.params)
    for k, v in eng.named_views().items():                     # (output layers at 30 x normc(0.01): the draws move the states)
        if k.endswith("._model.2._model.0.weight"):
            v.mul_(IC.OUT_GAIN)
    before = eng.params.clone()
    got = torch.tensor(tr.evaluate_rollout(horizon, mode="track")["horizon_mse"], dtype=torch.float64)
    starts = torch.from_numpy(torch_models.rollout_windows(ds, horizon)).to(DEV)
    assert len(starts) > 2 * eng.max_batch                     # (three chunks at least)
    st_dev = ds.device_arrays(eng.device)[0]

    def by_chunks(base, stride):
        total = torch.zeros(horizon, dtype=torch.float64)
        for i, lo in enumerate(range(0, len(starts), eng.max_batch)):
            idx = starts[lo: lo + eng.max_batch].contiguous()
            out = eng.imagine("track", (st_dev, idx), horizon, goals=(st_dev, idx, 1), targets=(st_dev, idx, 1), noise=True,
                              seed=tr.rng_seed, offset=base + i * stride, want=())
            total += out["err"].double().cpu() * idx.numel()
        return total / len(starts)
    want = by_chunks(tr.ROLLOUT_RNG_OFFSET, horizon)
    assert float(((got - want).abs() / want).max()) <= IC.FORWARD_BOUND, (got, want)
    # every chunk on chunk 0's draws is another result, and by more than the bound above lets pass: the comparison can tell
    # the chunks' offsets apart
    other = by_chunks(tr.ROLLOUT_RNG_OFFSET, 0)
    e = float(((got - other).abs() / other).max())
    print("chunk offsets: wrong stride moves horizon_mse by", e)
    assert e > IC.FORWARD_BOUND, e
    assert torch.equal(before, tr.engine.params)
    with pytest.raises(KeyError):
        tr.evaluate_rollout(2, data="validation")
