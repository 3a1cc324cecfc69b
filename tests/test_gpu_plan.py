"""Planning over imagined rollouts on the device (include/pvae.h pvae_plan; HipEngine.plan, PhysicsVAE.plan,
TrainModel.evaluate_plan) on the 42 configurations of tests/plan_cases.py (seven models, max_batch 64).

  1 stages        stage by stage on the device's own intermediates (selection is discontinuous, so nothing is compared
                  across it): z_cand, one step's states, a0 / s1 within ROLLOUT_BOUND of float64, cost within FORWARD_BOUND
                  relative of the float64 cost of the device's states, plan_z within FORWARD_BOUND of plan_select_torch on the
                  device's costs and candidates; best EQUAL to the argmin of the returned float32 cost; candidate 0 and the
                  lam == 0 copy bit for bit; the launch count as pvae_plan_launches states it
  2 consistency   K == 1 is imagine("prior") + a one-step call, bit for bit; one call of two iterations is two chained calls of
                  one; two calls agree in every byte; equal costs choose candidate 0; in-place sources give the dense bits
  3 module        PhysicsVAE.plan over two chunks is one engine call per chunk with its row0, and not with row0 = 0
  4 guards        every output and the scratch inside guard bands; outputs not asked for are not written
  5 refusals      every refusal answers -1 with its message and leaves the outputs alone
  6 trainer       evaluate_plan with one candidate is the open-loop rollout of the zero code; with more it is the composition
                  of plan and imagine, and no worse than the nominal"""
import ctypes as C

import pytest
import torch

import guards as G
import imagine_cases as IC
import infer_cases as I
import plan_cases as PC
from oracle import refpath as R
from physicsvae_amd import _lib
from physicsvae_amd import plan as P
from physicsvae_amd.engine_plan import PLAN_OUTPUTS
from physicsvae_amd.imagine import imagine_torch
from util import make_trainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, OFFSET = 11, 5
_MODELS = {}


def model(name):
    if name not in _MODELS:
        _MODELS[name] = I.module_for(IC.case(name), DEV)
    return _MODELS[name]


def dev(x):
    return None if x is None else x.to(DEV)


def run(c, iters=None, offset=OFFSET, nominal=None, noise=None, want=PLAN_OUTPUTS, **kw):
    """eng.plan on the case: its supplied noise, or Philox at (SEED, offset) where the case draws."""
    iters = c.iters if iters is None else iters
    if noise is None and not c.philox:
        noise = c.noise[:iters]
    args = dict(iters=iters, sigma=c.sigma, lam=c.lam, nominal=dev(c.nominal if nominal is None else nominal), noise=dev(noise),
                col_weight=dev(c.cw), step_weight=dev(c.sw), seed=SEED, offset=offset, want=want)
    args.update(kw)
    return model(c.model).engine.plan(dev(c.s0), dev(c.targets), c.H, c.K, **args)


def cpu(out):
    return {k: v.cpu() for k, v in out.items()}


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. stage by stage against float64 ------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", PC.CONFIG_IDS)
def test_stages_against_float64_on_the_devices_intermediates(cid):
    c, eng = PC.case(cid), model(PC.BY_ID[cid].model).engine
    got = cpu(run(c))
    per_step, per_iter, closing = eng.plan_launches()
    assert per_iter <= 3 and eng.plan_launched == c.iters * (c.H * per_step + per_iter) + closing
    assert closing == per_step + 1 and (c.m.prior == I.STATE_MEAN or per_step == eng.imagine_launches("prior")[0])
    u_in = PC.nominal_before_last(c, lambda iters: cpu(run(c, iters=iters, want=("plan_z",))))
    n = got["noise_out"].reshape(c.H, c.E, c.K, c.m.Z)
    assert not bool(n[:, :, 0].view(torch.int32).any())                       # candidate 0: the written noise is exactly 0.0
    if c.philox:
        assert bool((n[:, :, 1:] != 0).all()) and abs(float(n[:, :, 1:].std()) - 1.0) < 0.2
        if c.m.prior in (I.ZERO_MEAN, I.STATE_MEAN):                            # the sampler's draw of (seed, offset + i * H + t), row r
            for t in range(c.H):
                ref = eng.reparam(torch.zeros(c.rows, 2 * c.m.Z, device=DEV), seed=SEED, offset=OFFSET + (c.iters - 1) * c.H + t)
                assert torch.equal(n[t, :, 1:], ref.cpu().reshape(c.E, c.K, c.m.Z)[:, 1:]), t
    else:
        want = c.noise[c.iters - 1].reshape(c.H, c.E, c.K, c.m.Z).clone()
        want[:, :, 0] = 0
        assert torch.equal(n, want)
    zc = got["z_cand"].reshape(c.H, c.E, c.K, c.m.Z)
    if c.m.prior != I.SPHERE:
        assert same_bits(zc[:, :, 0], u_in)                                     # candidate 0 is the nominal, bit for bit
    e = PC.stage_errors(c, got, u_in, got["noise_out"])
    print(cid, e)
    for k, v in e.items():
        assert v <= PC.BOUNDS[k], (k, v)
    assert torch.equal(got["best"], P.plan_best_torch(got["cost"]))
    pick = torch.arange(c.E)
    assert torch.equal(got["iter_cost"][-1], got["cost"][pick, got["best"].long()])
    if c.lam == 0:
        assert same_bits(got["plan_z"], zc[:, pick, got["best"].long()])        # the selected candidate, copied
        ic = got["iter_cost"].double()                                          # candidate 0 carries the previous best
        assert bool((ic[1:] <= ic[:-1] * (1 + PC.FORWARD_BOUND)).all()), ic


# ---- 2. consistency -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [i for i in PC.CONFIG_IDS if PC.BY_ID[i].K == 1])
def test_one_candidate_is_imagine_and_a_one_step_call(cid):
    c, eng = PC.case(cid), model(PC.BY_ID[cid].model).engine
    got = run(c, iters=1)
    z = got["z_cand"]
    if c.m.prior != I.SPHERE:
        assert same_bits(z, dev(c.nominal))
    assert same_bits(got["plan_z"], z)
    ref = eng.imagine("prior", dev(c.s0), c.H, z=z, want=("states",))
    assert same_bits(got["states"], ref["states"])
    one = eng.imagine("prior", dev(c.s0), 1, z=got["plan_z"][:1].contiguous(), want=("states", "actions"))
    assert same_bits(got["a0"], one["actions"][0]) and same_bits(got["s1"], one["states"][0])


@pytest.mark.parametrize("cid", [i for i in PC.CONFIG_IDS if PC.BY_ID[i].iters == 2])
def test_two_iterations_are_two_chained_calls(cid):
    c = PC.case(cid)
    whole = run(c)
    first = run(c, iters=1)
    second = run(c, iters=1, offset=OFFSET + c.H, nominal=first["plan_z"], noise=None if c.philox else c.noise[1:2])
    for k in PLAN_OUTPUTS:
        if k != "iter_cost":
            assert same_bits(whole[k], second[k]), k
    assert same_bits(whole["iter_cost"], torch.cat([first["iter_cost"], second["iter_cost"]]))


@pytest.mark.parametrize("cid", ("zero_mean-2x32-H3-i2-mppi", "sphere-3x11-H3-i2-philox", "helper-3x11-H3-i2-w-mppi-philox"))
def test_two_calls_agree_in_every_byte(cid):
    c = PC.case(cid)
    a = {k: v.clone() for k, v in run(c).items()}
    model(c.model).engine.infer(torch.randn(7, 2 * c.m.Db, device=DEV))      # (another call in between)
    b = run(c)
    for k in PLAN_OUTPUTS:
        assert same_bits(a[k], b[k]), k


@pytest.mark.parametrize("cid", ("zero_mean-3x11-H1-i1-w", "sphere-2x32-H3-i1-w-mppi", "db1-1x5-H3-i1-w-mppi"))
def test_equal_costs_choose_candidate_zero(cid):
    c = PC.case(cid)
    got = cpu(run(c, sigma=0.0, noise=torch.zeros_like(c.noise)))
    assert bool((got["cost"].view(torch.int32) == got["cost"][:, :1].view(torch.int32)).all())
    assert got["best"].tolist() == [0] * c.E


@pytest.mark.parametrize("name", ("zero_mean", "db1"))
def test_in_place_sources_give_the_dense_bits(name):
    m, eng = IC.case(name), model(name).engine
    g = torch.Generator().manual_seed(4)
    N, E, K, H = 120, 5, 7, 3
    states = torch.randn(N, m.Db, generator=g).to(DEV)
    idx = torch.randint(0, N - H - 1, (E,), generator=g).to(torch.int32).to(DEV)
    li = idx.long()
    noise = torch.randn(1, H, E * K, m.Z, generator=g).to(DEV)
    dense = eng.plan(states[li], torch.stack([states[li + 1 + t] for t in range(H)]), H, K, noise=noise, want=PLAN_OUTPUTS)
    there = eng.plan((states, idx), (states, idx, 1), H, K, noise=noise, want=PLAN_OUTPUTS)
    for k in PLAN_OUTPUTS:
        assert same_bits(dense[k], there[k]), k


# ---- 3. the module's chunks -----------------------------------------------------------------------------------------
def test_module_chunks_number_their_rows_globally():
    name = "zero_mean"
    m, mod = IC.case(name), model(name)
    eng, E, K, H, iters = mod.engine, 7, 11, 3, 2
    g = torch.Generator().manual_seed(5)
    s0, targets = torch.randn(E, m.Db, generator=g).to(DEV), torch.randn(H, E, m.Db, generator=g).to(DEV)
    chunks = P.plan_chunks(E, K, eng.max_batch)
    assert len(chunks) == 2
    mod.seed(SEED)
    mod._rng_calls = OFFSET - 1
    want = PLAN_OUTPUTS
    out = mod.plan(s0, targets, H, K, iters=iters, sigma=0.5, lam=0.01, want=want)
    assert mod._rng_calls == OFFSET - 1 + iters * H
    again = mod.plan(s0, targets, H, K, iters=iters, sigma=0.5, lam=0.01, want=want, seed=SEED, offset=OFFSET)
    assert mod._rng_calls == OFFSET - 1 + iters * H                             # (overrides leave the counter alone)
    env_dim = lambda k: 0 if k in ("best", "cost", "a0", "s1") else 1        # noqa: E731

    def by_chunks(numbered):
        parts = [eng.plan(s0[lo:hi], targets[:, lo:hi], H, K, iters=iters, sigma=0.5, lam=0.01, seed=SEED, offset=OFFSET,
                          row0=row0 if numbered else 0, want=want) for lo, hi, row0 in chunks]
        return {k: torch.cat([p[k] for p in parts], dim=env_dim(k)) for k in want}
    right, wrong = by_chunks(True), by_chunks(False)
    for k in want:
        assert tuple(out[k].shape)[env_dim(k)] == (E * K if k in ("z_cand", "noise_out", "states") else E)
        assert same_bits(out[k], right[k]) and same_bits(again[k], right[k]), k
    lo = chunks[1][2]                                                          # the second chunk's rows: other noise wherever drawn
    drawn = (torch.arange(E * K, device=DEV) % K != 0) & (torch.arange(E * K, device=DEV) >= lo)
    assert bool((right["noise_out"][:, drawn] != wrong["noise_out"][:, drawn]).all())
    assert same_bits(right["noise_out"][:, :lo], wrong["noise_out"][:, :lo])
    with pytest.raises(ValueError, match="candidates"):
        mod.plan(s0, targets, H, eng.max_batch + 1)


# ---- 4. guard bands ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ("state_mean-3x11-H3-i1-w-mppi", "db1-2x32-H3-i1-w-mppi", "sphere-64x1-H1-i2", "helper-1x5-H1-i2"))
def test_outputs_and_scratch_stay_inside_their_guards(cid):
    c, eng = PC.case(cid), model(PC.BY_ID[cid].model).engine
    Db, Da, Z = c.m.Db, c.m.Da, c.m.Z
    shapes = {"plan_z": (c.H, c.E, Z), "best": (c.E,), "cost": (c.E, c.K), "iter_cost": (c.iters, c.E), "a0": (c.E, Da),
              "s1": (c.E, Db), "z_cand": (c.H, c.rows, Z), "noise_out": (c.H, c.rows, Z), "states": (c.H, c.rows, Db)}
    bufs = {k: G.guarded(s, fill=None, device=DEV) for k, s in shapes.items()}
    need = int(eng.lib.pvae_plan_scratch_bytes(eng.ctx, c.H, c.rows))
    assert need > 0 and need % 16 == 0
    sbuf, sview = G.guarded(need // 4, fill=None, device=DEV)
    keep = getattr(eng, "_plan_scratch", None)
    eng._plan_scratch = sview.view(torch.float64)
    views = {k: (v.view(torch.int32) if k == "best" else v) for k, (b, v) in bufs.items()}
    try:
        out = run(c, out=views)
        torch.cuda.synchronize()
        for k, (b, v) in bufs.items():
            assert G.guards_intact(b, v), k
            assert out[k].data_ptr() == v.data_ptr() and bool((v.view(torch.int32) != G.POISON_BITS).all()), k
        assert G.guards_intact(sbuf, sview)
        # outputs not asked for are not written
        for b, v in bufs.values():
            v.copy_(G.poison(v.numel(), DEV).view(v.shape))
        out = run(c, want=("a0",), out=views)
        torch.cuda.synchronize()
        assert set(out) == {"a0"}
        for k, (b, v) in bufs.items():
            assert G.guards_intact(b, v), k
            if k != "a0":
                assert not bool((v.view(torch.int32) != G.POISON_BITS).any()), k
        assert G.guards_intact(sbuf, sview)
    finally:
        eng._plan_scratch = keep


# ---- 5. refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("zero_mean", "sphere"))
def test_refusals_answer_minus_one_and_write_nothing(name):
    m, eng = IC.case(name), model(name).engine
    E, K, H, iters = 3, 5, 2, 2
    rows = E * K
    shapes = {"plan_z": (H, E, m.Z), "best": (E,), "cost": (E, K), "iter_cost": (iters, E), "a0": (E, m.Da), "s1": (E, m.Db),
              "z_cand": (H, rows, m.Z), "noise_out": (H, rows, m.Z), "states": (H, rows, m.Db)}
    outs = {k: G.guarded(s, fill=None, device=DEV) for k, s in shapes.items()}
    scratch = torch.zeros(int(eng.lib.pvae_plan_scratch_bytes(eng.ctx, H, rows)) // 4, device=DEV)
    s0, targets = dev(m.s0[:E]), dev(m.targets[:H, :E])
    null = _lib.ImagineSrc()

    def args():
        a, keep = _lib.PlanArgs(), []
        a.envs, a.candidates, a.horizon, a.iters, a.sigma, a.lam = E, K, H, iters, 0.5, 0.1
        a.s0 = eng._imagine_src(s0, m.Db, None, E, "s0", keep)
        a.targets = eng._imagine_src(targets, m.Db, H, E, "targets", keep)
        for k, (b, v) in outs.items():
            setattr(a, k, v.data_ptr())
        a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel() * 4
        return a, keep

    def refused(edit, word):
        a, keep = args()
        edit(a)
        rc = eng.lib.pvae_plan(eng.ctx, C.byref(a), None)
        torch.cuda.synchronize()
        assert rc == -1 and word in eng.lib.pvae_last_error(), (rc, eng.lib.pvae_last_error())
        for k, (b, v) in outs.items():
            assert not bool((b.view(torch.int32) != G.POISON_BITS).any()), k

    refused(lambda a: setattr(a, "s0", null), b"s0")
    refused(lambda a: setattr(a, "targets", null), b"targets")
    refused(lambda a: setattr(a, "envs", 0), b"envs")
    refused(lambda a: setattr(a, "candidates", 0), b"candidates")
    refused(lambda a: setattr(a, "candidates", _lib.PLAN_MAX_CANDIDATES + 1), b"candidates")
    refused(lambda a: setattr(a, "candidates", 22), b"rows")                   # 66 rows > max_batch
    refused(lambda a: setattr(a, "horizon", 0), b"horizon")
    refused(lambda a: setattr(a, "iters", 0), b"iters")
    for bad in (-0.5, float("inf"), float("nan")):
        refused(lambda a: setattr(a, "sigma", bad), b"sigma")
        refused(lambda a: setattr(a, "lam", bad), b"lam")
    refused(lambda a: setattr(a, "scratch", None), b"scratch")
    refused(lambda a: setattr(a, "scratch_bytes", scratch.numel() * 4 - 16), b"scratch")
    refused(lambda a: setattr(a, "scratch", scratch.data_ptr() + 8), b"aligned")
    assert eng.lib.pvae_plan(eng.ctx, None, None) == -1 and b"args" in eng.lib.pvae_last_error()
    with pytest.raises(ValueError, match="max_batch"):
        eng.plan(s0, targets, H, 22)
    # and the accepted call still runs, with the launches the library states
    a, keep = args()
    per_step, per_iter, closing = eng.plan_launches()
    assert eng.lib.pvae_plan(eng.ctx, C.byref(a), None) == iters * (H * per_step + per_iter) + closing
    torch.cuda.synchronize()


# ---- 6. the trainer's hook -------------------------------------------------------------------------------------------
def test_evaluate_plan_is_plan_then_the_open_loop_rollout():
    from physicsvae_amd import torch_models
    arch = R.make_arch(7, 3, latent=4, te=(16, 2), md=(24, 2), wm=(32, 2))
    data = R.synth_demo(seed=0, n_episodes=3, n_steps=15, dim_body=7, dim_action=3, kind="dynamics")
    tr = make_trainer(arch, data, 8, device=DEV)
    tr.model.load_state_dict(R.perturb_biases(R.init_state_dict(arch, 1), 3))
    eng, H = tr.engine, 4
    for k, v in eng.named_views().items():                     # (output layers at 30 x normc(0.01): the codes move the states)
        if k.endswith("._model.2._model.0.weight"):
            v.mul_(IC.OUT_GAIN)
    before = eng.params.clone()
    ds = tr.train_loader.dataset
    sd = {k: v.detach().cpu() for k, v in tr.model.state_dict().items()}
    starts = torch.from_numpy(torch_models.rollout_windows(ds, H)).long()
    st = torch.from_numpy(ds.states).double()
    nxt = torch.stack([st[starts + 1 + t] for t in range(H)])
    # one candidate: nothing to choose, the zero code replayed
    got = torch.tensor(tr.evaluate_plan(H, 1)["horizon_mse"], dtype=torch.float64)
    want = imagine_torch(eng.arch, sd, "prior", st[starts], H, z=torch.zeros(H, len(starts), 4, dtype=torch.float64), targets=nxt)
    d = want["states"] - nxt
    ref = (d * d).mean(dim=(1, 2))
    assert float(((got - ref).abs() / ref).max()) <= IC.FORWARD_BOUND, (got, ref)
    # four candidates, two iterations: the composition of plan and imagine over the same chunks, and no worse than the nominal
    K, iters = 4, 2
    planned = torch.tensor(tr.evaluate_plan(H, K, iters=iters, sigma=0.8)["horizon_mse"], dtype=torch.float64)
    chunks = P.plan_chunks(len(starts), K, eng.max_batch)
    assert len(chunks) > 2
    st_dev, index = ds.device_arrays(eng.device)[0], starts.to(torch.int32).to(DEV)
    total = torch.zeros(H, dtype=torch.float64)
    for i, (lo, hi, row0) in enumerate(chunks):
        idx = index[lo:hi].contiguous()
        p = eng.plan((st_dev, idx), (st_dev, idx, 1), H, K, iters=iters, sigma=0.8, seed=tr.rng_seed,
                     offset=tr.ROLLOUT_RNG_OFFSET + i * iters * H, row0=row0, want=("plan_z",))
        total += eng.imagine("prior", (st_dev, idx), H, z=p["plan_z"], targets=(st_dev, idx, 1), want=())["err"].double().cpu() * (hi - lo)
    assert float(((planned - total / len(starts)).abs() / planned).max()) <= IC.FORWARD_BOUND
    print("evaluate_plan: nominal", got.tolist(), "planned", planned.tolist())
    assert float(planned.sum()) <= float(got.sum()) * (1 + IC.FORWARD_BOUND) and float(planned.sum()) < float(got.sum())
    assert torch.equal(before, eng.params)
