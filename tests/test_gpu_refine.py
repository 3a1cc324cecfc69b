"""Backpropagation through imagined rollouts and gradient refinement on the device (include/pvae.h pvae_imagine_grad,
pvae_plan_refine; HipEngine.imagine_grad / .refine, PhysicsVAE.imagine_grad / .refine / .imagine_cost,
TrainModel.evaluate_plan(refine_steps=...)) on the configurations of tests/refine_cases.py (eight models, max_batch 64).

  1 gradients     cost within FORWARD_BOUND of the float64 cost of the device's states; dz_t, ds_t of every step within
                  GRAD_BOUND of the float64 one-step vector-Jacobian product at the device's s_t with the cotangent built from
                  the device's s_{t+1} and ds_{t+1}; the whole chain within CHAIN_BOUND of float64 backpropagation through
                  time; the launch count as pvae_imagine_grad_launches states it
  2 exact         cost is plan(K = 1)'s on the same codes and states_out imagine("prior", z)'s, bit for bit; two calls agree
                  in every byte; task_body's dz is +0.0 everywhere; parameters, gradient arena and Adam moments untouched
  3 refinement    every update within FORWARD_BOUND of one float64 Adam step on the device's iterate and gradients, the
                  exposed gradient within CHAIN_BOUND of float64; best_iter, plan_z, cost, a0 / s1 exactly what the returned
                  iter_cost and z_iters say; the launch count; descent after three steps
  4 guards        every output and the scratch inside guard bands; outputs not asked for keep their poison
  5 refusals      every refusal answers -1 with its word and writes nothing
  6 surfaces      the module's chunks, imagine_cost's backward, evaluate_plan(refine_steps)"""
import ctypes as C

import pytest
import torch

import guards as G
import imagine_cases as IC
import infer_cases as I
import refine_cases as RC
from oracle import refpath as R
from physicsvae_amd import _lib
from physicsvae_amd import refine as RF
from physicsvae_amd.engine_refine import GRAD_OUTPUTS, REFINE_OUTPUTS
from util import make_trainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
_MODELS = {}


def model(name):
    if name not in _MODELS:
        _MODELS[name] = I.module_for(IC.case(name), DEV)
    return _MODELS[name]


def dev(x):
    return None if x is None else x.to(DEV)


def cpu(out):
    return {k: v.cpu() for k, v in out.items()}


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_grad(c, want=GRAD_OUTPUTS, z=None, **kw):
    return model(c.model).engine.imagine_grad(dev(c.s0), dev(c.z) if z is None else z, dev(c.targets), group=c.G,
                                              col_weight=dev(c.cw), step_weight=dev(c.sw), want=want, **kw)


def run_refine(c, steps=None, want=REFINE_OUTPUTS, **kw):
    return model(c.model).engine.refine(dev(c.s0), dev(c.targets), c.H, c.steps if steps is None else steps, c.lr,
                                        nominal=dev(c.nominal), col_weight=dev(c.cw), step_weight=dev(c.sw), want=want, **kw)


def arenas(eng):
    return [t.clone() for t in (eng.params, eng.grads, eng.exp_avg, eng.exp_avg_sq)]


# ---- 1. gradients against float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", RC.GRAD_IDS)
def test_gradients_against_float64_on_the_devices_intermediates(cid):
    c, eng = RC.grad_case(cid), model(RC.BY_ID[cid].model).engine
    before = arenas(eng)
    got = cpu(run_grad(c))
    assert eng.imagine_grad_launched == eng.imagine_grad_launches(c.H)
    f, b, per_call = eng.imagine_grad_launches()
    assert f == eng.plan_launches()[0] and per_call == 1 and b == sum(
        len(getattr(c.m, k)[0]) + 1 for k in ("wm", "md", "mh") if getattr(c.m, k) is not None) + 2
    e = RC.grad_errors(c, got)
    print(cid, e)
    for k, v in e.items():
        assert v <= RC.BOUNDS[k], (k, v)
    if not RC.reads_code(c.m):
        assert not bool(got["dz"].view(torch.int32).any())                       # +0.0 bits everywhere
    else:
        assert bool((got["dz"] != 0).any())
    for x, y in zip(before, arenas(eng)):
        assert torch.equal(x, y)
    # forward only: the same cost and states with the forward's launches alone
    fwd = run_grad(c, want=("cost", "states"))
    assert eng.imagine_grad_launched == eng.imagine_grad_launches(c.H, backward=False)
    assert same_bits(fwd["cost"].cpu(), got["cost"]) and same_bits(fwd["states"].cpu(), got["states"])


# ---- 2. exact properties --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", RC.GRAD_IDS)
def test_cost_is_plans_and_states_are_imagines_bit_for_bit(cid):
    c, eng = RC.grad_case(cid), model(RC.BY_ID[cid].model).engine
    s0_rows, tg_rows = dev(c.s0).repeat_interleave(c.G, dim=0), dev(c.targets).repeat_interleave(c.G, dim=1)
    p = eng.plan(s0_rows, tg_rows, c.H, 1, iters=1, nominal=dev(c.z), col_weight=dev(c.cw), step_weight=dev(c.sw),
                 want=("cost", "z_cand", "states"))
    z = p["z_cand"].clone()                                   # (under the sphere: the projected codes plan unrolled)
    a = {k: v.clone() for k, v in run_grad(c, z=z).items()}
    assert same_bits(a["cost"], p["cost"].reshape(-1)) and same_bits(a["states"], p["states"])
    ref = eng.imagine("prior", s0_rows, c.H, z=z, want=("states",))
    assert same_bits(a["states"], ref["states"])
    eng.infer(torch.randn(7, 2 * c.m.Db, device=DEV))         # (another call in between)
    b = run_grad(c, z=z)
    for k in GRAD_OUTPUTS:
        assert same_bits(a[k], b[k]), k


# ---- 3. refinement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", RC.REFINE_IDS)
def test_refinement_updates_and_keeps_the_best_iterate(cid):
    c, eng = RC.refine_case(cid), model(RC.BY_ID[cid].model).engine
    before = arenas(eng)
    runs = {}

    def run(steps):
        if steps not in runs:
            runs[steps] = cpu(run_refine(c, steps))
            assert eng.refine_launched == eng.refine_launches(c.H, steps)
        return runs[steps]
    got = run(c.steps)
    e = RC.refine_errors(c, run)
    print(cid, e)
    for k, v in e.items():
        assert v <= RC.BOUNDS[k], (k, v)
    for x, y in zip(before, arenas(eng)):
        assert torch.equal(x, y)
    ic, pick = got["iter_cost"], torch.arange(c.E)
    assert torch.equal(got["best_iter"], RF.best_iter_torch(ic))
    assert same_bits(got["plan_z"], got["z_iters"][got["best_iter"].long(), :, pick].permute(1, 0, 2))
    assert same_bits(got["cost"], ic[got["best_iter"].long(), pick]) and bool((got["cost"] <= ic[0]).all())
    if c.m.prior != I.SPHERE:
        assert same_bits(got["z_iters"][0], c.nominal)
    if c.steps == 0:
        assert same_bits(got["plan_z"], got["z_iters"][0]) and not bool(got["grad"].view(torch.int32).any())
    one = eng.imagine("prior", dev(c.s0), 1, z=dev(got["plan_z"][:1]).contiguous(), want=("states", "actions"))
    assert same_bits(got["a0"], one["actions"][0].cpu()) and same_bits(got["s1"], one["states"][0].cpu())
    for i in range(c.steps + 1):                              # every stored cost is imagine_grad's of that iterate
        g = eng.imagine_grad(dev(c.s0), dev(got["z_iters"][i]), dev(c.targets), col_weight=dev(c.cw), step_weight=dev(c.sw),
                             want=("cost",))
        assert same_bits(g["cost"].cpu(), ic[i]), i
    again = cpu(run_refine(c))
    for k in REFINE_OUTPUTS:
        assert same_bits(again[k], got[k]), k
    if c.steps == 3:
        if RC.reads_code(c.m):
            assert float(ic[3].double().sum()) < float(ic[0].double().sum()), ic.double().sum(dim=1)
        else:
            assert got["best_iter"].tolist() == [0] * c.E and same_bits(ic[3], ic[0])


# ---- 4. guard bands -------------------------------------------------------------------------------------------------------
def _guarded_call(eng, shapes, scratch_bytes, call, keep_one):
    bufs = {k: G.guarded(s, fill=None, device=DEV) for k, s in shapes.items()}
    assert scratch_bytes > 0 and scratch_bytes % 16 == 0
    sbuf, sview = G.guarded(scratch_bytes // 4, fill=None, device=DEV)
    keep = getattr(eng, "_refine_scratch", None)
    eng._refine_scratch = sview.view(torch.float64)
    views = {k: (v.view(torch.int32) if k == "best_iter" else v) for k, (b, v) in bufs.items()}
    try:
        out = call(tuple(shapes), views)
        torch.cuda.synchronize()
        for k, (b, v) in bufs.items():
            assert G.guards_intact(b, v), k
            assert out[k].data_ptr() == v.data_ptr() and bool((v.view(torch.int32) != G.POISON_BITS).all()), k
        assert G.guards_intact(sbuf, sview)
        for b, v in bufs.values():                            # outputs not asked for are not written
            v.copy_(G.poison(v.numel(), DEV).view(v.shape))
        out = call((keep_one,), views)
        torch.cuda.synchronize()
        assert set(out) == {keep_one}
        for k, (b, v) in bufs.items():
            assert G.guards_intact(b, v), k
            if k != keep_one:
                assert not bool((v.view(torch.int32) != G.POISON_BITS).any()), k
        assert G.guards_intact(sbuf, sview)
    finally:
        eng._refine_scratch = keep


@pytest.mark.parametrize("cid", ("state_mean-3x11-H3-w", "db1-64x1-H1-w", "helper-5x1-H3-w", "sphere-1x1-H1"))
def test_gradient_outputs_and_scratch_stay_inside_their_guards(cid):
    c, eng = RC.grad_case(cid), model(RC.BY_ID[cid].model).engine
    shapes = {"cost": (c.rows,), "dz": (c.H, c.rows, c.m.Z), "ds": (c.H, c.rows, c.m.Db), "states": (c.H, c.rows, c.m.Db)}
    for keep_one in ("cost", "dz"):
        _guarded_call(eng, shapes, int(eng.lib.pvae_imagine_grad_scratch_bytes(eng.ctx, c.H, c.rows)),
                      lambda want, views: run_grad(c, want=want, out=views), keep_one)


@pytest.mark.parametrize("cid", ("state_mean-E33-s3-H3-w", "db1-E5-s1-H3", "sphere-E1-s3-H1", "helper-E5-s0-H3-w"))
def test_refinement_outputs_and_scratch_stay_inside_their_guards(cid):
    c, eng = RC.refine_case(cid), model(RC.BY_ID[cid].model).engine
    Z, E, H, S = c.m.Z, c.E, c.H, c.steps
    shapes = {"plan_z": (H, E, Z), "cost": (E,), "best_iter": (E,), "iter_cost": (S + 1, E), "a0": (E, c.m.Da), "s1": (E, c.m.Db),
              "z_iters": (S + 1, H, E, Z), "grad": (H, E, Z)}
    _guarded_call(eng, shapes, int(eng.lib.pvae_plan_refine_scratch_bytes(eng.ctx, H, E)),
                  lambda want, views: run_refine(c, want=want, out=views), "a0")


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("zero_mean", "sphere"))
def test_refusals_answer_minus_one_and_write_nothing(name):
    m, eng = IC.case(name), model(name).engine
    E, Gr, H, S = 3, 5, 2, 2
    rows = E * Gr
    s0, targets, z = dev(m.s0[:E]), dev(m.targets[:H, :E]), dev(m.z[:H, :rows]).contiguous()
    null = _lib.ImagineSrc()

    def check(fn, make, outs, edit, word):
        a, keep = make()
        edit(a)
        rc = fn(eng.ctx, C.byref(a), None)
        torch.cuda.synchronize()
        assert rc == -1 and word in eng.lib.pvae_last_error(), (rc, eng.lib.pvae_last_error())
        for k, (b, v) in outs.items():
            assert not bool((b.view(torch.int32) != G.POISON_BITS).any()), k

    # pvae_imagine_grad
    g_shapes = {"cost": (rows,), "dz": (H, rows, m.Z), "ds": (H, rows, m.Db), "states_out": (H, rows, m.Db)}
    g_outs = {k: G.guarded(s, fill=None, device=DEV) for k, s in g_shapes.items()}
    g_scratch = torch.zeros(int(eng.lib.pvae_imagine_grad_scratch_bytes(eng.ctx, H, rows)) // 4, device=DEV)

    def g_args():
        a, keep = _lib.ImagineGradArgs(), []
        a.envs, a.group, a.horizon = E, Gr, H
        a.s0 = eng._imagine_src(s0, m.Db, None, E, "s0", keep)
        a.targets = eng._imagine_src(targets, m.Db, H, E, "targets", keep)
        a.z = z.data_ptr()
        for k, (b, v) in g_outs.items():
            setattr(a, k, v.data_ptr())
        a.scratch, a.scratch_bytes = g_scratch.data_ptr(), g_scratch.numel() * 4
        return a, keep
    fn = eng.lib.pvae_imagine_grad
    check(fn, g_args, g_outs, lambda a: setattr(a, "s0", null), b"s0")
    check(fn, g_args, g_outs, lambda a: setattr(a, "targets", null), b"targets")
    check(fn, g_args, g_outs, lambda a: setattr(a, "z", None), b"z is null")
    check(fn, g_args, g_outs, lambda a: setattr(a, "envs", 0), b"envs")
    check(fn, g_args, g_outs, lambda a: setattr(a, "group", 0), b"group")
    check(fn, g_args, g_outs, lambda a: setattr(a, "group", 22), b"rows")                # 66 rows > max_batch
    check(fn, g_args, g_outs, lambda a: setattr(a, "horizon", 0), b"horizon")
    check(fn, g_args, g_outs, lambda a: setattr(a, "scratch", None), b"scratch")
    check(fn, g_args, g_outs, lambda a: setattr(a, "scratch_bytes", g_scratch.numel() * 4 - 16), b"scratch")
    check(fn, g_args, g_outs, lambda a: setattr(a, "scratch", g_scratch.data_ptr() + 8), b"aligned")
    assert fn(eng.ctx, None, None) == -1 and b"args" in eng.lib.pvae_last_error()
    with pytest.raises(ValueError, match="max_batch"):
        eng.imagine_grad(s0, dev(m.z[:H, :66]), targets, group=22)
    a, keep = g_args()
    assert fn(eng.ctx, C.byref(a), None) == eng.imagine_grad_launches(H)               # the accepted call still runs
    torch.cuda.synchronize()

    # pvae_plan_refine
    r_shapes = {"plan_z": (H, E, m.Z), "cost": (E,), "best_iter": (E,), "iter_cost": (S + 1, E), "a0": (E, m.Da), "s1": (E, m.Db),
                "z_iters": (S + 1, H, E, m.Z), "grad": (H, E, m.Z)}
    r_outs = {k: G.guarded(s, fill=None, device=DEV) for k, s in r_shapes.items()}
    r_scratch = torch.zeros(int(eng.lib.pvae_plan_refine_scratch_bytes(eng.ctx, H, E)) // 4, device=DEV)

    def r_args():
        a, keep = _lib.PlanRefineArgs(), []
        a.envs, a.horizon, a.steps, a.lr = E, H, S, 0.05
        a.s0 = eng._imagine_src(s0, m.Db, None, E, "s0", keep)
        a.targets = eng._imagine_src(targets, m.Db, H, E, "targets", keep)
        for k, (b, v) in r_outs.items():
            setattr(a, k, v.data_ptr())
        a.scratch, a.scratch_bytes = r_scratch.data_ptr(), r_scratch.numel() * 4
        return a, keep
    fn = eng.lib.pvae_plan_refine
    check(fn, r_args, r_outs, lambda a: setattr(a, "s0", null), b"s0")
    check(fn, r_args, r_outs, lambda a: setattr(a, "targets", null), b"targets")
    check(fn, r_args, r_outs, lambda a: setattr(a, "envs", 0), b"envs")
    check(fn, r_args, r_outs, lambda a: setattr(a, "envs", 65), b"rows")
    check(fn, r_args, r_outs, lambda a: setattr(a, "horizon", 0), b"horizon")
    check(fn, r_args, r_outs, lambda a: setattr(a, "steps", -1), b"steps")
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        check(fn, r_args, r_outs, lambda a: setattr(a, "lr", bad), b"lr")
    check(fn, r_args, r_outs, lambda a: setattr(a, "scratch", None), b"scratch")
    check(fn, r_args, r_outs, lambda a: setattr(a, "scratch_bytes", r_scratch.numel() * 4 - 16), b"scratch")
    check(fn, r_args, r_outs, lambda a: setattr(a, "scratch", r_scratch.data_ptr() + 8), b"aligned")
    assert fn(eng.ctx, None, None) == -1 and b"args" in eng.lib.pvae_last_error()
    with pytest.raises(ValueError, match="max_batch"):
        eng.refine(dev(m.s0[:65]), dev(m.targets[:H, :65]), H, 1, 0.05)
    with pytest.raises(ValueError, match="lr"):
        eng.refine(s0, targets, H, 1, 0.0)
    a, keep = r_args()
    assert fn(eng.ctx, C.byref(a), None) == eng.refine_launches(H, S)
    torch.cuda.synchronize()


# ---- 6. surfaces ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("zero_mean", "sphere"))
def test_module_chunks_are_the_dense_engine_calls(name):
    m, mod = IC.case(name), model(name)
    eng = mod.engine
    g = torch.Generator().manual_seed(6)
    E, Gr, H = 7, 11, 3
    s0, targets = torch.randn(E, m.Db, generator=g).to(DEV), torch.randn(H, E, m.Db, generator=g).to(DEV)
    z = torch.randn(H, E * Gr, m.Z, generator=g).to(DEV)
    calls = mod._rng_calls
    chunks = RF.refine_chunks(E, Gr, eng.max_batch)
    assert chunks == [(0, 5), (5, 7)]
    out = mod.imagine_grad(s0, z, targets, group=Gr, want=GRAD_OUTPUTS)
    parts = [eng.imagine_grad(s0[lo:hi], z[:, lo * Gr: hi * Gr].contiguous(), targets[:, lo:hi], group=Gr, want=GRAD_OUTPUTS)
             for lo, hi in chunks]
    for k in GRAD_OUTPUTS:
        assert same_bits(out[k], torch.cat([p[k] for p in parts], dim=0 if k == "cost" else 1)), k
    E = 70
    s0, targets = dev(m.s0[:E]), dev(m.targets[:H, :E])
    nominal = 0.5 * dev(m.z[:H, :E])
    out = mod.refine(s0, targets, H, 2, RC.LR, nominal=nominal, want=REFINE_OUTPUTS)
    parts = [eng.refine(s0[lo:hi], targets[:, lo:hi], H, 2, RC.LR, nominal=nominal[:, lo:hi], want=REFINE_OUTPUTS)
             for lo, hi in ((0, 64), (64, 70))]
    dims = {"cost": 0, "best_iter": 0, "a0": 0, "s1": 0, "iter_cost": 1, "plan_z": 1, "grad": 1, "z_iters": 2}
    for k in REFINE_OUTPUTS:
        assert tuple(out[k].shape)[dims[k]] == E and same_bits(out[k], torch.cat([p[k] for p in parts], dim=dims[k])), k
    assert mod._rng_calls == calls                            # nothing is drawn


@pytest.mark.parametrize("name", ("helper", "task_body"))
def test_imagine_cost_backward_is_imagine_grads_dz(name):
    m, mod = IC.case(name), model(name)
    H = 3
    for E, Gr in ((5, 1), (3, 4)):
        s0 = dev(m.s0[:E]).clone().requires_grad_(Gr == 1)
        z = dev(m.z[:H, :E * Gr]).contiguous().clone().requires_grad_(True)
        targets = dev(m.targets[:H, :E])
        before = [p.grad for p in mod.parameters()]
        cost = mod.imagine_cost(s0, z, targets, group=Gr)
        cost.sum().backward()
        ref = mod.engine.imagine_grad(s0.detach(), z.detach(), targets, group=Gr, want=("cost", "dz", "ds"))
        assert same_bits(cost.detach(), ref["cost"]) and same_bits(z.grad, ref["dz"])
        if Gr == 1:
            assert same_bits(s0.grad, ref["ds"][0])
        assert all(p.grad is q for p, q in zip(mod.parameters(), before))       # the parameters get no gradient
        z.grad = None
        w = torch.linspace(0.5, 2.0, E * Gr, device=DEV)
        (mod.imagine_cost(s0.detach(), z, targets, group=Gr) * w).sum().backward()
        assert torch.equal(z.grad, w[None, :, None] * ref["dz"])


def test_evaluate_plan_with_refinement_is_no_worse_per_window():
    arch = R.make_arch(7, 3, latent=4, te=(16, 2), md=(24, 2), wm=(32, 2))
    data = R.synth_demo(seed=0, n_episodes=3, n_steps=15, dim_body=7, dim_action=3, kind="dynamics")
    tr = make_trainer(arch, data, 8, device=DEV)
    tr.model.load_state_dict(R.perturb_biases(R.init_state_dict(arch, 1), 3))
    eng, H, K = tr.engine, 4, 4
    for k, v in eng.named_views().items():                     # (output layers at 30 x normc(0.01): the codes move the states)
        if k.endswith("._model.2._model.0.weight"):
            v.mul_(IC.OUT_GAIN)
    before = eng.params.clone()
    plain = tr.evaluate_plan(H, K, iters=2, sigma=0.8)
    zero = tr.evaluate_plan(H, K, iters=2, sigma=0.8, refine_steps=0)
    assert set(plain) == set(zero) == {"horizon_mse"} and plain["horizon_mse"] == zero["horizon_mse"]
    got = tr.evaluate_plan(H, K, iters=2, sigma=0.8, refine_steps=2, refine_lr=RC.LR)
    refined = torch.tensor(got["window_cost"], dtype=torch.float64)
    unrefined = torch.tensor(got["window_cost_unrefined"], dtype=torch.float64)
    assert refined.numel() == unrefined.numel() > eng.max_batch // K
    assert bool((refined <= unrefined).all()) and float(refined.sum()) < float(unrefined.sum())
    # the unrefined window costs are the plain call's: summed over the windows they are its horizon errors (J = sum_t mean_c d^2)
    total = float(torch.tensor(plain["horizon_mse"], dtype=torch.float64).sum())
    assert abs(float(unrefined.mean()) - total) / total <= IC.FORWARD_BOUND
    print("evaluate_plan: planned", plain["horizon_mse"], "refined", got["horizon_mse"])
    assert sum(got["horizon_mse"]) < sum(plain["horizon_mse"])
    assert torch.equal(before, eng.params)
