"""Torch autograd through the module (physicsvae_amd/autograd.py; include/pvae.h pvae_net_backward /
pvae_reparam_backward): what PPO's loss.backward() does to PhysicsVAE.forward and the stage functions when the encoder and
decoder are learnable (rmt:473, 488, 743-771), checked against oracle.refpath.RefModel on the CPU with torch autograd and
the same draws.  Gradients use the parity suite's bound (max_err_scaled < 1e-4)."""
import math

import numpy as np
import pytest
import torch

from oracle import refpath as R
from physicsvae_amd import _lib
from physicsvae_amd import autograd as AG
from physicsvae_amd.model import PhysicsVAE
from physicsvae_amd.spaces import Box
from util import arch_from_meta, max_err_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda"
STACKS = {"_task_encoder": _lib.NET_TE, "_motor_decoder": _lib.NET_MD, "_world_model": _lib.NET_WM,
          "_latent_prior": _lib.NET_PR, "_motor_decoder_helper": _lib.NET_MH}


def build(arch, max_batch=256, lookahead=1, seed=1):
    """A PhysicsVAE of `arch` (RefModel's description) on the GPU and the RefModel holding the same weights."""
    Db, Da = arch["Db"], arch["Da"]
    act = arch.get("act", "relu")
    prior = arch.get("prior", R.PRIORS[0])
    cmc = dict(observation_space=Box(np.zeros(2 * Db), np.zeros(2 * Db)), observation_space_body=Box(np.zeros(Db), np.zeros(Db)),
               observation_space_task=Box(np.zeros(Db), np.zeros(Db)), action_space=Box(np.zeros(Da), np.zeros(Da)),
               task_encoder_layers=R.fc_layer_list(arch["te"], act), motor_decoder_layers=R.fc_layer_list(arch["md"], act),
               world_model_layers=R.fc_layer_list(arch["wm"], act), task_encoder_output_dim=arch["Z"],
               latent_prior_type=prior, device=DEV, max_batch=max_batch, lookahead=lookahead,
               task_encoder_inputs=list(arch.get("te_inputs", R.BOTH)), motor_decoder_inputs=list(arch.get("md_inputs", R.BOTH)))
    if prior == R.PRIORS[1]:
        cmc["latent_prior_layers"] = R.fc_layer_list(arch["pr"], act)
    if arch.get("mh"):
        layers = R.fc_layer_list(arch["mh"], act)
        layers[-1]["activation"] = "tanh"
        cmc.update(motor_decoder_helper_enable=True, motor_decoder_helper_layers=layers,
                   motor_decoder_helper_range=arch["mh_range"])
    m = PhysicsVAE(cmc["observation_space"], cmc["action_space"], 2 * Da, {"custom_model_config": cmc}, "physics_vae")
    sd = R.perturb_biases(R.init_state_dict(arch, seed=seed), seed=seed + 2)
    if arch.get("mh"):                        # a helper term as large as the decoder's (its default output std is 0.01)
        k = "_motor_decoder_helper._model.%d._model.0.weight" % len(arch["mh"])
        sd[k] = sd[k] * 60.0
    m.load_state_dict(sd)
    ref = R.RefModel(arch)
    ref.load_state_dict(sd)
    return m, ref


def tiny(**kw):
    return R.make_arch(7, 3, latent=4, te=(16, 2), md=(24, 2), wm=(32, 2), **kw)


def grads_match(m, ref, nets, bound=1e-4):
    for name in nets:
        mine = dict(getattr(m, name).named_parameters())
        for k, q in getattr(ref, name).named_parameters():
            p = mine[k]
            if q.grad is None:                   # (no path to the loss upstream: structural zeros here, e.g. a decoder on s_t only)
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, (name, k)
                continue
            assert p.grad is not None, (name, k)
            err = max_err_scaled(p.grad.cpu(), q.grad)
            assert err < bound, (name, k, err)


def zero_grads(*mods):
    for mod in mods:
        for p in mod.parameters():
            p.grad = None


def rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


_MODELS = {}


def fixture_model(golden, name):
    if name not in _MODELS:
        _MODELS[name] = build(arch_from_meta(golden(name)))
    return _MODELS[name]


@pytest.mark.parametrize("name", ["single_tiny", "single_default", "single_tiny_tanh", "single_tiny_elu", "single_tiny_sigmoid"])
def test_forward_backward_reaches_every_encoder_and_decoder_parameter(golden, name):
    """forward() -> (logits[:, :Da]**2).sum().backward(): every TE and MD parameter gets the RefModel's gradient, at 1, 3,
    4 (the rollout GEMV path), 5, 33 and 256 rows, with supplied draws, Philox draws (read back) and noise off."""
    m, ref = fixture_model(golden, name)
    arch = ref.arch
    Db, Da, Z = arch["Db"], arch["Da"], arch["Z"]
    for rows in (1, 3, 4, 5, 33, 256):
        obs = rand(rows, 2 * Db, seed=rows)
        for mode in ("eps", "philox", "off"):
            m.latent_prior_noise = ref.latent_prior_noise = mode != "off"
            eps = rand(rows, Z, seed=100 + rows) if mode == "eps" else None
            zero_grads(m, ref)
            logits, _ = m.forward({"obs_flat": obs.to(DEV)}, [], None, eps=eps.to(DEV) if eps is not None else None)
            used = m.engine.read("eps", rows).cpu() if mode == "philox" else eps
            (logits[:, :Da] ** 2).sum().backward()
            ref.eps_source = (lambda shape, e=used: e) if used is not None else None
            want = ref(obs)
            (want[:, :Da] ** 2).sum().backward()
            assert max_err_scaled(logits.detach().cpu(), want.detach()) < 1e-5, (rows, mode)
            grads_match(m, ref, ["_task_encoder", "_motor_decoder"])
    m.latent_prior_noise = ref.latent_prior_noise = True


def stack_check(m, ref, net_name, rows, seed=0):
    """HipNet on one stack against the RefModel's stack on a random dy: dx and every parameter gradient."""
    arch = ref.arch
    Db, Z = arch["Db"], arch["Z"]
    eng, net = m.engine, STACKS[net_name]
    n_in = [l for l in eng.layers if l["net"] == net][0]
    full = {_lib.NET_TE: 2 * Db, _lib.NET_MD: Db + Z, _lib.NET_MH: Db + Z, _lib.NET_WM: Db + arch["Da"], _lib.NET_PR: Db}[net]
    x = rand(rows, full, seed=seed)
    win = slice(n_in["col0"], n_in["col0"] + n_in["n_in"])
    zero_grads(m, ref)
    xg = x.clone().to(DEV).requires_grad_(True)
    out = AG.HipNet.apply(eng, net, xg, *m._stack_params(net))
    dy = rand(*out.shape, seed=seed + 1)
    out.backward(dy.to(DEV))
    xr = x[:, win].clone().requires_grad_(True)
    want = getattr(ref, net_name)(xr)
    want.backward(dy)
    assert max_err_scaled(out.detach().cpu(), want.detach()) < 1e-5
    dx = xg.grad.cpu()
    assert max_err_scaled(dx[:, win], xr.grad) < 1e-4, (net_name, rows)
    outside = torch.ones(full, dtype=torch.bool)
    outside[win] = False
    assert float(dx[:, outside].abs().max() if outside.any() else 0.0) == 0.0
    grads_match(m, ref, [net_name])


@pytest.mark.parametrize("cfg", ["zero_mean", "state_mean", "hypersphere", "none", "te_body", "te_task", "md_body",
                                 "md_task", "helper", "look2"])
def test_each_stack_prior_kind_and_input_subset(cfg):
    """HipNet per stack (TE, MD, WM, the learned prior, the helper with its tanh output) against the RefModel stack, then the
    module's graph-building forward (the fused call, or stage by stage: learned prior, lookahead-2 engines) against the
    RefModel: every prior kind, both input subsets of encoder and decoder."""
    arch = tiny()
    kw = {}
    if cfg in ("state_mean", "hypersphere"):
        arch = tiny(prior={"state_mean": R.PRIORS[1], "hypersphere": R.PRIORS[2]}[cfg])
    elif cfg == "none":
        arch = tiny(prior=False)
    elif cfg.startswith("te_"):
        arch = R.with_inputs(arch, te_inputs=(cfg[3:],))
    elif cfg.startswith("md_"):
        arch = R.with_inputs(arch, md_inputs=(cfg[3:],))
    elif cfg == "helper":
        arch = R.with_helper(arch, hidden=((16, "relu"), (16, "tanh")))
    elif cfg == "look2":
        kw["lookahead"] = 2
    m, ref = build(arch, max_batch=64, **kw)
    nets = ["_task_encoder", "_motor_decoder", "_world_model"] + (["_latent_prior"] if cfg == "state_mean" else []) \
        + (["_motor_decoder_helper"] if cfg == "helper" else [])
    for rows in (3, 37):
        for net_name in nets:
            stack_check(m, ref, net_name, rows, seed=rows)
    Db, Da, Z = arch["Db"], arch["Da"], arch["Z"]
    for rows in (2, 37):
        obs, eps = rand(rows, 2 * Db, seed=7 + rows), rand(rows, Z, seed=8 + rows)
        zero_grads(m, ref)
        logits, _ = m.forward({"obs_flat": obs.to(DEV)}, [], None, eps=eps.to(DEV))
        loss = (logits[:, :Da] ** 2).sum() + (m._cur_future_state ** 2).sum()
        if cfg == "state_mean":
            loss = loss + (m._cur_latent_prior_mu ** 2).sum()
        loss.backward()
        ref.eps_source = lambda shape, e=eps: e
        want = ref(obs)
        rloss = (want[:, :Da] ** 2).sum() + (ref.cur_future_state ** 2).sum()
        if cfg == "state_mean":
            rloss = rloss + (ref.cur_prior_mu ** 2).sum()
        rloss.backward()
        assert abs(float(loss) - float(rloss)) <= 1e-5 * abs(float(rloss)), (cfg, rows)
        grads_match(m, ref, nets)


def test_chunked_batches_forward_and_world_model():
    """Rows 257 and 600 (max_batch 256) through forward() and forward_world, with and without grad: values match the
    RefModel; gradients match a single-chunk engine (max_batch 640) and the RefModel."""
    arch = tiny()
    m, ref = build(arch, max_batch=256)
    m1, _ = build(arch, max_batch=640)
    Db, Da, Z = arch["Db"], arch["Da"], arch["Z"]
    for rows in (257, 600):
        obs, eps = rand(rows, 2 * Db, seed=rows), rand(rows, Z, seed=rows + 1)
        ref.eps_source = lambda shape, e=eps: e
        want = ref(obs)
        with torch.no_grad():
            lg, _ = m.forward({"obs_flat": obs.to(DEV)}, [], None, eps=eps.to(DEV))
            s2 = m.forward_world(obs.to(DEV), lg)
        assert lg.shape == (rows, 2 * Da) and max_err_scaled(lg.cpu(), want.detach()) < 1e-5
        assert max_err_scaled(s2.cpu(), ref.cur_future_state.detach()) < 1e-5
        grads = []
        for mod in (m, m1):
            zero_grads(mod)
            lg, _ = mod.forward({"obs_flat": obs.to(DEV)}, [], None, eps=eps.to(DEV))
            s2 = mod.forward_world(obs.to(DEV), lg)
            ((lg[:, :Da] ** 2).sum() + (s2 ** 2).sum()).backward()
            assert max_err_scaled(lg.detach().cpu(), want.detach()) < 1e-5
            grads.append({k: p.grad.clone() for k, p in mod.named_parameters() if p.grad is not None and "_value" not in k})
        zero_grads(ref)
        ((want[:, :Da] ** 2).sum() + (ref.forward_world(obs, want) ** 2).sum()).backward()
        grads_match(m, ref, ["_task_encoder", "_motor_decoder", "_world_model"])
        assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 0
        for k in grads[0]:
            assert max_err_scaled(grads[0][k].cpu(), grads[1][k].cpu()) < 1e-4, k


def test_accumulate_is_the_sum_of_two_stores_bit_for_bit():
    """net_backward(accumulate=1) twice into one buffer == the sum of two stored calls, bit for bit (every gradient tile is
    summed by one workgroup in a fixed order), at the rows of every weight-gradient geometry."""
    m, _ = build(R.make_arch(197, 45, latent=32, te=(256, 2), md=(512, 3), wm=(1024, 2)), max_batch=256)
    eng = m.engine
    for net in (_lib.NET_TE, _lib.NET_MD, _lib.NET_WM):
        cnt = eng.segments[net][1]
        n_in = {_lib.NET_TE: 2 * 197, _lib.NET_MD: 197 + 32, _lib.NET_WM: 197 + 45}[net]
        n_out = [l for l in eng.layers if l["net"] == net][-1]["n_out"]
        for rows in (3, 33, 256):
            x1, x2 = rand(rows, n_in, seed=1), rand(rows, n_in, seed=2)
            d1, d2 = rand(rows, n_out, seed=3), rand(rows, n_out, seed=4)
            g1 = torch.empty(cnt, device=DEV)
            g2 = torch.empty(cnt, device=DEV)
            eng.net_backward(net, x1.to(DEV), d1.to(DEV), False, g1)
            eng.net_backward(net, x2.to(DEV), d2.to(DEV), False, g2)
            acc = torch.zeros(cnt, device=DEV)
            eng.net_backward(net, x1.to(DEV), d1.to(DEV), False, acc, accumulate=True)
            eng.net_backward(net, x2.to(DEV), d2.to(DEV), False, acc, accumulate=True)
            assert torch.equal(acc, g1 + g2), (net, rows)
            assert float(g1.abs().sum()) > 0


def test_stale_nan_in_the_workspace_never_reaches_a_gradient():
    """Workspace filled with NaN (what earlier calls may leave in pad rows and columns), then backward at 1, 3 and 33 rows:
    finite gradients, equal to the RefModel's."""
    for act in ("relu", "tanh"):
        arch = tiny(act=act)
        m, ref = build(arch, max_batch=64)
        for rows in (1, 3, 33):
            m.engine.workspace.fill_(float("nan"))
            for net_name in ("_task_encoder", "_motor_decoder", "_world_model"):
                stack_check(m, ref, net_name, rows, seed=rows)
                for p in getattr(m, net_name).parameters():
                    assert bool(torch.isfinite(p.grad).all())


def ppo_loss(logits, value, act, adv, ret, old_logp, Da):
    mean, log_std = logits[:, :Da], logits[:, Da:]
    logp = (-0.5 * (((act - mean) / torch.exp(log_std)) ** 2).sum(1) - log_std.sum(1) - 0.5 * Da * math.log(2 * math.pi))
    ratio = torch.exp(logp - old_logp)
    surr = torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv)
    return -surr.mean() + 0.5 * ((value - ret) ** 2).mean()


@pytest.mark.parametrize("frozen_md", [False, True])
def test_ppo_shaped_updates_at_the_runtime_spec_shapes(frozen_md):
    """Five PPO-shaped updates (clipped-ratio Gaussian log-likelihood + value loss, torch.optim.Adam over
    model.parameters()) of 500 rows at the runtime spec's shapes (Db 361, Da 54, Z 32, TE 256x2, MD 512x3, WM 1024x2)
    against the same updates on the RefModel: the loss after every step, the parameters at the end.  With the decoder
    frozen its weights stay bit-unchanged and get no .grad, while the encoder still trains."""
    arch = R.make_arch(361, 54, latent=32, te=(256, 2), md=(512, 3), wm=(1024, 2))
    m, ref = build(arch)
    Db, Da, Z, rows = 361, 54, 32, 500
    if frozen_md:
        m.set_learnable_motor_decoder(False)
        ref.set_learnable("_motor_decoder", False)
    md_before = {k: v.clone() for k, v in m._motor_decoder.state_dict().items()}
    obs, eps = rand(rows, 2 * Db, seed=1), rand(rows, Z, seed=2)
    act, adv, ret = rand(rows, Da, seed=3, scale=0.1), rand(rows, seed=4), rand(rows, seed=5)
    ref.eps_source = lambda shape: eps
    with torch.no_grad():
        want = ref(obs)
        old_logp = (-0.5 * (((act - want[:, :Da]) / 0.1) ** 2).sum(1)).detach() + 0.01 * rand(rows, seed=6)
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-4)
    ropt = torch.optim.Adam([p for p in ref.parameters() if p.requires_grad], lr=1e-4)
    d = {k: t.to(DEV) for k, t in (("obs", obs), ("eps", eps), ("act", act), ("adv", adv), ("ret", ret), ("old", old_logp))}
    for step in range(5):
        opt.zero_grad(set_to_none=True)
        logits, _ = m.forward({"obs_flat": d["obs"]}, [], None, eps=d["eps"])
        loss = ppo_loss(logits, m.value_function(), d["act"], d["adv"], d["ret"], d["old"], Da)
        loss.backward()
        opt.step()
        ropt.zero_grad(set_to_none=True)
        want = ref(obs)
        rloss = ppo_loss(want, ref.cur_value, act, adv, ret, old_logp, Da)
        rloss.backward()
        ropt.step()
        assert float(loss) == pytest.approx(float(rloss), rel=2e-4), step
        if frozen_md:
            assert all(p.grad is None for p in m._motor_decoder.parameters())
    mine = dict(m.named_parameters())
    for k, q in ref.named_parameters():
        if k.startswith(("_task_encoder", "_motor_decoder", "_value_branch")):
            assert max_err_scaled(mine[k].detach().cpu(), q.detach()) < 2e-3, k
    if frozen_md:
        for k, v in m._motor_decoder.state_dict().items():
            assert torch.equal(v, md_before[k]), k
    else:
        assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in m._motor_decoder.parameters())


def test_guards_values_inplace_writes_profiler():
    """A graph-building forward() gives the no-grad forward's bits; an optimizer step between forward and backward raises;
    the arena stacks run no aten::mm / addmm in either direction, and the backward launches are the library's."""
    arch = tiny()
    m, _ = build(arch, max_batch=64)
    Db, Da, Z = arch["Db"], arch["Da"], arch["Z"]
    for rows in (1, 4, 40):
        obs, eps = rand(rows, 2 * Db, seed=rows).to(DEV), rand(rows, Z, seed=9).to(DEV)
        with torch.no_grad():
            want, _ = m.forward({"obs_flat": obs}, [], None, eps=eps)
            wz, wmu = m.task_encoder_variable().clone(), m._cur_task_encoder_mu.clone()
            ws2 = m._cur_future_state.clone()
        got, _ = m.forward({"obs_flat": obs}, [], None, eps=eps)
        assert got.requires_grad and torch.equal(got.detach(), want)
        assert torch.equal(m.task_encoder_variable().detach(), wz) and torch.equal(m._cur_task_encoder_mu.detach(), wmu)
        assert torch.equal(m._cur_future_state.detach(), ws2)
    # an optimizer step between forward and backward
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    logits, _ = m.forward({"obs_flat": obs}, [], None, eps=eps)
    (logits[:, :Da] ** 2).sum().backward()
    opt.step()
    logits, _ = m.forward({"obs_flat": obs}, [], None, eps=eps)
    opt.step()
    with pytest.raises(RuntimeError, match="inplace"):
        (logits[:, :Da] ** 2).sum().backward()
    z_body, z_task, _ = m.forward_encoder(obs, eps=eps)
    dec, _ = m.forward_decoder(z_body, z_task)
    opt.step()
    with pytest.raises(RuntimeError, match="inplace"):
        (dec[:, :Da] ** 2).sum().backward()
    # no torch GEMM on the arena stacks; the library's backward launches are counted
    lib = m.engine.lib
    lib.pvae_profile_enable(1)
    try:
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            logits, _ = m.forward({"obs_flat": obs}, [], None, eps=eps)
            loss = (logits[:, :Da] ** 2).sum()
            z_body, z_task, _ = m.forward_encoder(obs, eps=eps)
            dec, _ = m.forward_decoder(z_body, z_task)
            s2 = m.forward_world(obs, dec)
            (loss + (dec[:, :Da] ** 2).sum() + (s2 ** 2).sum()).backward()
            torch.cuda.synchronize()
        launches = 0
        import ctypes as C
        for cat in (1, 2, 3):
            ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
            _lib.check(lib.pvae_profile_read(cat, C.byref(ms), C.byref(n), C.byref(fl)))
            launches += n.value
    finally:
        lib.pvae_profile_enable(0)
    names = {e.key for e in prof.key_averages()}
    assert not names & {"aten::mm", "aten::addmm", "aten::linear", "aten::matmul"}, names
    assert launches >= 5 * 3, launches              # (five stack backwards -- TE, MD twice, WM -- of three layers each)


def test_graph_building_forward_frees_its_outputs_and_guards_its_inputs():
    """The Functions keep no output of their own on ctx (a cycle through the graph that gc cannot break): five graph-building
    forwards + backwards leave none of their logits / codes alive once the module moves on.  Inputs are saved tensors: an
    observation (or stack input) written in place before the backward raises; value_function() reads its own copy of the
    observation; rollout_predicts_state = False keeps the prediction off under autograd too; an input of the wrong width is
    refused before anything is launched."""
    import gc
    import weakref
    arch = tiny()
    m, _ = build(arch, max_batch=64)
    Db, Da = arch["Db"], arch["Da"]
    obs = rand(5, 2 * Db, seed=3).to(DEV)
    refs = []
    for _ in range(5):
        logits, _ = m.forward({"obs_flat": obs}, [], None)
        z = m.task_encoder_variable()
        (logits[:, :Da] ** 2).sum().backward()
        refs += [weakref.ref(logits), weakref.ref(z)]
        del logits, z
    with torch.no_grad():
        m.forward({"obs_flat": obs}, [], None)              # the module's `_cur_*` state moves on
    gc.collect()
    assert sum(r() is not None for r in refs) == 0
    # in-place writes to saved inputs
    buf = obs.clone()
    logits, _ = m.forward({"obs_flat": buf}, [], None)
    buf.add_(1.0)
    with pytest.raises(RuntimeError, match="inplace"):
        (logits[:, :Da] ** 2).sum().backward()
    xg = rand(5, 2 * Db, seed=4).to(DEV).requires_grad_(True)
    out = AG.HipNet.apply(m.engine, _lib.NET_TE, xg, *m._stack_params(_lib.NET_TE))
    with torch.no_grad():
        xg.add_(1.0)
    with pytest.raises(RuntimeError, match="inplace"):
        out.sum().backward()
    # value_function after the caller recycled its buffer: the value of the rows the forward saw
    buf = obs.clone()
    m.forward({"obs_flat": buf}, [], None)
    buf.normal_()
    want = m._value_branch(obs).squeeze(1)
    assert torch.equal(m.value_function().detach(), want.detach())
    # the prediction follows rollout_predicts_state under autograd as well
    m.rollout_predicts_state = False
    try:
        logits, _ = m.forward({"obs_flat": obs}, [], None)
        assert m._cur_future_state is None and logits.requires_grad
        (logits[:, :Da] ** 2).sum().backward()
    finally:
        m.rollout_predicts_state = "lazy"
    with pytest.raises(AssertionError, match="full input width"):
        m.engine.net_backward(_lib.NET_TE, obs[:, :Db], torch.zeros(5, m.engine.layers[0]["n_out"]), True)
    with pytest.raises(AssertionError, match="full input width"):
        m.engine.net_forward(_lib.NET_TE, obs[:, :Db])
