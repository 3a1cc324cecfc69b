"""FullyConnectedPolicy ("fcnn", rmt:323-457) on the grouped stack kernels (include/pvae.h pvae_fc_*;
physicsvae_amd/fcnn.py, autograd.HipStackSet): logits, value and every gradient against the reference's capture
(tests/golden/fcnn_tiny.npz) and against a plain torch twin at the runtime shapes, the grouped schedule against the
stack-by-stack one bit for bit, launch counts, frozen stacks, chunked accumulation, stale workspaces, autograd guards,
weight files and five PPO-shaped updates.  Bounds are the suite's standing ones: outputs 1e-5, gradients 1e-4
(max_err_scaled), as tests/test_gpu_parity.py and tests/test_gpu_autograd.py."""
import gc
import json
import math
import weakref

import numpy as np
import pytest
import torch
import torch.nn as nn

from physicsvae_amd import FullyConnectedPolicy
from physicsvae_amd import autograd as AG
from physicsvae_amd.engine import Stack, StackSetEngine, set_fc_per_stack
from physicsvae_amd.spaces import Box
from util import max_err_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda"
VARIANTS = ("constant", "state_independent", "state_dependent")
ACTS = {"relu": nn.ReLU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid, "elu": nn.ELU}


def policy(cmc, obs=22, num_outputs=10, max_batch=512):
    cmc = dict(cmc, device=DEV, max_batch=max_batch)
    return FullyConnectedPolicy(Box(np.zeros(obs), np.zeros(obs)), Box(np.zeros(num_outputs // 2), np.zeros(num_outputs // 2)),
                                num_outputs, {"custom_model_config": cmc}, "fcnn")


def rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def captured_state_dict(g, name):
    flat, sd, o = torch.from_numpy(g[name + "/sd"]), {}, 0
    for k, shape in json.loads(str(g[name + "/keys"])):
        n = int(np.prod(shape))
        sd[k] = flat[o: o + n].reshape(shape).clone()
        o += n
    return sd


def unflatten(flat, m):
    out, o = {}, 0
    for k, p in m.named_parameters():
        out[k] = torch.from_numpy(flat[o: o + p.numel()]).reshape(p.shape)
        o += p.numel()
    assert o == flat.size
    return out


class Twin(nn.Module):
    """FullyConnectedPolicy.forward (rmt:430-441) on plain nn.Linear stacks, holding a HIP policy's weights (CPU)."""

    def __init__(self, m, cmc):
        super().__init__()
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

        def stack(prefix, layers):
            mods, i = [], 0
            for i, l in enumerate(layers):
                w = sd["%s._model.%d._model.0.weight" % (prefix, i)]
                lin = nn.Linear(w.shape[1], w.shape[0])
                with torch.no_grad():
                    lin.weight.copy_(w)
                    lin.bias.copy_(sd["%s._model.%d._model.0.bias" % (prefix, i)])
                mods.append(lin)
                if l["activation"] not in ("linear", None):
                    mods.append(ACTS[l["activation"]]())
            return nn.Sequential(*mods)
        cfg = dict(FullyConnectedPolicy.DEFAULT_CONFIG)
        cfg.update(cmc)
        self.pol = stack("_policy_fn", cfg["policy_fn_layers"])
        self.val = stack("_value_fn", cfg["value_fn_layers"])
        self.kind = cfg["log_std_type"]
        n = self.pol[-1].out_features if isinstance(self.pol[-1], nn.Linear) else None
        if self.kind == "state_dependent":
            self.ls = stack("_log_std_fn", cfg["log_std_fn_layers"])
            self.base = float(np.log(cfg["sample_std"]))
        else:
            ls = torch.as_tensor(np.log(np.asarray(cfg["sample_std"], dtype=np.float64)) * np.ones(n), dtype=torch.float32)
            self.log_std = nn.Parameter(ls) if self.kind == "state_independent" else ls

    def forward(self, obs):
        mean = self.pol(obs)
        self.cur_value = self.val(obs).squeeze(1)
        if self.kind == "state_dependent":
            return torch.cat([mean, self.base + self.ls(obs)], dim=-1)
        return torch.cat([mean, self.log_std.reshape(1, -1).expand(obs.shape[0], -1)], dim=-1)

    def named_like(self, m):
        """This twin's parameters under the HIP policy's names."""
        out = {}
        for prefix, seq in (("_policy_fn", self.pol), ("_value_fn", self.val), ("_log_std_fn", getattr(self, "ls", None))):
            if seq is None:
                continue
            lins = [x for x in seq if isinstance(x, nn.Linear)]
            for i, lin in enumerate(lins):
                out["%s._model.%d._model.0.weight" % (prefix, i)] = lin.weight
                out["%s._model.%d._model.0.bias" % (prefix, i)] = lin.bias
            if prefix == "_policy_fn" and self.kind == "state_independent":
                out["_policy_fn._model.%d.log_std" % len(lins)] = self.log_std
        return out


def run(m, x, c1, c2):
    """forward + backward of (logits * c1).sum() + (value * c2).sum(): (logits, value, dx, {name: grad})."""
    for p in m.parameters():
        p.grad = None
    xg = x.clone().requires_grad_(True)
    logits, _ = m.forward({"obs_flat": xg}, [], None)
    value = m.value_function()
    ((logits * c1).sum() + (value * c2).sum()).backward()
    return logits.detach(), value.detach(), xg.grad, {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}


@pytest.fixture(autouse=True)
def grouped_by_default():
    set_fc_per_stack(False)
    yield
    set_fc_per_stack(False)


@pytest.mark.parametrize("name", VARIANTS)
def test_logits_value_and_gradients_match_the_reference_capture(golden, name):
    g = golden("fcnn_tiny")
    m = policy(json.loads(str(g[name + "/spec"])))
    m.load_state_dict(captured_state_dict(g, name), strict=True)
    for rows in (7, 40):
        tag = "%s/r%d/" % (name, rows)
        x, c1, c2 = (torch.from_numpy(g[tag + k]).to(DEV) for k in ("x", "c1", "c2"))
        with torch.no_grad():
            plain, _ = m.forward({"obs_flat": x}, [], None)
            plain_v = m.value_function().clone()
        logits, value, dx, grads = run(m, x, c1, c2)
        assert torch.equal(logits, plain) and torch.equal(value, plain_v)       # the graph-building forward is the same call
        e_l, e_v = max_err_scaled(logits.cpu(), g[tag + "logits"]), max_err_scaled(value.cpu(), g[tag + "value"])
        e_x = max_err_scaled(dx.cpu(), g[tag + "gx"])
        print(name, rows, "logits %.3g value %.3g dx %.3g" % (e_l, e_v, e_x))
        assert logits.shape == (rows, 10) and value.shape == (rows,)
        assert e_l < 1e-5 and e_v < 1e-5 and e_x < 1e-4
        want = unflatten(g[tag + "g"], m)
        for k, w in want.items():
            e = max_err_scaled(grads[k].cpu(), w)
            assert e < 1e-4, (name, rows, k, e)


RUNTIME_ROWS = (1, 2, 4, 5, 33, 250, 256, 500, 1024)
_RUNTIME = {}


def runtime_pair(kind):
    """The runtime-shaped policy (obs 722, num_outputs 108, default 256x2 / 64x2 stacks, max_batch 512) and its twin."""
    if kind not in _RUNTIME:
        torch.manual_seed(11)
        cmc = {"log_std_type": kind, "sample_std": 0.6}
        m = policy(cmc, obs=722, num_outputs=108)
        with torch.no_grad():                    # biases off zero; output layers at a visible scale
            for k, p in m.named_parameters():
                if k.endswith("bias"):
                    p.copy_(0.1 * rand(*p.shape, seed=3).to(DEV))
                elif "._model.2." in k:
                    p.mul_(30.0)
        _RUNTIME[kind] = (m, Twin(m, cmc), cmc)
    return _RUNTIME[kind]


@pytest.mark.parametrize("kind", ["constant", "state_dependent"])
@pytest.mark.parametrize("rows", RUNTIME_ROWS)
def test_runtime_shapes_match_the_torch_twin(kind, rows):
    """GEMV path (<= 4 rows), tile path, and chunking (1024 rows at max_batch 512) against nn.Linear stacks."""
    m, twin, _ = runtime_pair(kind)
    x, c1, c2 = rand(rows, 722, seed=rows), rand(rows, 108, seed=rows + 1), rand(rows, seed=rows + 2)
    logits, value, dx, grads = run(m, x.to(DEV), c1.to(DEV), c2.to(DEV))
    for p in twin.parameters():
        p.grad = None
    xr = x.clone().requires_grad_(True)
    want = twin(xr)
    ((want * c1).sum() + (twin.cur_value * c2).sum()).backward()
    e_l, e_v = max_err_scaled(logits.cpu(), want.detach()), max_err_scaled(value.cpu(), twin.cur_value.detach())
    e_x = max_err_scaled(dx.cpu(), xr.grad)
    print(kind, rows, "logits %.3g value %.3g dx %.3g" % (e_l, e_v, e_x))
    assert e_l < 1e-5 and e_v < 1e-5 and e_x < 1e-4
    for k, q in twin.named_like(m).items():
        if q.grad is None:
            continue
        e = max_err_scaled(grads[k].cpu(), q.grad)
        assert e < 1e-4, (kind, rows, k, e)
    assert all(v is not None and bool(torch.isfinite(v).all()) for k, v in grads.items())


def stack_set(S, max_batch=512):
    specs = [(Stack((256, 256), ("relu", "tanh")), 54), (Stack((256, 256), "relu"), 1), (Stack((64, 64), ("elu", "relu")), 54),
             (Stack((128, 64), "sigmoid"), 7)][:S]
    eng = StackSetEngine(722, specs, max_batch, device=DEV)
    g = torch.Generator().manual_seed(5)
    for s in range(S):
        for w, b in eng.views(s):
            w.copy_((torch.randn(w.shape, generator=g) / math.sqrt(w.shape[1])).to(DEV))
            b.copy_((0.1 * torch.randn(b.shape, generator=g)).to(DEV))
    return eng


def test_grouped_equals_stack_by_stack_bit_for_bit():
    """Grouping changes which workgroup computes a tile, not the order of any tile's sum: outputs, the input gradient and
    every parameter gradient are the same bits under both schedules (store and accumulate), GEMV and tile paths."""
    eng = stack_set(4)
    for rows in (1, 3, 33, 256, 500):
        x = rand(rows, 722, seed=rows).to(DEV)
        dys = [rand(rows, n, seed=rows + 10 + s).to(DEV) for s, n in enumerate(eng.n_outs)]
        got = {}
        for per_stack in (False, True):
            set_fc_per_stack(per_stack)
            outs = eng.forward(x)
            g = torch.full((eng.arena_floats,), float("nan"), device=DEV)
            dx = eng.backward(x, dys, True, g, grad_mask=15)
            acc = torch.ones(eng.arena_floats, device=DEV)
            eng.backward(x, dys, False, acc, grad_mask=15, accumulate=True)
            got[per_stack] = (outs, dx, g, acc, eng.launches())
        a, b = got[False], got[True]
        assert all(torch.equal(p, q) for p, q in zip(a[0], b[0])), rows
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), rows
        assert bool(torch.isfinite(a[2]).all()) and float(a[2].abs().sum()) > 0
        assert torch.equal(a[3], a[2] + 1.0)                    # read-add-write of the same tile sums
        assert a[4][0] < b[4][0] and a[4][1] < b[4][1], (a[4], b[4])


def test_launch_counts_do_not_grow_with_the_number_of_stacks():
    """Equal-depth stacks: S = 3 and S = 4 launch exactly what S = 1 launches -- copy-in + one launch per layer depth
    forward; copy-in, the forward's launches, the seed, one launch per depth and the dx copy-out backward (+ one zeroing
    launch on the <= 4-row path).  Stack by stack the per-depth launches multiply."""
    counts = {}
    for S in (1, 3, 4):
        eng = stack_set(S)
        for rows in (2, 500):
            x = rand(rows, 722, seed=1).to(DEV)
            dys = [rand(rows, n, seed=2 + s).to(DEV) for s, n in enumerate(eng.n_outs)]
            eng.forward(x)
            eng.backward(x, dys, True, torch.empty(eng.arena_floats, device=DEV), grad_mask=(1 << S) - 1)
            counts[(S, rows)] = eng.launches()
    print(counts)
    assert counts[(1, 500)] == (1 + 3, 1 + 3 + 1 + 3 + 1)
    assert counts[(1, 2)] == (1 + 3, 1 + 1 + 3 + 1 + 3 + 1)
    for rows in (2, 500):
        assert counts[(3, rows)] == counts[(1, rows)] and counts[(4, rows)] == counts[(1, rows)]
    set_fc_per_stack(True)
    eng = stack_set(3)
    x = rand(500, 722, seed=1).to(DEV)
    eng.forward(x)
    assert eng.launches()[0] == 1 + 3 * 3
    # an output nobody wants costs no launch work of its own: forward of the value stack alone
    set_fc_per_stack(False)
    outs = eng.forward(x, want=[False, True, False])
    assert outs[0] is None and outs[2] is None and eng.launches()[0] == 4
    full = eng.forward(x)
    assert torch.equal(outs[1], full[1])


def test_frozen_value_stack_and_undifferentiated_outputs():
    m, twin, _ = runtime_pair("state_dependent")
    x, c1, c2 = rand(40, 722, seed=1).to(DEV), rand(40, 108, seed=2).to(DEV), rand(40, seed=3).to(DEV)
    _, _, dx_all, g_all = run(m, x, c1, c2)
    for p in m._value_fn.parameters():
        p.requires_grad_(False)
    try:
        _, _, dx_frozen, g_frozen = run(m, x, c1, c2)
        assert all(g_frozen[k] is None for k in g_frozen if k.startswith("_value_fn"))
        assert all(torch.equal(g_frozen[k], g_all[k]) for k in g_all if not k.startswith("_value_fn"))
        assert torch.equal(dx_frozen, dx_all)                    # the frozen stack still passes its input gradient
    finally:
        for p in m._value_fn.parameters():
            p.requires_grad_(True)
    # only the value is differentiated: the policy and log-std stacks get no gradient and no backward work
    for p in m.parameters():
        p.grad = None
    m.forward({"obs_flat": x}, [], None)
    (m.value_function() * c2).sum().backward()
    assert all((p.grad is None) == (not k.startswith("_value_fn")) for k, p in m.named_parameters())
    assert m.engine.launches()[1] == 1 + 3 + 1 + 3              # (no dx: the observation does not require grad)
    for k, p in m.named_parameters():
        if k.startswith("_value_fn"):
            assert torch.equal(p.grad, g_all[k]), k              # (the value stack's gradient depends on its own dy only)


def test_chunked_accumulation_is_the_explicit_two_call_accumulate_bit_for_bit():
    m, _, _ = runtime_pair("constant")
    eng = m.engine
    rows = 1024                                                   # two chunks of max_batch = 512
    x, c1, c2 = rand(rows, 722, seed=7).to(DEV), rand(rows, 108, seed=8).to(DEV), rand(rows, seed=9).to(DEV)
    _, _, dx, grads = run(m, x, c1, c2)
    g = torch.empty(eng.arena_floats, device=DEV)
    dys = [c1[:, :54].contiguous(), c2.reshape(rows, 1).contiguous()]
    dx0 = eng.backward(x[:512], [d[:512] for d in dys], True, g, grad_mask=3)
    dx1 = eng.backward(x[512:], [d[512:] for d in dys], True, g, grad_mask=3, accumulate=True)
    assert torch.equal(dx, torch.cat([dx0, dx1]))
    views = AG.stack_set_grad_views(eng, g)
    names = [k for k, _ in m.named_parameters()]
    assert len(views) == len(names)
    for k, v in zip(names, views):
        assert torch.equal(grads[k], v), k
    # ... and equals the sum of two stored calls
    g0, g1 = torch.empty_like(g), torch.empty_like(g)
    eng.backward(x[:512], [d[:512] for d in dys], False, g0, grad_mask=3)
    eng.backward(x[512:], [d[512:] for d in dys], False, g1, grad_mask=3)
    assert torch.equal(g, g0 + g1)


def test_stale_nan_in_the_workspace_reaches_nothing(golden):
    g = golden("fcnn_tiny")
    name = "state_dependent"
    m = policy(json.loads(str(g[name + "/spec"])), max_batch=64)
    m.load_state_dict(captured_state_dict(g, name), strict=True)
    tag = name + "/r40/"
    for rows in (1, 3, 7, 33, 40):
        x, c1, c2 = (torch.from_numpy(g[tag + k][:rows].copy()).to(DEV) for k in ("x", "c1", "c2"))
        m.engine.workspace.fill_(0.0)
        clean = run(m, x, c1, c2)
        m.engine.workspace.fill_(float("nan"))
        logits, value, dx, grads = run(m, x, c1, c2)
        assert torch.equal(logits, clean[0]) and torch.equal(value, clean[1]) and torch.equal(dx, clean[2])
        assert all(torch.equal(grads[k], clean[3][k]) for k in grads)
        assert all(bool(torch.isfinite(v).all()) for v in grads.values()) and bool(torch.isfinite(dx).all())
        if rows == 40:
            assert max_err_scaled(logits.cpu(), g[tag + "logits"]) < 1e-5
            assert max_err_scaled(dx.cpu(), g[tag + "gx"]) < 1e-4


def test_autograd_guards_and_freed_graphs():
    m, _, _ = runtime_pair("constant")
    x = rand(5, 722, seed=3).to(DEV)
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    logits, _ = m.forward({"obs_flat": x}, [], None)
    opt.zero_grad()
    (logits ** 2).sum().backward()
    opt.step()                                                    # (momentum-free, lr 0: still an in-place write)
    logits, _ = m.forward({"obs_flat": x}, [], None)
    opt.step()
    with pytest.raises(RuntimeError, match="inplace"):
        (logits ** 2).sum().backward()
    buf = x.clone()
    logits, _ = m.forward({"obs_flat": buf}, [], None)
    buf.add_(1.0)
    with pytest.raises(RuntimeError, match="inplace"):
        (logits ** 2).sum().backward()
    refs = []
    for _ in range(5):
        logits, _ = m.forward({"obs_flat": x}, [], None)
        value = m.value_function()
        ((logits ** 2).sum() + value.sum()).backward()
        refs += [weakref.ref(logits), weakref.ref(value)]
        del logits, value
    with torch.no_grad():
        m.forward({"obs_flat": x}, [], None)
    gc.collect()
    assert sum(r() is not None for r in refs) == 0
    with torch.no_grad():
        logits, _ = m.forward({"obs_flat": x}, [], None)
    assert not logits.requires_grad and m.engine.launches()[0] == 4
    with pytest.raises(AssertionError, match=r"\[rows, 722\]"):
        m.forward({"obs_flat": x[:, :700]}, [], None)


def test_set_exploration_std_and_call_surface():
    m, twin, _ = runtime_pair("constant")
    x = rand(3, 722, seed=4).to(DEV)
    try:
        m.set_exploration_std(0.25)
        with torch.no_grad():
            logits, state = m({"obs": x}, None, None)
        assert state == [] and logits.shape == (3, 108)
        assert torch.allclose(logits[:, 54:].cpu(), torch.full((3, 54), math.log(0.25)))
        assert max_err_scaled(logits[:, :54].cpu(), twin.pol(x.cpu()).detach()) < 1e-5
        assert max_err_scaled(m.value_function().cpu(), twin.val(x.cpu()).squeeze(1).detach()) < 1e-5
    finally:
        m.set_exploration_std(0.6)


def test_weight_files_round_trip_through_the_captured_state_dict(golden, tmp_path):
    g = golden("fcnn_tiny")
    for name in VARIANTS:
        sd = captured_state_dict(g, name)
        m = policy(json.loads(str(g[name + "/spec"])))
        f = str(tmp_path / (name + ".pt"))
        torch.save(sd, f)                                        # what the reference's torch.save(state_dict()) holds
        m.load_state_dict(torch.load(f), strict=True)
        x = torch.from_numpy(g[name + "/r7/x"]).to(DEV)
        with torch.no_grad():
            logits, _ = m.forward({"obs_flat": x}, [], None)
        assert max_err_scaled(logits.cpu(), g[name + "/r7/logits"]) < 1e-5
        pol = str(tmp_path / (name + "_policy.pt"))
        m.save_policy_weights(pol)
        got = torch.load(pol)
        want = {k[len("_policy_fn."):]: v for k, v in sd.items() if k.startswith("_policy_fn.")}
        assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
        m2 = policy(json.loads(str(g[name + "/spec"])))
        m2.load_policy_weights(pol)
        with torch.no_grad():
            l2, _ = m2.forward({"obs_flat": x}, [], None)
        assert torch.equal(l2[:, :5], logits[:, :5])
        back = str(tmp_path / (name + "_back.pt"))
        torch.save(m.state_dict(), back)
        full = torch.load(back)
        assert list(full) == list(sd) and all(torch.equal(full[k].cpu(), sd[k]) for k in sd)


def ppo_loss(logits, value, act, adv, ret, old_logp, Da):
    mean, log_std = logits[:, :Da], logits[:, Da:]
    logp = (-0.5 * (((act - mean) / torch.exp(log_std)) ** 2).sum(1) - log_std.sum(1) - 0.5 * Da * math.log(2 * math.pi))
    ratio = torch.exp(logp - old_logp)
    surr = torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv)
    return -surr.mean() + 0.5 * ((value - ret) ** 2).mean()


@pytest.mark.parametrize("kind", VARIANTS)
def test_ppo_shaped_updates_at_the_runtime_spec_shapes(kind):
    """Five PPO-shaped updates (clipped-ratio diagonal-Gaussian log-likelihood + value loss, torch.optim.Adam) of 500 rows
    on the HIP policy and on the torch twin from identical weights: the loss after every step (rel 2e-4) and the
    parameters at the end (2e-3), the pattern and bounds of tests/test_gpu_autograd.py's PPO test."""
    torch.manual_seed(21)
    cmc = {"log_std_type": kind, "sample_std": 0.1}
    m = policy(cmc, obs=722, num_outputs=108)
    twin = Twin(m, cmc)
    Da, rows = 54, 500
    obs = rand(rows, 722, seed=1)
    act, adv, ret = rand(rows, Da, seed=3, scale=0.1), rand(rows, seed=4), rand(rows, seed=5)
    with torch.no_grad():
        want = twin(obs)
        old_logp = (-0.5 * (((act - want[:, :Da]) / 0.1) ** 2).sum(1)).detach() + 0.01 * rand(rows, seed=6)
        old_logp = old_logp - want[:, Da:].sum(1) - 0.5 * Da * math.log(2 * math.pi)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    ropt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    d = {k: t.to(DEV) for k, t in (("obs", obs), ("act", act), ("adv", adv), ("ret", ret), ("old", old_logp))}
    for step in range(5):
        opt.zero_grad(set_to_none=True)
        logits, _ = m.forward({"obs_flat": d["obs"]}, [], None)
        loss = ppo_loss(logits, m.value_function(), d["act"], d["adv"], d["ret"], d["old"], Da)
        loss.backward()
        opt.step()
        ropt.zero_grad(set_to_none=True)
        want = twin(obs)
        rloss = ppo_loss(want, twin.cur_value, act, adv, ret, old_logp, Da)
        rloss.backward()
        ropt.step()
        print(kind, step, float(loss), float(rloss))
        assert float(loss) == pytest.approx(float(rloss), rel=2e-4), step
    mine = dict(m.named_parameters())
    names = twin.named_like(m)
    assert set(names) == set(mine)
    for k, q in names.items():
        assert max_err_scaled(mine[k].detach().cpu(), q.detach()) < 2e-3, k
    assert float(eng_pad_max(m)) == 0.0


def eng_pad_max(m):
    """Largest magnitude among the arena's pad entries (they must stay zero through optimizer steps)."""
    eng = m.engine
    live = torch.zeros_like(eng.params, dtype=torch.bool)
    for s in range(len(eng.stacks)):
        for w, b in eng.views(s, live):
            w.fill_(True)
            b.fill_(True)
    return eng.params[~live].abs().max()
