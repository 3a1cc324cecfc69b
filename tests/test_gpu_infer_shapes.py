"""Sweep of the rollout and autograd entry points of physicsvae_amd/csrc/pvae_infer.hip against float64, through `HipEngine`,
`PhysicsVAE` and physicsvae_amd/autograd.py: the 32 random and 10 directed models of tests/infer_cases.py -- stacks given layer
by layer, the four latent priors, the nine input-subset pairs, the helper, layers that read more than 1024 columns, Z = 130,
Db = Da = Z = 1 -- at 1 .. 131 rows.  tests/test_infer_cases_cpu.py checks without a GPU that the cases are what is claimed
here and that the float32 twin of each stays within a quarter of these bounds.

  rollout   `infer` under supplied draws, Philox draws (read back) and no noise, on the fused <= 4-row path and with the process
            option "rollout_fused" = 0 (the staged path); the bit-for-bit identities between `infer`, `infer_logits`,
            `infer_host` and `PhysicsVAE.forward`; guard bands around logits (row stride 2 Da + 7), s2_hat and z_out; the value
            branch; `mlp_forward` on strided operands.
  autograd  `HipNet` per stack, `net_backward` into a guarded segment (pads, accumulate), `HipReparam`, the graph-building
            `forward` (HipPolicy, or stage by stage past max_batch and under a learned prior), chunked batches against an
            engine that holds them whole.
  server    the rollout server on six cases against `infer`, bit for bit.

Bounds (infer_cases.py): rollout values 2e-5, the value 1e-4, autograd forward values 1e-5, every gradient 1e-4, all by
max_err_scaled against the float64 twin.  Gradients are taken on rows that keep ppo_cases.KINK from every ReLU kink: the pools
are filtered on the CPU; under Philox draws, which only the GPU knows, the rows at a kink leave the loss through a 0 / 1 weight.

The rollout server refuses one prior by design -- pvae_rollout_server.hip server_plan:
    if (c->L.cfg.prior_kind == PVAE_PRIOR_HYPERSPHERE)
        return fail(-24, "rollout server: this latent prior is served by the per-layer launches only");
-- so SERVER_CASES holds none; every other -24 on these small models is a failure."""
import numpy as np
import pytest
import torch

import infer_cases as I
from physicsvae_amd import _lib
from physicsvae_amd import autograd as AG
from ppo_cases import KINK
from test_gpu_rollout_server import served
from util import max_err_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
NET_ID = {"te": _lib.NET_TE, "md": _lib.NET_MD, "mh": _lib.NET_MH, "wm": _lib.NET_WM, "pr": _lib.NET_PR}
NORMAL = (I.ZERO_MEAN, I.STATE_MEAN)
_MODELS = {}


def model(name):
    """One module per case, shared by the tests of this file."""
    if name not in _MODELS:
        _MODELS[name] = I.module_for(I.case(name), DEV)
    return _MODELS[name]


def nan_buffer(shape, guard=64):
    """(flat NaN buffer, view of `shape` in it behind `guard` floats, with `guard` more behind it)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), NAN, dtype=torch.float32, device=DEV)
    return buf, buf[guard: guard + n].view(shape)


def only_these_are_written(buf, view, written):
    """Every float of `view` under the bool mask `written` is finite and every other float of `buf` is still NaN."""
    off = (view.data_ptr() - buf.data_ptr()) // 4
    want = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    want[off: off + view.numel()] = written.reshape(-1).to(buf.device)
    return bool((torch.isfinite(buf) == want).all()) and bool((torch.isnan(buf) == ~want).all())


def twin_forward(c, rows, eps, noise):
    with torch.no_grad():
        return I.forward(c, I.leaves(c, torch.float64), c.obs[:rows].double(), None if eps is None else eps.double(), noise)


def used_draws(c, eng, rows, mode):
    """The standard normals the last rollout / sampler call used, as the twin needs them (None where it uses none)."""
    if mode == "off" or c.prior not in NORMAL:
        return None
    return eng.read("eps", rows).cpu() if mode == "philox" else c.eps[:rows]


class Worst(dict):
    def up(self, key, v):
        self[key] = max(self.get(key, 0.0), float(v))
        return v


# ---------------------------------------------------------------------------------------
# rollout
# ---------------------------------------------------------------------------------------
def guarded_infer_logits(c, eng, obs, ls, want_s2, eps, noise, seed, offset):
    """pvae_infer_logits through the C ABI with every output in a NaN-filled buffer one row longer than the call, logits at a
    row stride of 2 Da + 7: (logits [rows, 2 Da], s2 | None, z), after checking that nothing else was written."""
    rows, ld = obs.shape[0], 2 * c.Da + 7
    assert obs.shape == (rows, 2 * c.Db) and obs.is_contiguous() and rows <= eng.max_batch and ls.shape == (c.Da,)
    assert eps is None or (eps.shape == (rows, c.Z) and eps.is_contiguous())
    lbuf, logits = nan_buffer((rows + 1, ld))
    sbuf, s2 = nan_buffer((rows + 1, c.Db))
    zbuf, z = nan_buffer((rows + 1, c.Z))
    _lib.check(eng.lib.pvae_infer_logits(eng.ctx, obs.data_ptr(), rows, eps.data_ptr() if eps is not None else None, 1 if noise else 0,
                                         seed, offset, logits.data_ptr(), ld, ls.data_ptr(), s2.data_ptr() if want_s2 else None,
                                         z.data_ptr(), eng._stream()), "pvae_infer_logits")
    torch.cuda.synchronize()
    mask = lambda width, used: (torch.arange(rows + 1)[:, None] < rows) & (torch.arange(width)[None, :] < used)     # noqa: E731
    assert only_these_are_written(lbuf, logits, mask(ld, 2 * c.Da)), "logits"
    assert only_these_are_written(sbuf, s2, mask(c.Db, c.Db if want_s2 else 0)), "s2_hat"
    assert only_these_are_written(zbuf, z, mask(c.Z, c.Z)), "z_out"
    return logits[:rows, :2 * c.Da].clone(), s2[:rows].clone() if want_s2 else None, z[:rows].clone()


def rollout_pass(c, m, fused, worst):
    eng = m.engine
    ls = m._als.on_device(eng.device).detach()
    assert torch.equal(ls.cpu(), c.ls_vec)
    for rows in I.rollout_rows(c):
        obs = c.obs[:rows].to(DEV)
        for mode in I.NOISE_MODES:
            noise, eps = mode != "off", c.eps[:rows].to(DEV) if mode == "eps" else None
            draws = dict(eps=eps, noise=noise, seed=5, offset=40 + rows)
            a, s2, z = eng.infer(obs, **draws)
            want = twin_forward(c, rows, used_draws(c, eng, rows, mode), noise)
            e = {"a_hat": max_err_scaled(a.cpu(), want.a), "s2_hat": max_err_scaled(s2.cpu(), want.s2), "z": max_err_scaled(z.cpu(), want.z)}
            for key, v in e.items():
                worst.up(key, v)
                assert v < I.ROLLOUT_BOUND, (c.name, "fused" if fused else "staged", rows, mode, key, v)
            # identities, bit for bit
            a2, none, z2 = eng.infer(obs, want_s2=False, **draws)
            assert none is None and torch.equal(a2, a) and torch.equal(z2, z), (c.name, rows, mode, "want_s2=False")
            lg, s2l, zl = eng.infer_logits(obs, ls, **draws)
            assert torch.equal(lg[:, :c.Da], a) and torch.equal(lg[:, c.Da:], ls.reshape(1, -1).expand(rows, -1)), (c.name, rows, mode)
            assert torch.equal(s2l, s2) and torch.equal(zl, z), (c.name, rows, mode, "infer_logits")
            for want_s2 in (True, False):                            # (False: the decoder's last launch writes the caller's rows)
                glg, gs2, gz = guarded_infer_logits(c, eng, obs, ls, want_s2, eps, noise, 5, 40 + rows)
                assert torch.equal(glg, lg) and torch.equal(gz, z) and (gs2 is None or torch.equal(gs2, s2)), (c.name, rows, mode, want_s2)
            if fused and eng.fused_rollout and rows in (1, 2, 4) and mode != "eps":
                host = eng.infer_host(c.obs[:rows], noise=noise, seed=5, offset=40 + rows)
                assert torch.equal(host, a.cpu()), (c.name, rows, mode, "infer_host")
            # the module's forward without a graph is that call (stage by stage under a learned prior: held to the twin)
            m.latent_prior_noise = noise
            m.seed(5)
            with torch.no_grad():
                mlg, _ = m.forward({"obs_flat": obs}, [], None, eps=eps)
                value = m.value_function()
            if c.prior == I.STATE_MEAN:
                used = used_draws(c, eng, rows, mode)
                mwant = twin_forward(c, rows, used, noise)
                assert worst.up("a_hat", max_err_scaled(mlg[:, :c.Da].cpu(), mwant.a)) < I.ROLLOUT_BOUND, (c.name, rows, mode)
                assert torch.equal(mlg[:, c.Da:], lg[:, c.Da:])
            else:
                assert torch.equal(mlg, eng.infer_logits(obs, ls, eps=eps, noise=noise, seed=5, offset=1)[0]), (c.name, rows, mode, "forward")
            assert worst.up("value", max_err_scaled(value.cpu(), want.value)) < I.VALUE_BOUND, (c.name, rows)
    m.latent_prior_noise = c.noise != "off"


@pytest.mark.parametrize("name", I.CASE_IDS)
def test_rollout_matches_the_float64_twin_on_both_paths(name):
    c, m = I.case(name), model(name)
    lib = _lib.load()
    fused, staged = Worst(), Worst()
    rollout_pass(c, m, True, fused)
    _lib.check(lib.pvae_set_option(None, b"rollout_fused", 0), "rollout_fused")
    try:
        assert not lib.pvae_rollout_is_fused()
        rollout_pass(c, m, False, staged)
    finally:
        _lib.check(lib.pvae_set_option(None, b"rollout_fused", 1), "rollout_fused")
    print(name, "Db %d Da %d Z %d" % (c.Db, c.Da, c.Z), c.prior, c.te_inputs, c.md_inputs, "helper" if c.mh else "",
          "fused", {k: "%.3g" % v for k, v in fused.items()}, "staged", {k: "%.3g" % v for k, v in staged.items()},
          "bounds %.3g / value %.3g" % (I.ROLLOUT_BOUND, I.VALUE_BOUND))


@pytest.mark.parametrize("name", I.CASE_IDS)
def test_mlp_forward_on_strided_operands(name):
    """`eng.mlp_forward` with 1-4 layers of the case's widths, weights that are column blocks of wider tensors, an input that is
    one, an activation per hidden layer and a linear or tanh output, against float64."""
    c, eng = I.case(name), model(name).engine
    g = torch.Generator().manual_seed(c.seed + 77)
    widths = (c.te[0] + c.md[0] + c.wm[0] + (5, 17, 31))[:3]
    n_in, worst = c.Db + 3, 0.0
    for n in (1, 2, 3, 4):
        dims = (n_in,) + widths[:n - 1] + (c.Da,)
        acts = [I.ACT_NAMES[(n + i + c.seed) % 5] for i in range(n - 1)]
        layers = []
        for i in range(n):
            wide = torch.randn(dims[i + 1], dims[i] + 5, generator=g) / np.sqrt(dims[i])
            layers.append((wide.to(DEV)[:, :dims[i]], (0.1 * torch.randn(dims[i + 1], generator=g)).to(DEV)))
        assert all(w.stride(0) == w.shape[1] + 5 for w, _ in layers)
        for rows in (1, 3, 4, 5, 33):
            xw = torch.randn(rows, n_in + 2, generator=g).to(DEV)
            x = xw[:, :n_in]
            for out_act in (None, "tanh"):
                got = eng.mlp_forward(x, layers, act=acts, out_act=out_act)
                h = x.cpu().double()
                for i, (w, b) in enumerate(layers):
                    h = h @ w.cpu().double().T + b.cpu().double()
                    if i < n - 1:
                        h = F_apply(acts[i], h)
                want = torch.tanh(h) if out_act else h
                e = max_err_scaled(got.cpu(), want)
                worst = max(worst, e)
                assert got.shape == (rows, c.Da) and e < I.ROLLOUT_BOUND, (name, n, rows, acts, out_act, e)
    print(name, "mlp_forward %.3g  bound %.3g" % (worst, I.ROLLOUT_BOUND))


def F_apply(name, t):
    return {"relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "elu": torch.nn.functional.elu, "linear": lambda v: v}[name](t)


# ---------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------
def zero_grads(m):
    for p in m.parameters():
        p.grad = None


def check_param_grads(c, m, key, want, worst, where):
    params = m._stack_params(NET_ID[key])
    assert len(params) == 2 * len(want)
    for i, pair in enumerate(want):
        for j, g in enumerate(pair):
            p = params[2 * i + j]
            if g is None or I.structurally_zero(c, key) and where[0] == "policy":      # no path to the loss: None, or exact zeros
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, (c.name, key, i, j) + where
                continue
            assert p.grad is not None, (c.name, key, i, j) + where
            e = worst.up("gradients", max_err_scaled(p.grad.cpu(), g))
            assert e < I.GRAD_BOUND, (c.name, key, i, j, e) + where


def stack_check(c, m, key, rows, worst):
    """`HipNet` on stack `key`: the output, dx inside the stack's window (exactly zero outside it) and every parameter gradient."""
    eng, net = m.engine, NET_ID[key]
    x, dy = I.twin(c.name, rows).x[key], c.dy[key][:rows]
    assert x.shape[1] == eng.net_in_width(net) == I.in_width(c, key)
    zero_grads(m)
    xg = x.to(DEV).requires_grad_(True)
    out = AG.HipNet.apply(eng, net, xg, *m._stack_params(net))
    out.backward(dy.to(DEV))
    want = I.stack_twin(c, key, x, dy)
    assert worst.up("forward", max_err_scaled(out.detach().cpu(), want.out)) < I.FORWARD_BOUND, (c.name, key, rows)
    lo, hi = I.window(c, key)
    dx = xg.grad.cpu()
    assert worst.up("dx", max_err_scaled(dx[:, lo:hi], want.dx)) < I.GRAD_BOUND, (c.name, key, rows)
    outside = torch.ones(x.shape[1], dtype=torch.bool)
    outside[lo:hi] = False
    assert not outside.any() or float(dx[:, outside].abs().max()) == 0.0, (c.name, key, rows)
    check_param_grads(c, m, key, want.grads, worst, ("stack", rows))
    assert all(bool(torch.isfinite(p.grad).all()) for p in m._stack_params(net))


@pytest.mark.parametrize("name", I.CASE_IDS)
def test_every_stack_under_autograd(name):
    """Largest batch first, so that the panels' pad rows are dirty; before the calls of at most 4 rows -- whose recomputed forward
    is the GEMV family, which writes the live rows only -- the whole workspace is NaN, as in
    test_stale_nan_in_the_workspace_never_reaches_a_gradient: whatever an earlier call left must reach no gradient."""
    c, m = I.case(name), model(name)
    worst = Worst()
    try:
        for rows in sorted(I.autograd_rows(c), reverse=True):
            if rows <= 4:
                m.engine.workspace.fill_(NAN)
            for key in I.nets_of(c):
                stack_check(c, m, key, rows, worst)
    finally:
        m.engine.workspace.zero_()
    print(name, {k: "%.3g" % v for k, v in worst.items()}, "bounds forward %.3g gradients %.3g" % (I.FORWARD_BOUND, I.GRAD_BOUND))


def pad_mask(eng, net):
    """bool [segment]: True at the pad entries of the stack's segment (first-layer columns outside an input subset included)."""
    marks = torch.zeros(eng.segments[net][1], dtype=torch.float32, device=DEV)
    for v in AG.grad_views(eng, net, marks):
        v.fill_(1.0)
    return marks == 0


@pytest.mark.parametrize("name", I.CASE_IDS)
def test_net_backward_writes_its_segment_and_nothing_else(name):
    """`pvae_net_backward` with dx and the gradient segment inside NaN buffers, 64 guard floats on each side (dx one row longer
    than the call): the guards stay NaN, every entry of the segment is written -- the weight-gradient tiles cover the padded
    blocks W[n_out_pad][ld] and the bias sums all n_out_pad columns -- and the pad entries hold exactly 0.0, the sums of padded
    operands that net_seed_kernel, pad_copy_kernel and the forward's n_valid zeroed; accumulate = 1 twice into zeros is, bit for
    bit, twice the stored gradient (every tile is summed by one workgroup in a fixed order), on both weight-gradient
    geometries."""
    c, m = I.case(name), model(name)
    eng = m.engine
    for rows in sorted({3, min(33, c.max_batch), min(64, c.max_batch), min(97, c.max_batch)}, reverse=True):
        tw = I.twin(name, rows)
        for key in I.nets_of(c):
            net = NET_ID[key]
            x, dy = tw.x[key].to(DEV).contiguous(), c.dy[key][:rows].to(DEV).contiguous()
            cnt, n_in = eng.segments[net][1], x.shape[1]
            # (the C ABI is called directly below: the shapes the engine's wrapper would check)
            assert x.shape == (rows, eng.net_in_width(net)) and dy.shape == (rows, I.out_width(c, key)) and rows <= eng.max_batch
            gbuf, seg = nan_buffer((cnt,))
            dbuf, dx = nan_buffer((rows + 1, n_in))
            _lib.check(eng.lib.pvae_net_backward(eng.ctx, net, x.data_ptr(), rows, dy.data_ptr(), dx.data_ptr(), seg.data_ptr(), 0,
                                                 eng._stream()), "pvae_net_backward")
            torch.cuda.synchronize()
            assert only_these_are_written(gbuf, seg, torch.ones(cnt, dtype=torch.bool)), (name, key, rows, "grad")
            assert only_these_are_written(dbuf, dx, torch.arange(rows + 1)[:, None].expand(-1, n_in) < rows), (name, key, rows, "dx")
            pads = pad_mask(eng, net)
            assert bool(pads.any()) and float(seg[pads].abs().max()) == 0.0, (name, key, rows, "pads")
            assert float(seg[~pads].abs().max()) > 0.0
            stored = seg.clone()
            assert torch.equal(eng.net_backward(net, x, dy, True, seg), dx[:rows]) and torch.equal(seg, stored)      # the engine's call: same bits
            abuf, acc = nan_buffer((cnt,))
            acc.zero_()
            for _ in range(2):
                eng.net_backward(net, x, dy, False, acc, accumulate=True)
            torch.cuda.synchronize()
            assert torch.equal(acc, stored + stored), (name, key, rows, "accumulate")
            assert only_these_are_written(abuf, acc, torch.ones(cnt, dtype=torch.bool))


@pytest.mark.parametrize("name", I.CASE_IDS)
def test_sampler_under_autograd(name):
    """`HipReparam` for the case's prior with the noise on (supplied draws; Philox draws read back on the Philox cases) and off:
    z and d_mu_logvar against the twin; with the noise off on the Normal kinds the logvar half is exactly 0.0."""
    c, eng = I.case(name), model(name).engine
    worst = Worst()
    for rows in [r for r in I.autograd_rows(c) if r <= c.max_batch]:
        h = I.twin(name, rows).h.float()
        dz = c.dz[:rows]
        for mode in ("eps", "off") + (("philox",) if c.noise == "philox" else ()):
            noise = mode != "off"
            hg = h.to(DEV).requires_grad_(True)
            z = AG.HipReparam.apply(eng, noise, 9, rows, c.eps[:rows].to(DEV) if mode == "eps" else None, hg)
            used = used_draws(c, eng, rows, mode)
            z.backward(dz.to(DEV))
            used = None if used is None else used.double()
            want_z = I.sampler(c, h.double(), used, noise)
            want_d = I.sampler_backward(c, h.double(), used, noise, dz.double())
            assert worst.up("z", max_err_scaled(z.detach().cpu(), want_z)) < I.FORWARD_BOUND, (name, rows, mode)
            assert worst.up("d_mu_logvar", max_err_scaled(hg.grad.cpu(), want_d)) < I.GRAD_BOUND, (name, rows, mode)
            if not noise and c.prior in NORMAL:
                assert float(hg.grad[:, c.Z:].abs().max()) == 0.0 and torch.equal(hg.grad[:, :c.Z].cpu(), dz)
    print(name, c.prior, "Z %d" % c.Z, {k: "%.3g" % v for k, v in worst.items()}, "bounds %.3g / %.3g" % (I.FORWARD_BOUND, I.GRAD_BOUND))


def policy_check(c, m, rows, mode, worst):
    """The module's graph-building forward on (logits[:, :Da]**2).sum() + (_cur_future_state**2).sum() [+ the prior mean's]."""
    eng = m.engine
    noise = mode != "off"
    philox = mode == "philox" and c.prior in NORMAL
    obs = c.obs[:rows].to(DEV)
    m.latent_prior_noise = noise
    m.seed(3)
    zero_grads(m)
    logits, _ = m.forward({"obs_flat": obs}, [], None, eps=c.eps[:rows].to(DEV) if mode == "eps" else None)
    assert logits.requires_grad and logits.shape == (rows, 2 * c.Da)
    used = eng.read("eps", rows).cpu() if philox else (c.eps[:rows] if noise else None)
    weight = None
    if philox:                                   # draws only the GPU knows: the rows they put at a ReLU kink leave the sum
        weight = (twin_forward(c, rows, used, noise).margin >= KINK).double()
        worst["philox rows dropped"] = worst.get("philox rows dropped", 0) + int(rows - weight.sum())
    w = torch.ones(rows, 1, device=DEV) if weight is None else weight.float().reshape(-1, 1).to(DEV)
    loss = (w * logits[:, :c.Da] ** 2).sum() + (w * m._cur_future_state ** 2).sum()
    if c.prior == I.STATE_MEAN:
        loss = loss + (w * m._cur_latent_prior_mu ** 2).sum()
    loss.backward()
    want = I.policy_twin(c, c.obs[:rows], used, noise, weight=weight)
    e = worst.up("loss", abs(float(loss) - float(want.loss)) / abs(float(want.loss)))
    assert e <= I.FORWARD_BOUND, (c.name, rows, mode, e)
    for key in I.nets_of(c):
        check_param_grads(c, m, key, want.grads[key], worst, ("policy", rows, mode))
    for p in list(m._value_branch.parameters()):
        assert p.grad is None


@pytest.mark.parametrize("name", I.CASE_IDS)
def test_graph_building_forward(name):
    """Every autograd row count: `HipPolicy` up to max_batch rows, stage by stage (HipNet in chunks, accumulate = 1 after the first)
    past it and under a learned prior.  The case's noise mode; Philox only where one call draws for all rows."""
    c, m = I.case(name), model(name)
    worst = Worst()
    for rows in I.autograd_rows(c):
        mode = c.noise if (c.noise != "philox" or rows <= c.max_batch) else "eps"
        policy_check(c, m, rows, mode, worst)
    m.latent_prior_noise = c.noise != "off"
    print(name, c.prior, c.noise, {k: "%.3g" % v for k, v in worst.items()}, "bounds loss %.3g gradients %.3g" % (I.FORWARD_BOUND, I.GRAD_BOUND))


@pytest.mark.parametrize("name", ["chunk64", "chunk32"])
def test_chunked_batches_equal_a_single_chunk(name):
    """loss.backward() through forward + forward_world at row counts past max_batch (chunks of 64 + 64 [+ 3] rows on 32x32
    weight-gradient tiles; of 32 rows and a last one of 1 row on 64x64 tiles) against the twin and against a second module of the
    same weights that holds the batch in one chunk."""
    c, m = I.case(name), model(name)
    m1 = I.module_for(c, DEV, max_batch=160)
    worst = Worst()
    for rows in c.extra_rows:
        obs, eps = c.obs[:rows].to(DEV), c.eps[:rows].to(DEV)
        grads = []
        for mod in (m, m1):
            zero_grads(mod)
            lg, _ = mod.forward({"obs_flat": obs}, [], None, eps=eps)
            s2 = mod.forward_world(obs, lg)
            ((lg[:, :c.Da] ** 2).sum() + (s2 ** 2).sum()).backward()
            grads.append({k: p.grad.clone() for k, p in mod.named_parameters() if p.grad is not None})
        want = I.policy_twin(c, c.obs[:rows], c.eps[:rows], True)
        for key in I.nets_of(c):
            check_param_grads(c, m, key, want.grads[key], worst, ("chunked", rows))
        assert grads[0].keys() == grads[1].keys() and len(grads[0]) == 2 * sum(len(getattr(c, k)[0]) + 1 for k in ("te", "md", "wm"))
        for k in grads[0]:
            assert worst.up("against one chunk", max_err_scaled(grads[0][k].cpu(), grads[1][k].cpu())) < I.GRAD_BOUND, (name, rows, k)
    print(name, {k: "%.3g" % v for k, v in worst.items()}, "bound %.3g" % I.GRAD_BOUND)


# ---------------------------------------------------------------------------------------
# the rollout server
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", I.SERVER_CASES)
def test_rollout_server_equals_infer_bit_for_bit(name):
    """One start per case, stopped in `finally`; rows 1-4 with the noise on and off, single-row requests through both calls."""
    c, eng = I.case(name), model(name).engine
    torch.cuda.synchronize()
    with served(eng, idle_ms=200.0, lifetime_s=30.0):
        assert eng.rollout_server_status()[0]
        for rows in (1, 2, 3, 4):
            obs = c.obs[:rows]
            for noise in (True, False):
                draws = dict(noise=noise, seed=11, offset=300 + rows)
                got = [tuple(t.copy() for t in eng.rollout_server_infer_rows(obs.numpy(), **draws))]
                if rows == 1:
                    a, ml, z = (t.copy() for t in eng.rollout_server_infer(obs[0].numpy(), **draws))
                    got.append((a[None], ml[None], z[None]))
                want_a, _, want_z = eng.infer(obs.to(DEV), want_s2=False, **draws)
                for a, _, z in got:
                    assert np.array_equal(a, want_a.cpu().numpy()), (name, rows, noise, "a_hat")
                    assert np.array_equal(z, want_z.cpu().numpy()), (name, rows, noise, "z")
    assert eng.rollout_server_status()[0] is False
