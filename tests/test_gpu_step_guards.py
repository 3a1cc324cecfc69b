"""The supervised training step inside guard bands (tests/guards.py).

The step's kernels run whole padded tiles without bounds checks over buffers the caller sizes with pvae_arena_floats and
pvae_workspace_bytes.  Here a bare HipEngine gets its four arenas and its workspace -- bound with EXACTLY
pvae_workspace_bytes, zero-filled, 256-byte aligned -- as views inside poisoned buffers (guard_engine), and every tensor a
call takes (x, y, eps, loss_out, the dataset arrays, the rollout outputs) is such a view too.  A store outside a buffer
changes the bits of a guard; a load outside it that reaches a result makes that result NaN.

Every case is built exactly as tests/test_gpu_shapes.py::_check builds it (same oracle calls, same kink filter, same
seeds) and runs on a guarded twin with max_batch == rows (Bp as tight as the layout allows) and on one with max_batch
130.  Per phase: set_batch + forward_backward with the gradient stored, evaluation, forward_seed + every backward_stage,
three fused steps, three flat-Adam steps (both also with weight_decay = 0.01), and at lookahead 1 gather, train_step and
train_step_prefetch over a guarded dataset -- minibatches with the first window, with the window that ends on the very
last dataset row, and a ragged last one.  Asserted: every guard intact after each entry point (the message names the
call); losses 1e-5 and gradients 1e-4 against the oracle; every tensor bit-equal to the unguarded trainer engine's; the
pad entries of params / exp_avg / exp_avg_sq (the arena minus the union of named_views) exactly zero after Adam."""
import pytest
import torch

import guards as G
import tile_rules as TR
from oracle import refpath as R
from physicsvae_amd import _lib
from physicsvae_amd.engine import HipEngine, make_step_params
from test_gpu_shapes import _case, _case_stacks
from util import make_trainer, max_err_scaled, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TERMS = ("loss_a", "loss_kl", "loss_s", "loss_cyc")
TWIN_ROWS = 130

# a dozen seeds of the sweep whose kink filter keeps (nearly) every row: rows 1, 2, 7, 31, 32, 33, 64, 97 and 130 all
# run, lookahead 1, 2 and 3, MSE and L1 (survivors of both phases checked on the CPU with R.relu_kink_margin)
PLAIN = [2, 5, 6, 9, 11, 17, 20, 26, 33]       # rows 1, 2, 7, 33, 32, 64, 31, 130, 97; L 1, 3, 2, 3, 1, 1, 1, 1, 1
STACKS = [3, 4, 10]                            # rows 32, 130, 31; L 2, 2, 3; L1 loss; per-layer widths and activations


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


class Case:
    """One architecture + minibatch + weights, the oracle's answers per phase (computed once, shared by every engine)."""

    def __init__(self, arch, data, x, y, sd, eps, L=1, loss="MSE", trainer=make_trainer, joint_cfg=None, margin=None,
                 extra=None, strict=True):
        self.arch, self.data, self.x, self.y, self.sd, self.eps, self.L, self.lk = arch, data, x, y, sd, eps, L, loss
        self.rows = x.shape[0]
        self.joint_cfg, self.margin, self.strict = joint_cfg, margin, strict
        self.extra = dict({"lookahead": L, "loss": loss}, **(extra or {}))
        self.trainer = trainer
        self._phase = {}
        self.tr = None

    def coeffs(self, world):
        return R.phase_coeffs(world, self.joint_cfg)

    def phase(self, world):
        """(xk, yk, e_in, n, want) off the ReLU kinks, as _check forms them."""
        if world not in self._phase:
            x, y, eps, L = self.x, self.y, self.eps, self.L
            if self.margin is not None and not world:
                m = self.margin(self.arch, self.sd, x, y, eps, self.coeffs(False))
            else:
                m = R.relu_kink_margin(self.arch, self.sd, x, y, eps, world)
            keep = m > 4e-6
            n = int(keep.sum())
            assert n >= max(1, self.rows - max(4, self.rows // 4)), "the kink filter drops more rows than its cap"
            xk, yk, ek = x[keep], y[keep], eps[:, keep]
            want = R.loss_and_grads(self.arch, self.sd, xk, yk, ek if L > 1 else ek[0], world,
                                    coeff_cfg=self.joint_cfg, loss=self.lk)
            e_in = (ek if L > 1 else ek[0]) if (not world or L > 1) else None
            self._phase[world] = (xk, yk, e_in, n, want)
        return self._phase[world]

    def reference(self):
        """The unguarded engine: the trainer's, built as _check builds it."""
        if self.tr is None:
            self.tr = self.trainer(self.arch, self.data, self.rows, device=DEV, extra=self.extra)
            self.tr.model.load_state_dict(self.sd)
        return self.tr.engine

    def twin(self, max_batch, **options):
        ref = self.reference()
        eng = HipEngine(ref.arch, max_batch, DEV, lookahead=self.L)
        G.guard_engine(eng, joint_s_rec=bool(self.joint_cfg and self.joint_cfg.get("s_rec_coeff")), **options)
        eng.params.copy_(ref.params)
        return eng

    def sp(self, world, rows, t=1, wd=0.0):
        c = self.coeffs(world)
        return make_step_params(lr=5e-4, adam_t=(t,) * _lib.NUM_NETS, a_rec=c["a_rec_coeff"], kl=c["vae_kl_coeff"],
                                s_rec=c["s_rec_coeff"], cyc=c["vae_cycle_coeff"], global_rows=rows, loss=self.lk, weight_decay=wd)


def _sweep_case(c, seed):
    L, rows, lk = c["L"], c["rows"], c["loss"]
    arch = R.make_arch(c["Db"], c["Da"], latent=c["Z"], te=c["te"], md=c["md"], wm=c["wm"])
    data = R.synth_demo(seed, 2, rows + L + 3, c["Db"], c["Da"], kind="dynamics")
    X, Y = R.build_windows(data, lookahead=L)
    x, y = next(iter(R.make_loader(X, Y, rows)))
    assert x.shape[0] == rows
    sd = R.perturb_biases(R.init_state_dict(arch, seed=seed + 1), seed=seed + 3)
    es = R.eps_stream(seed + 2, c["Z"])
    eps = torch.stack([es(t, (rows, c["Z"])) for t in range(L)])
    return Case(arch, data, x, y, sd, eps, L=L, loss=lk)


class Placer:
    """Tensors of one engine's calls: views inside guarded buffers for a guarded engine, plain device tensors else."""

    def __init__(self, eng):
        self.eng, self.on, self.extra = eng, hasattr(eng, "guards"), []

    def put(self, name, t, fill=True):
        t = t.to(DEV, torch.float32).contiguous()
        if not self.on:
            return t.clone()
        buf, view = G.guarded(t.shape, guard=64 * max(int(t.shape[-1]), 1), fill=None, device=DEV)
        if fill:
            view.copy_(t)
        self.extra.append((name, buf, view))
        return view

    def check(self, what):
        if self.on:
            G.check_engine_guards(self.eng, what, self.extra)


def _nets(eng, world):
    """The stacks a phase trains (arena order TE | MD | MH | PR | WM: adjacent)."""
    if world:
        return [_lib.NET_WM]
    return [n for n in (_lib.NET_TE, _lib.NET_MD, _lib.NET_MH, _lib.NET_PR) if eng.segments[n][1] > 0]


def _pads_zero(eng, pads, tag):
    for name, a in (("params", eng.params), ("exp_avg", eng.exp_avg), ("exp_avg_sq", eng.exp_avg_sq)):
        if bool(pads.any()):
            assert float(a[pads].abs().max()) == 0.0, "pad entries of %s moved (%s)" % (name, tag)


def _drive(case, eng, world):
    """Operations 1-5 of one phase on one engine -> {name: CPU tensor}."""
    xk, yk, e_in, n, _ = case.phase(world)
    phase = _lib.PHASE_WORLD if world else _lib.PHASE_JOINT
    P = Placer(eng)
    x_d, y_d = P.put("x", xk.reshape(n, -1)), P.put("y", yk.reshape(n, -1))
    e_d = P.put("eps", e_in) if e_in is not None else None
    lo = P.put("loss_out", torch.zeros(5))
    nets = _nets(eng, world)
    sp = case.sp(world, n)
    out = {}
    p0 = eng.params.clone()
    # 1: gradient stored
    eng.set_batch(x_d, y_d)
    P.check("set_batch")
    eng.grads.fill_(float("nan"))
    eng.forward_backward(phase, n, sp, eps=e_d, fused_adam=False, loss_out=lo)
    P.check("forward_backward")
    out["loss"], out["grads"] = lo.cpu().clone(), eng.segment(eng.grads, nets).cpu().clone()
    out["views"] = {k: v.cpu().clone() for k, v in eng.named_views(eng.grads).items()}
    # 2: evaluation
    eng.set_batch(x_d, y_d)
    eng.forward_backward(phase, n, sp, eps=e_d, backward=False, loss_out=lo)
    P.check("forward_backward(backward=False)")
    out["eval"] = lo.cpu().clone()
    # 3: the staged backward
    eng.set_batch(x_d, y_d)
    eng.grads.fill_(float("nan"))
    lo.zero_()
    eng.forward_seed(phase, n, sp, eps=e_d)
    P.check("forward_seed")
    k, n_stages = 0, 1
    while k < n_stages:
        _, _, n_stages = eng.backward_stage(phase, n, sp, k, loss_out=lo)
        P.check("backward_stage %d of %d" % (k, n_stages))
        k += 1
    out["staged_loss"], out["staged_grads"] = lo.cpu().clone(), eng.segment(eng.grads, nets).cpu().clone()
    # 4, 5: three fused steps, three flat-Adam steps, without and with weight decay
    pads = G.pad_mask(eng)
    for wd in (0.0, 0.01):
        for fused in (True, False):
            eng.params.copy_(p0)
            eng.exp_avg.zero_()
            eng.exp_avg_sq.zero_()
            for t in (1, 2, 3):
                spt = case.sp(world, n, t=t, wd=wd)
                eng.set_batch(x_d, y_d)
                eng.forward_backward(phase, n, spt, eps=e_d, fused_adam=fused, loss_out=lo)
                P.check("forward_backward(fused_adam=%s) step %d" % (fused, t))
                if not fused:
                    eng.adam(nets, spt)
                    P.check("adam step %d" % t)
            tag = "%s_wd%g" % ("fused" if fused else "flat", wd)
            for name, a in (("params", eng.params), ("exp_avg", eng.exp_avg), ("exp_avg_sq", eng.exp_avg_sq)):
                out["%s_%s" % (tag, name)] = a.cpu().clone()
            _pads_zero(eng, pads, tag)
            assert not _bits(out[tag + "_params"], p0.cpu()), tag
            out[tag + "_loss"] = lo.cpu().clone()
    eng.params.copy_(p0)
    return out


def _spans(n_windows, rows):
    mb = min(rows, n_windows)
    rag = max(1, mb // 2)
    return mb, rag, (0, mb), (n_windows - rag, rag)


def _drive_dataset(case, eng, world, next_states=None):
    """Operation 6 (lookahead 1): gather / train_step / train_step_prefetch over the trainer's dataset."""
    assert case.L == 1
    ds = case.reference_dataset
    phase = _lib.PHASE_WORLD if world else _lib.PHASE_JOINT
    P = Placer(eng)
    n_rows, n_win = ds.states.shape[0], len(ds.window_row)
    assert int(ds.window_row[-1]) + 1 == n_rows - 1            # the last window ends on the very last dataset row
    if P.on:
        placed, prow = G.poison_row_dataset(torch.from_numpy(ds.states), torch.from_numpy(ds.actions),
                                            torch.from_numpy(ds.window_row), next_states=next_states, device=DEV)
        for name, (buf, view) in placed.items():
            P.extra.append((name, buf, view) + ((prow,) if name == "window_row" else ()))
        eng.bind_dataset(placed["states"][1], placed["actions"][1], placed["window_row"][1],
                         next_states=placed["next_states"][1] if next_states is not None else None)
    else:
        st, ac, wr = ds.device_arrays(DEV)[:3]
        eng.bind_dataset(st, ac, wr, next_states=next_states.to(DEV) if next_states is not None else None)
    P.check("bind_dataset")
    mb, rag, first, last = _spans(n_win, min(case.rows, eng.max_batch))
    g = torch.Generator().manual_seed(77)
    Z = case.arch["Z"]
    e_mb = P.put("eps", torch.randn(mb, Z, generator=g)) if not world else None
    e_rag = P.put("eps_ragged", torch.randn(rag, Z, generator=g)) if not world else None
    lo = P.put("loss_out", torch.zeros(5))
    nets = _nets(eng, world)
    p0 = eng.params.clone()
    eng.exp_avg.zero_()
    eng.exp_avg_sq.zero_()
    out = {}
    for tag, (f, r), e in (("first", first, e_mb), ("last", last, e_rag)):
        eng.gather(f, r)
        P.check("gather(%d, %d)" % (f, r))
        eng.grads.fill_(float("nan"))
        eng.forward_backward(phase, r, case.sp(world, r), eps=e, fused_adam=False, loss_out=lo)
        P.check("forward_backward after gather(%d, %d)" % (f, r))
        out["gather_%s_loss" % tag], out["gather_%s_grads" % tag] = lo.cpu().clone(), eng.segment(eng.grads, nets).cpu().clone()
    eng.train_step(phase, first[0], mb, case.sp(world, mb, t=1), eps=e_mb, loss_out=lo)
    P.check("train_step")
    out["step1_loss"] = lo.cpu().clone()
    eng.train_step(phase, first[0], mb, case.sp(world, mb, t=2), eps=e_mb, loss_out=lo, next_span=last)
    P.check("train_step_prefetch")
    out["step2_loss"] = lo.cpu().clone()
    eng.train_step(phase, last[0], rag, case.sp(world, rag, t=3), eps=e_rag, loss_out=lo)
    P.check("train_step on the prefetched ragged last minibatch")
    out["step3_loss"] = lo.cpu().clone()
    for name, a in (("params", eng.params), ("exp_avg", eng.exp_avg), ("exp_avg_sq", eng.exp_avg_sq)):
        out["steps_" + name] = a.cpu().clone()
    _pads_zero(eng, G.pad_mask(eng), "train steps")
    assert not _bits(out["steps_params"], p0.cpu())
    eng.params.copy_(p0)
    eng.exp_avg.zero_()
    eng.exp_avg_sq.zero_()
    eng.invalidate_staging()
    return out


def _against_oracle(case, world, got, what):
    _, _, _, n, want = case.phase(world)
    for key in ("loss", "eval", "staged_loss"):
        loss = got[key]
        assert float(loss[0]) == pytest.approx(float(want["total"]), rel=1e-5, abs=1e-9), (what, key)
        for i, k in enumerate(TERMS):
            assert float(loss[1 + i]) == pytest.approx(float(want[k]), rel=1e-5, abs=1e-9), (what, key, k)
    for k, gr in want["grads"].items():
        ours = got["views"][k]
        assert torch.isfinite(ours).all(), (what, k)
        err = max_err_scaled(ours, gr)
        assert err < 1e-4, (what, k, err)
        if case.strict:
            assert rel_err(ours, gr) < 1e-4, (what, k)
    assert _bits(got["staged_grads"], got["grads"]), what        # the staged backward is the same launches


def _finite(got, what):
    for k, v in got.items():
        if isinstance(v, torch.Tensor) and k != "views":
            assert torch.isfinite(v).all(), "%s: %s is not finite" % (what, k)


def _same(ref, got, what):
    assert ref.keys() == got.keys()
    for k in ref:
        if k == "views":
            continue
        assert _bits(ref[k], got[k]), "%s: %s differs from the unguarded engine's" % (what, k)


def _run(case, twins=None, worlds=(True, False), dataset=False, with_next=False):
    ref = case.reference()
    twins = twins if twins is not None else sorted({case.rows, TWIN_ROWS})
    next_states = None
    if dataset:
        case.reference_dataset = case.tr.train_loader.dataset
        if with_next:                                            # a next_states array (cond "rel"), row-aligned with states
            next_states = torch.randn(case.reference_dataset.states.shape, generator=torch.Generator().manual_seed(5))
    for world in worlds:
        want = _drive(case, ref, world)
        _finite(want, "unguarded")
        want_ds = _drive_dataset(case, ref, world, next_states) if dataset else None
        for mb in twins:
            what = "max_batch %d, %s phase" % (mb, "world" if world else "joint")
            eng = case.twin(mb)
            got = _drive(case, eng, world)
            _finite(got, what)
            _against_oracle(case, world, got, what)
            _same(want, got, what)
            if dataset:
                got_ds = _drive_dataset(case, eng, world, next_states)
                _finite(got_ds, what)
                _same(want_ds, got_ds, what)
            del eng


# ------------------------------------------------------------------------------------- the sweep's shapes
@pytest.mark.parametrize("seed", PLAIN)
def test_sweep_shapes_inside_guard_bands(seed):
    c = _case(seed)
    case = _sweep_case(c, seed)
    _run(case, dataset=c["L"] == 1, with_next=seed == 20)      # (one case with a next_states array)


@pytest.mark.parametrize("seed", STACKS)
def test_per_layer_stacks_inside_guard_bands(seed):
    c = _case_stacks(seed)
    _run(_sweep_case(c, seed), dataset=c["L"] == 1)


def test_the_chosen_seeds_cover_every_row_count_lookahead_and_loss():
    cs = [_case(s) for s in PLAIN] + [_case_stacks(s) for s in STACKS]
    assert len(cs) == 12
    assert {c["rows"] for c in cs} == {1, 2, 7, 31, 32, 33, 64, 97, 130}
    assert {c["L"] for c in cs} == {1, 2, 3} and {c["loss"] for c in cs} == {"MSE", "L1"}


# ------------------------------------------------------------------------------------- joint-phase state reconstruction
@pytest.mark.parametrize("rows", [5, 33])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_joint_state_reconstruction_inside_guard_bands(L, rows):
    """world_model_s_rec_coeff = 0.5 in the joint phase at odd widths: the forward-only pass (lookahead 1) and the
    input-gradient-only chain through the frozen world model (lookahead 2, 3)."""
    from test_gpu_srec_joint import _margin
    arch = R.make_arch(23, 7, latent=5, te=(129, 2), md=(31, 2), wm=(100, 3))
    pool = rows + 8                                              # exactly `rows` rows run: the first that lie off every kink
    data = R.synth_demo(3, 2, pool + L + 3, 23, 7, kind="dynamics")
    X, Y = R.build_windows(data, lookahead=L)
    x, y = next(iter(R.make_loader(X, Y, pool)))
    sd = R.perturb_biases(R.init_state_dict(arch, seed=4), seed=6)
    es = R.eps_stream(5, 5)
    eps = torch.stack([es(t, (pool, 5)) for t in range(L)])
    cfg = dict(R.phase_coeffs(False), s_rec_coeff=0.5)
    keep = torch.nonzero(_margin(arch, sd, x, y, eps, cfg) > 4e-6)[:, 0]
    assert keep.numel() >= rows
    keep = keep[:rows]
    x, y, eps = x[keep], y[keep], eps[:, keep]
    case = Case(arch, data, x, y, sd, eps, L=L, joint_cfg=cfg, margin=_margin, extra={"world_model_s_rec_coeff": 0.5},
                strict=False)
    assert float(case.phase(False)[4]["loss_s"]) > 0.0
    _run(case, worlds=(False,))


# ------------------------------------------------------------------------------------- helper, learned prior, input subset
def test_decoder_helper_inside_guard_bands():
    from test_gpu_helper_training import _trainer, _weights
    base = R.make_arch(7, 3, latent=4, te=(16, 2), md=(24, 2), wm=(32, 2))
    h, sd = _weights(base)
    data = R.synth_demo(0, 2, 40, 7, 3, kind="dynamics")
    X, Y = R.build_windows(data)
    x, y = next(iter(R.make_loader(X, Y, 33)))
    eps = R.eps_stream(2, 4)(0, (33, 4))[None]

    def trainer(arch, data, batch, **kw):
        return _trainer(base, data, batch, **kw)
    _run(Case(h, data, x, y, sd, eps, trainer=trainer, strict=False), dataset=True)


def test_learned_prior_inside_guard_bands():
    from test_gpu_priors import _setup
    arch, data, x, y, sd, eps = _setup(R.PRIORS[1], "tiny")
    _run(Case(arch, data, x, y, sd, eps[None], strict=False), dataset=True)


def test_input_subset_inside_guard_bands():
    """motor_decoder_inputs = ["body"]: the sampler's z goes to the side panel, the last one before `W.zero`."""
    arch = R.with_inputs(R.make_arch(23, 7, latent=8, te=(64, 2), md=(96, 2), wm=(128, 2)), ("body", "task"), ("body",))
    data = R.synth_demo(0, 2, 40, 23, 7, kind="dynamics")
    X, Y = R.build_windows(data)
    x, y = next(iter(R.make_loader(X, Y, 33)))
    sd = R.perturb_biases(R.init_state_dict(arch, seed=1), seed=3)
    eps = R.eps_stream(2, 8)(0, (33, 8))[None]
    _run(Case(arch, data, x, y, sd, eps, strict=False), dataset=True)


# ------------------------------------------------------------------------------------- wide tile bodies
@pytest.mark.parametrize("rows,fwd,pair", [(512, "64x32", "64x32"), (1024, "64x64", "64x32"), (544, "32x32", "32x32")])
def test_wide_tile_bodies_inside_guard_bands(rows, fwd, pair):
    """1024-wide stacks of depth 2: 512 rows run the forward and the pairs' input-gradient half on 64x32 tiles, 1024 rows
    the forward on 64x64; 544 rows (M % 64 == 32) must fall back to 32-row tiles.  max_batch == rows."""
    assert TR.plan_tiles("forward", rows, 1024)[0] == fwd and TR.plan_tiles("pair", rows, 1024)[0] == pair
    arch = R.make_arch(23, 7, latent=8, te=(1024, 2), md=(1024, 2), wm=(1024, 2))
    pool = rows + 300
    data = R.synth_demo(5, 2, pool // 2 + 4, 23, 7, kind="dynamics")
    X, Y = R.build_windows(data)
    x, y = next(iter(R.make_loader(X, Y, pool)))
    sd = R.perturb_biases(R.init_state_dict(arch, seed=2), seed=4)
    eps = R.eps_stream(3, 8)(0, (x.shape[0], 8))
    ok = (R.relu_kink_margin(arch, sd, x, y, eps, True) > 4e-6) & (R.relu_kink_margin(arch, sd, x, y, eps, False) > 4e-6)
    keep = torch.nonzero(ok)[:, 0]
    assert keep.numel() >= rows
    keep = keep[:rows]
    _run(Case(arch, data, x[keep], y[keep], sd, eps[keep][None]), twins=[rows])


# ------------------------------------------------------------------------------------- the opt-in direct path
@pytest.mark.parametrize("world", [True, False])
def test_direct_path_reads_nothing_it_keeps_from_behind_the_last_dataset_row(world):
    """pvae_set_direct at the dimensions of tests/test_gpu_direct.py (197 / 45, 2 x 512, 250 rows): the second and third
    minibatch hold the window that ends on the last dataset row, where the 16-byte chunk that reaches 12 bytes past the
    array fetches poison.  Nothing of it may reach a result: finite, bit-equal to the staged step of the unguarded engine
    (whose array has zeros behind it), guards intact.  (World phase: the world model gathers s_t and a_t rows only and the
    loss epilogue reads s_{t+1} element by element.  Joint phase: the encoder's operand [s_t | s_{t+1}] has 394 columns,
    its last chunk ends two floats behind the array -- NaN x the weight block's zero pad columns is NaN, which the hidden
    ReLU turned into a first layer of zeros for that window: finite and wrong.  That minibatch now stages its panels,
    DirectStep::enter.)"""
    Db, Da, rows, T = 197, 45, 250, 300
    arch = R.make_arch(Db, Da, latent=32, te=(512, 2), md=(512, 2), wm=(512, 2))
    tr = make_trainer(arch, R.synth_demo(0, 2, 8, Db, Da), rows, device=DEV)
    tr.model.load_state_dict(R.perturb_biases(R.init_state_dict(arch, 1), 3))
    g = torch.Generator().manual_seed(5)
    states, actions = torch.randn(2 * T, Db, generator=g), torch.randn(2 * T, Da, generator=g).clamp_(-3, 3)
    idx = (torch.arange(2)[:, None] * T + torch.arange(T - 1)[None, :]).reshape(-1).to(torch.int32)
    n_win = idx.numel()
    assert int(idx[-1]) + 1 == 2 * T - 1
    phase = _lib.PHASE_WORLD if world else _lib.PHASE_JOINT
    c = R.phase_coeffs(world)
    eps = torch.randn(3, rows, 32, generator=g)
    spans = [(0, rows), (n_win - rows, rows), (n_win - rows, rows)]

    def steps(eng, direct, P):
        eng.set_direct(direct)
        lo = P.put("loss_out", torch.zeros(3, 5))
        e_d = P.put("eps", eps)
        act = []
        for i, (f, r) in enumerate(spans):
            sp = make_step_params(lr=5e-4, adam_t=(i + 1,) * 3, a_rec=c["a_rec_coeff"], kl=c["vae_kl_coeff"],
                                  s_rec=c["s_rec_coeff"], cyc=c["vae_cycle_coeff"], global_rows=r)
            act.append(eng.direct_active(phase, r, sp, fused=True))
            eng.train_step(phase, f, r, sp, eps=e_d[i], loss_out=lo[i], next_span=spans[i + 1] if i + 1 < len(spans) else None)
            P.check("train_step %d (direct=%s)" % (i, direct))
        return act, [lo.cpu().clone(), eng.params.cpu().clone(), eng.exp_avg.cpu().clone(), eng.exp_avg_sq.cpu().clone()]

    ref = tr.engine
    room = lambda a: torch.cat([a.reshape(-1), torch.zeros(16)]).to(DEV)[: a.numel()].view(a.shape)   # noqa: E731
    ref.bind_dataset(room(states), room(actions), idx.to(DEV))
    p0 = ref.params.clone()
    act, staged = steps(ref, False, Placer(ref))
    assert not any(act)
    twin = HipEngine(ref.arch, rows, DEV, lookahead=1)
    G.guard_engine(twin, direct=True)
    twin.params.copy_(p0)
    P = Placer(twin)
    placed, prow = G.poison_row_dataset(states, actions, idx, device=DEV)
    for name, (buf, view) in placed.items():
        P.extra.append((name, buf, view) + ((prow,) if name == "window_row" else ()))
    twin.bind_dataset(placed["states"][1], placed["actions"][1], placed["window_row"][1])
    act, direct = steps(twin, True, P)
    assert all(act), "the step did not take the direct path"
    for a, b in zip(staged, direct):
        assert torch.isfinite(b).all() and _bits(a, b)
    pads = G.pad_mask(twin).cpu()
    for a in direct[1:]:
        assert float(a[pads].abs().max()) == 0.0


# ------------------------------------------------------------------------------------- infer
@pytest.mark.parametrize("noise", [True, False])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 33])
def test_infer_writes_guarded_outputs_only(rows, noise):
    """The fused <= 4-row rollout path and the staged path, outputs through `out=` into guarded caller buffers; against the
    unguarded engine bit for bit and the oracle's forward at 2e-5 (the bound of the forward read-backs of
    test_gpu_priors.py / test_gpu_helper_training.py)."""
    c = _case(11)
    case = _sweep_case(c, 11)
    ref = case.reference()
    Db, Da, Z = c["Db"], c["Da"], c["Z"]
    g = torch.Generator().manual_seed(100 + rows)
    obs, eps = torch.randn(rows, 2 * Db, generator=g), torch.randn(rows, Z, generator=g)
    model = R.RefModel(case.arch)
    model.load_state_dict(case.sd)
    model.latent_prior_noise = noise
    model.eps_source = lambda shape: eps
    with torch.no_grad():
        logits = model(obs)
    plain = HipEngine(ref.arch, TWIN_ROWS, DEV)                  # (the case's trainer holds 32 rows)
    plain.params.copy_(ref.params)
    want = plain.infer(obs.to(DEV), eps=eps.to(DEV) if noise else None, noise=noise)
    for mb in (33, TWIN_ROWS):
        eng = case.twin(mb)
        P = Placer(eng)
        o_d = P.put("obs", obs)
        e_d = P.put("eps", eps) if noise else None
        out = (P.put("a_hat", torch.zeros(rows, Da), fill=False), P.put("s2_hat", torch.zeros(rows, Db), fill=False),
               P.put("z", torch.zeros(rows, Z), fill=False))
        got = eng.infer(o_d, eps=e_d, noise=noise, out=out)
        P.check("infer(%d rows)" % rows)
        assert all(a is b for a, b in zip(got, out))
        for a, b in zip(want, got):
            assert torch.isfinite(b).all() and _bits(a.cpu(), b.cpu())
        assert max_err_scaled(got[0].cpu(), logits[:, :Da]) < 2e-5
        assert max_err_scaled(got[1].cpu(), model.cur_future_state) < 2e-5
        assert max_err_scaled(got[2].cpu(), model.cur_z) < 2e-5
