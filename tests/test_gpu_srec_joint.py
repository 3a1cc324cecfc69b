"""Joint phase with `world_model_s_rec_coeff` > 0 (tpv:411-414, 421-434 while the world model is frozen, tpv:347-350): the
HIP step through `forward_backward`, as test_gpu_lookahead.py drives it, against the oracle and the capture of the
reference's own trainer (tests/golden/srec_tiny.npz).  Bounds are the standing ones of test_gpu_parity.py /
test_gpu_lookahead.py: loss terms 1e-5 relative, gradients 1e-4 by max_err_scaled, samples on a ReLU kink removed.

lookahead 1: s1 and a_gt are data -- the term is a forward-only pass of the world model, a number in the loss; encoder and
decoder gradients are the bits of the same step without it, and nothing of the world model is touched.
lookahead > 1: s1_t (t >= 1) is the world model's own prediction -- the term's gradient enters through the state columns
of the frozen world model's first-layer input gradient; the isolated case has no other gradient path at all.

A context runs the term once it has been told to (`HipEngine.set_joint_s_rec`, pvae_set_option "joint_s_rec"); the trainer
tells it when its config holds a non-zero `world_model_s_rec_coeff`.  A context that was not told refuses as before."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import refpath as R
from physicsvae_amd import _lib
from physicsvae_amd.engine import make_step_params
from test_srec_cpu import ALONE, capture_inputs, captured_grads, scaled_outputs
from util import arch_from_meta, make_trainer, max_err_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH = R.make_arch(7, 3, latent=4, te=(32, 2), md=(32, 2), wm=(32, 2))
S_REC = 0.5
TERMS = ("loss_a", "loss_kl", "loss_s", "loss_cyc")
_cache = {}


def _coeffs(**kw):
    return dict(R.phase_coeffs(False), **kw)


def _sp(rows, c, **kw):
    return make_step_params(lr=5e-4, a_rec=c["a_rec_coeff"], kl=c["vae_kl_coeff"], s_rec=c["s_rec_coeff"],
                            cyc=c["vae_cycle_coeff"], global_rows=rows, **kw)


def _data(arch, L):
    key = ("data", arch["Db"], arch["Da"], L)
    if key not in _cache:
        data = R.synth_demo(0, 3, 40, arch["Db"], arch["Da"], kind="dynamics")
        X, Y = R.build_windows(data, lookahead=L)
        x, y = next(iter(R.make_loader(X, Y, 64)))
        es = R.eps_stream(2, arch["Z"])
        eps = torch.stack([es(t, (64, arch["Z"])) for t in range(L)])
        _cache[key] = (data, x, y, eps)
    return _cache[key]


def _trainer(L, loss="MSE"):
    """One trainer per (lookahead, loss) for the whole module: tests load the weights they need."""
    key = ("trainer", L, loss)
    if key not in _cache:
        _cache[key] = make_trainer(ARCH, _data(ARCH, L)[0], 64, device=DEV, extra={"lookahead": L, "loss": loss})
    return _cache[key]


def _margin(arch, sd, x, y, eps, coeffs):
    """R.relu_kink_margin with the demonstrated-action pass included: the smallest |pre-activation| of every hidden ReLU
    that runs under `coeffs` (the oracle's helper runs the default joint coefficients, where that pass does not exist)."""
    model = R.RefModel(arch)
    model.load_state_dict(sd)
    model.eps_source = R._eps_feeder(eps)
    seen, hooks = [], []
    nets = [("_task_encoder", "te"), ("_motor_decoder", "md"), ("_world_model", "wm")]
    if arch.get("mh"):
        nets.append(("_motor_decoder_helper", "mh"))
    for net, key in nets:
        for slim, a in zip(list(getattr(model, net)._model)[:-1], R.stack_acts(arch, key)):
            if a == "relu":
                hooks.append(slim._model[0].register_forward_hook(lambda m, i, o: seen.append(o.detach().abs().min(dim=1).values)))
    with torch.no_grad():
        R.compute_loss(model, x, y, coeffs)
    for h in hooks:
        h.remove()
    own = torch.stack(seen).min(dim=0).values
    return torch.minimum(own, R.relu_kink_margin(arch, sd, x, y, eps, False))


def _off_kinks(arch, sd, x, y, eps, coeffs):
    keep = _margin(arch, sd, x, y, eps, coeffs) > 4e-6
    rows = x.shape[0]
    assert int(keep.sum()) >= max(1, rows - max(4, rows // 4))
    return x[keep], y[keep], eps[:, keep]


def _wm_state(eng):
    off, cnt = eng.segments[_lib.NET_WM]
    return [a[off: off + cnt].clone() for a in (eng.params, eng.grads, eng.exp_avg, eng.exp_avg_sq)]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check_terms(loss, want):
    assert float(loss[0]) == pytest.approx(float(want["total"]), rel=1e-5)
    for i, k in enumerate(TERMS):
        assert float(loss[1 + i]) == pytest.approx(float(want[k]), rel=1e-5, abs=1e-9), k


def _check_grads(eng, want):
    gv = eng.named_views(eng.grads)
    for k, gr in want["grads"].items():
        ours = gv[k].cpu()
        assert torch.isfinite(ours).all(), k
        assert max_err_scaled(ours, gr) < 1e-4, k


# ------------------------------------------------------------------------------------------------ 0: the switch
def test_the_context_runs_the_term_once_told_and_the_trainer_tells_it():
    _, x, y, eps = _data(ARCH, 1)
    x, y, eps = x[:5], y[:5], eps[:, :5]
    sp = _sp(5, _coeffs(s_rec_coeff=S_REC))
    plain = make_trainer(ARCH, _data(ARCH, 1)[0], 64, device=DEV)
    told = make_trainer(ARCH, _data(ARCH, 1)[0], 64, device=DEV, extra={"world_model_s_rec_coeff": S_REC})
    sd = R.perturb_biases(R.init_state_dict(ARCH, seed=1), seed=3)
    want = R.loss_and_grads(ARCH, sd, x, y, eps, False, coeff_cfg=_coeffs(s_rec_coeff=S_REC))
    for tr in (plain, told):
        tr.model.load_state_dict(sd)
        tr.engine.set_batch(x, y)
    with pytest.raises(RuntimeError, match="joint_s_rec"):
        plain.engine.forward_backward(_lib.PHASE_JOINT, 5, sp, eps=eps)
    _check_terms(told.engine.forward_backward(_lib.PHASE_JOINT, 5, sp, eps=eps, fused_adam=False).cpu(), want)
    plain.engine.set_joint_s_rec(True)
    _check_terms(plain.engine.forward_backward(_lib.PHASE_JOINT, 5, sp, eps=eps, fused_adam=False).cpu(), want)
    plain.engine.set_joint_s_rec(False)
    with pytest.raises(RuntimeError, match="s_rec"):
        plain.engine.forward_backward(_lib.PHASE_JOINT, 5, sp, eps=eps)


# ------------------------------------------------------------------------------------------------ 1: lookahead 1
@pytest.mark.parametrize("lk", ["MSE", "L1"])
@pytest.mark.parametrize("rows", [1, 5, 33, 64])
def test_lookahead_one_adds_the_term_and_moves_nothing(rows, lk):
    tr = _trainer(1, lk)
    eng = tr.engine
    eng.set_joint_s_rec(True)
    _, x, y, eps = _data(ARCH, 1)
    x, y, eps = x[:rows], y[:rows], eps[:, :rows]
    sd = R.perturb_biases(R.init_state_dict(ARCH, seed=1), seed=3)
    tr.model.load_state_dict(sd)
    c1, c0 = _coeffs(s_rec_coeff=S_REC), _coeffs()
    want = R.loss_and_grads(ARCH, sd, x, y, eps, False, coeff_cfg=c1, loss=lk)
    assert float(want["loss_s"]) > 0.0
    te_md = [_lib.NET_TE, _lib.NET_MD]
    res = {}
    for tag, c in (("without", c0), ("with", c1)):
        eng.set_batch(x, y)
        eng.grads.fill_(float("nan"))
        eng.exp_avg.normal_(0, 1e-3)
        eng.exp_avg_sq.uniform_(1e-6, 1e-4)
        before = _wm_state(eng)
        loss = eng.forward_backward(_lib.PHASE_JOINT, rows, _sp(rows, c, loss=lk), eps=eps, fused_adam=False).cpu().clone()
        for a, b in zip(before, _wm_state(eng)):              # parameters, gradient segment (still the NaN fill), both moments
            assert _same_bits(a, b), tag
        res[tag] = (loss, eng.segment(eng.grads, te_md).clone())
    _check_terms(res["with"][0], want)
    assert torch.equal(res["with"][1], res["without"][1])     # every encoder / decoder gradient, bit for bit
    assert torch.isfinite(res["with"][1]).all()
    assert float(res["without"][0][3]) == 0.0 and torch.equal(res["with"][0][[1, 2, 4]], res["without"][0][[1, 2, 4]])
    # what the step leaves behind is the predicted-action pass (the demonstrated-action pass ran first)
    assert max_err_scaled(eng.read("s2_hat", rows).cpu(), want["future_state"]) < 3e-5
    # gradients against the oracle, off the kinks
    xk, yk, ek = _off_kinks(ARCH, sd, x, y, eps, c1)
    wk = R.loss_and_grads(ARCH, sd, xk, yk, ek, False, coeff_cfg=c1, loss=lk)
    eng.set_batch(xk, yk)
    eng.forward_backward(_lib.PHASE_JOINT, xk.shape[0], _sp(xk.shape[0], c1, loss=lk), eps=ek, fused_adam=False)
    _check_grads(eng, wk)
    # the fused-Adam path: the world model's parameters and moments stay, encoder and decoder move as without the term
    fused = {}
    for tag, c in (("without", c0), ("with", c1)):
        tr.model.load_state_dict(sd)
        eng.exp_avg.zero_(); eng.exp_avg_sq.zero_()
        off, cnt = eng.segments[_lib.NET_WM]
        eng.exp_avg[off: off + cnt].normal_(0, 1e-3)
        eng.exp_avg_sq[off: off + cnt].uniform_(1e-6, 1e-4)
        before = _wm_state(eng)
        eng.set_batch(x, y)
        loss = eng.forward_backward(_lib.PHASE_JOINT, rows, _sp(rows, c, loss=lk, adam_t=(3, 3, 3)), eps=eps, fused_adam=True).cpu().clone()
        for a, b in zip(before, _wm_state(eng)):
            assert _same_bits(a, b), tag
        fused[tag] = (loss, eng.segment(eng.params, te_md).clone(), eng.segment(eng.exp_avg, te_md).clone())
    assert torch.equal(fused["with"][1], fused["without"][1]) and torch.equal(fused["with"][2], fused["without"][2])
    assert float(fused["with"][2].abs().max()) > 0.0          # (the step did train them)
    _check_terms(fused["with"][0], want)


def test_lookahead_one_and_two_match_the_reference_capture(golden):
    g = golden("srec_tiny")
    for L in (1, 2):
        arch, x, y, eps, sd = capture_inputs(g, L)
        rows = x.shape[0]
        n_ep, n_steps = [int(v) for v in g["meta"][9:11]]
        tr = make_trainer(arch, R.synth_demo(0, n_ep, n_steps, arch["Db"], arch["Da"], kind="dynamics"), rows, device=DEV,
                          extra={"lookahead": L})
        tr.model.load_state_dict(sd)
        eng = tr.engine
        eng.set_joint_s_rec(True)
        c = float(g["s_rec_coeff"])
        eng.set_batch(x, y)
        loss = eng.forward_backward(_lib.PHASE_JOINT, rows, _sp(rows, _coeffs(s_rec_coeff=c)), eps=eps, fused_adam=False).cpu()
        pre = "L%d/" % L
        assert float(loss[0]) == pytest.approx(float(g[pre + "total"]), rel=1e-5)
        assert float(loss[3]) == pytest.approx((float(g[pre + "total"]) - float(g[pre + "total_without"])) / c, rel=1e-5)
        assert bool((_margin(arch, sd, x, y, eps, _coeffs(s_rec_coeff=c)) > 4e-6).all())     # (8 rows, none on a kink)
        gv = eng.named_views(eng.grads)
        for k, gr in captured_grads(g, pre).items():
            assert max_err_scaled(gv[k].cpu(), gr) < 1e-4, (L, k)


def test_direct_first_layers_carry_the_term_too():
    """`set_direct(True)` at dims where the joint step qualifies (197 / 45, 2x512, 250 rows): the demonstrated-action pass
    gathers [s_t | a_t] as the world phase does.  Direct == staged bit for bit with the term; encoder and decoder end where
    they end without it; the world model is not touched."""
    arch = R.make_arch(197, 45, latent=32, te=(512, 2), md=(512, 2), wm=(512, 2))
    rows, n_ep, T = 250, 2, 500
    tr = make_trainer(arch, R.synth_demo(0, 2, 8, 197, 45), rows, device=DEV)
    eng = tr.engine
    eng.set_joint_s_rec(True)
    gen = torch.Generator(device=DEV).manual_seed(5)

    def roomy(n, w):
        buf = torch.zeros(n * w + 16, device=DEV)
        v = buf[: n * w].view(n, w)
        v.copy_(torch.randn(n, w, generator=gen, device=DEV))
        return v
    states, actions = roomy(n_ep * T, 197), roomy(n_ep * T, 45).clamp_(-3, 3)
    idx = (torch.arange(n_ep, device=DEV)[:, None] * T + torch.arange(T - 1, device=DEV)[None, :]).reshape(-1).to(torch.int32)
    eng.bind_dataset(states, actions, idx)
    sd = R.perturb_biases(R.init_state_dict(arch, 1), 3)
    eps = torch.randn(2, rows, 32, generator=torch.Generator().manual_seed(9)).to(DEV)
    te_md = [_lib.NET_TE, _lib.NET_MD]
    got = {}
    for s_rec in (0.0, S_REC):
        for direct in (False, True):
            eng.set_direct(direct)
            tr.model.load_state_dict(sd)
            eng.exp_avg.zero_(); eng.exp_avg_sq.zero_(); eng.invalidate_staging()
            before = _wm_state(eng)
            out = torch.zeros(2, 5, device=DEV)
            for i in range(2):                                    # (the second minibatch crosses the episode boundary at window 499)
                sp = _sp(rows, _coeffs(s_rec_coeff=s_rec), adam_t=(i + 1, i + 1, i + 1))
                assert eng.direct_active(_lib.PHASE_JOINT, rows, sp, fused=True) == direct
                first = 200 + i * rows
                eng.train_step(_lib.PHASE_JOINT, first, rows, sp, eps=eps[i].contiguous(), loss_out=out[i], next_span=(first + rows, rows))
            torch.cuda.synchronize()
            for a, b in zip(before, _wm_state(eng)):
                assert _same_bits(a, b), (s_rec, direct)
            got[(s_rec, direct)] = (out.cpu(), eng.segment(eng.params, te_md).clone(), eng.segment(eng.exp_avg_sq, te_md).clone())
    eng.set_direct(False)
    for a, b in zip(got[(S_REC, False)], got[(S_REC, True)]):
        assert torch.equal(a, b)
    for direct in (False, True):
        assert torch.equal(got[(S_REC, direct)][1], got[(0.0, direct)][1]) and torch.equal(got[(S_REC, direct)][2], got[(0.0, direct)][2])
        with_, without = got[(S_REC, direct)][0], got[(0.0, direct)][0]
        assert bool((with_[:, 3] > 0.1).all()) and bool((without[:, 3] == 0).all())
        assert torch.allclose(with_[:, 0], without[:, 0] + S_REC * with_[:, 3], rtol=1e-6)
    # the term itself against the oracle on the first minibatch
    w = idx[200: 200 + rows].long()
    x = torch.cat([states[w], states[w + 1]], dim=1).cpu()[:, None, :]
    y = actions[w].cpu()[:, None, :]
    want = R.loss_and_grads(arch, sd, x, y, eps[0:1].cpu(), False, coeff_cfg=_coeffs(s_rec_coeff=S_REC))
    _check_terms(got[(S_REC, True)][0][0], want)


# ------------------------------------------------------------------------------------------------ 2, 3: the unroll
@pytest.mark.parametrize("rows", [5, 33])
@pytest.mark.parametrize("L", [2, 3])
def test_unrolled_default_coefficients_plus_the_term(L, rows):
    tr = _trainer(L)
    eng = tr.engine
    eng.set_joint_s_rec(True)
    _, x, y, eps = _data(ARCH, L)
    sd = R.perturb_biases(R.init_state_dict(ARCH, seed=1), seed=3)
    tr.model.load_state_dict(sd)
    c1 = _coeffs(s_rec_coeff=S_REC)
    x, y, eps = _off_kinks(ARCH, sd, x[:rows], y[:rows], eps[:, :rows], c1)
    rows = x.shape[0]
    want = R.loss_and_grads(ARCH, sd, x, y, eps, False, coeff_cfg=c1)
    eng.set_batch(x, y)
    eng.grads.fill_(float("nan"))
    before = _wm_state(eng)
    loss = eng.forward_backward(_lib.PHASE_JOINT, rows, _sp(rows, c1), eps=eps, fused_adam=False).cpu()
    _check_terms(loss, want)
    assert float(loss[3]) > 0.0
    _check_grads(eng, want)
    for a, b in zip(before, _wm_state(eng)):
        assert _same_bits(a, b)
    for t in range(L):                                             # the chain of predicted states is the one without the term
        assert max_err_scaled(eng.read("s2_hat", rows, step=t).cpu(), want["steps"][t]["future_state"]) < 3e-5, t
    # fused Adam == stored gradients + flat Adam on encoder and decoder; the world model stays
    p0 = eng.params.clone()
    eng.exp_avg.zero_(); eng.exp_avg_sq.zero_()
    sp = _sp(rows, c1, adam_t=(2, 2, 2))
    eng.adam([_lib.NET_TE, _lib.NET_MD], sp)
    p_sep, m_sep = eng.params.clone(), eng.exp_avg.clone()
    assert not torch.equal(p_sep, p0)
    eng.params.copy_(p0)                       # whole arena, pad entries included
    eng.exp_avg.zero_(); eng.exp_avg_sq.zero_()
    eng.set_batch(x, y)
    eng.forward_backward(_lib.PHASE_JOINT, rows, sp, eps=eps, fused_adam=True)
    assert torch.equal(eng.params, p_sep) and torch.equal(eng.exp_avg, m_sep)


@pytest.mark.parametrize("L", [2, 3])
def test_unrolled_term_isolated(L):
    """a_rec 0, kl 0, cyc 0, s_rec 1, output layers of decoder and world model x 30.  The oracle's largest gradient entry is
    3.6e-4 (lookahead 2) / 2.9e-4 (lookahead 3) at 33 rows, against 3e-7 at unscaled weights and a shift of 4e-6 of the
    default joint gradient's scale -- so only here does a missing gradient path fail the 1e-4 bound: every entry of every
    tensor comes through the frozen world model's demonstrated-action pass."""
    tr = _trainer(L)
    eng = tr.engine
    eng.set_joint_s_rec(True)
    _, x, y, eps = _data(ARCH, L)
    sd = scaled_outputs(ARCH, R.perturb_biases(R.init_state_dict(ARCH, seed=1), seed=3), 30.0)
    tr.model.load_state_dict(sd)
    x, y, eps = _off_kinks(ARCH, sd, x[:33], y[:33], eps[:, :33], ALONE)
    rows = x.shape[0]
    want = R.loss_and_grads(ARCH, sd, x, y, eps, False, coeff_cfg=ALONE)
    top = max(float(g.abs().max()) for g in want["grads"].values())
    print("isolated term, lookahead %d, %d rows: largest oracle gradient entry %.3g" % (L, rows, top))
    assert top > 1e-4                                              # (measured 3.6e-4 / 2.9e-4: not a comparison of zeros)
    for k, g in want["grads"].items():
        assert float(g.abs().max()) > 0.0, k
    eng.set_batch(x, y)
    eng.grads.fill_(float("nan"))
    before = _wm_state(eng)
    loss = eng.forward_backward(_lib.PHASE_JOINT, rows, _sp(rows, ALONE), eps=eps, fused_adam=False).cpu()
    _check_terms(loss, want)
    assert float(loss[0]) == float(loss[3])
    _check_grads(eng, want)
    for a, b in zip(before, _wm_state(eng)):
        assert _same_bits(a, b)


@pytest.mark.parametrize("L", [2, 3])
def test_unrolled_term_isolated_matches_the_reference_capture(golden, L):
    g = golden("srec_tiny")
    arch, x, y, eps, sd = capture_inputs(g, L)
    sd = scaled_outputs(arch, sd, float(g["out_scale"]))
    rows = x.shape[0]
    n_ep, n_steps = [int(v) for v in g["meta"][9:11]]
    tr = make_trainer(arch, R.synth_demo(0, n_ep, n_steps, arch["Db"], arch["Da"], kind="dynamics"), rows, device=DEV,
                      extra={"lookahead": L})
    tr.model.load_state_dict(sd)
    eng = tr.engine
    eng.set_joint_s_rec(True)
    eng.set_batch(x, y)
    loss = eng.forward_backward(_lib.PHASE_JOINT, rows, _sp(rows, ALONE), eps=eps, fused_adam=False).cpu()
    pre = "iso%d/" % L
    assert float(loss[0]) == pytest.approx(float(g[pre + "total"]), rel=1e-5)
    assert bool((_margin(arch, sd, x, y, eps, ALONE) > 4e-6).all())
    gv = eng.named_views(eng.grads)
    for k, gr in captured_grads(g, pre).items():
        assert float(gr.abs().max()) > 0.0
        assert max_err_scaled(gv[k].cpu(), gr) < 1e-4, k


# ------------------------------------------------------------------------------------------------ 4: helper, input subset
def test_unrolled_term_with_the_helper(golden):
    """helper_train_look2_tiny's architecture (the motor decoder's helper rides in every unrolled step's a_hat)."""
    from test_gpu_helper_training import _trainer as helper_trainer, _weights
    g = golden("helper_train_look2_tiny")
    base = arch_from_meta(g["meta"])
    h, sd = _weights(base)
    n_ep, n_steps, batch = [int(v) for v in g["meta"][9:12]]
    data = R.synth_demo(0, n_ep, n_steps, base["Db"], base["Da"], kind="dynamics")
    X, Y = R.build_windows(data, lookahead=2)
    x, y = next(iter(R.make_loader(X, Y, batch)))
    es = R.eps_stream(2, base["Z"])
    eps = torch.stack([es(t, (batch, base["Z"])) for t in range(2)])
    tr = helper_trainer(base, data, batch, device=DEV, extra={"lookahead": 2})
    tr.model.load_state_dict(sd)
    eng = tr.engine
    eng.set_joint_s_rec(True)
    for c in (_coeffs(s_rec_coeff=S_REC), ALONE):
        xk, yk, ek = _off_kinks(h, sd, x, y, eps, c)
        rows = xk.shape[0]
        want = R.loss_and_grads(h, sd, xk, yk, ek, False, coeff_cfg=c)
        assert any(k.startswith("_motor_decoder_helper") for k in want["grads"])
        eng.set_batch(xk, yk)
        eng.grads.fill_(float("nan"))
        before = _wm_state(eng)
        sp = make_step_params(lr=5e-4, adam_t=(1, 1, 1, 1, 1), a_rec=c["a_rec_coeff"], kl=c["vae_kl_coeff"], s_rec=c["s_rec_coeff"],
                              cyc=c["vae_cycle_coeff"], global_rows=rows)
        loss = eng.forward_backward(_lib.PHASE_JOINT, rows, sp, eps=ek, fused_adam=False).cpu()
        _check_terms(loss, want)
        _check_grads(eng, want)
        for a, b in zip(before, _wm_state(eng)):
            assert _same_bits(a, b)


def test_unrolled_term_with_an_input_subset():
    """task_encoder_inputs = ["task"], motor_decoder_inputs = ["body", "task"]: the predicted state reaches the decoder and
    both world-model passes, not the encoder."""
    arch = R.with_inputs(ARCH, ("task",), ("body", "task"))
    data, x, y, eps = _data(ARCH, 2)
    sd = R.perturb_biases(R.init_state_dict(arch, seed=1), seed=3)
    tr = make_trainer(arch, data, 64, device=DEV, extra={"lookahead": 2})
    tr.model.load_state_dict(sd)
    eng = tr.engine
    eng.set_joint_s_rec(True)
    for c in (_coeffs(s_rec_coeff=S_REC), ALONE):
        xk, yk, ek = _off_kinks(arch, sd, x[:33], y[:33], eps[:, :33], c)
        rows = xk.shape[0]
        want = R.loss_and_grads(arch, sd, xk, yk, ek, False, coeff_cfg=c)
        eng.set_batch(xk, yk)
        eng.grads.fill_(float("nan"))
        loss = eng.forward_backward(_lib.PHASE_JOINT, rows, _sp(rows, c), eps=ek, fused_adam=False).cpu()
        _check_terms(loss, want)
        _check_grads(eng, want)


# ------------------------------------------------------------------------------------------------ 5: evaluation
@pytest.mark.parametrize("L", [1, 2, 3])
def test_evaluation_returns_the_training_calls_forward(L):
    tr = _trainer(L)
    eng = tr.engine
    eng.set_joint_s_rec(True)
    _, x, y, eps = _data(ARCH, L)
    x, y, eps = x[:33], y[:33], eps[:, :33]
    tr.model.load_state_dict(R.perturb_biases(R.init_state_dict(ARCH, seed=1), seed=3))
    sp = _sp(33, _coeffs(s_rec_coeff=S_REC))
    eng.set_batch(x, y)
    train = eng.forward_backward(_lib.PHASE_JOINT, 33, sp, eps=eps, fused_adam=False).cpu().clone()
    eng.set_batch(x, y)
    ev = eng.forward_backward(_lib.PHASE_JOINT, 33, sp, eps=eps, backward=False).cpu().clone()
    assert float(ev[3]) > 0.0
    assert torch.equal(ev[2:], train[2:])                          # kl, s, cyc: the same launches write the same partials
    # (lookahead 1 forms the action term's partials in the seed epilogue when training and in its own kernel when not:
    #  another order of the same float32 sum)
    if L > 1:
        assert torch.equal(ev, train)
    else:
        assert torch.allclose(ev[:2], train[:2], rtol=1e-5, atol=0)
    # the backward plan of a joint step names the stacks it names without the term: no stage of the world model
    plan1 = eng.backward_plan(_lib.PHASE_JOINT, sp)
    plan0 = eng.backward_plan(_lib.PHASE_JOINT, _sp(33, _coeffs()))
    done = lambda plan: [(n, o, c) for n, o, c in plan if c > 0]
    assert done(plan1) == done(plan0) and all(n != _lib.NET_WM for n, _, c in plan1 if c > 0)
    if L == 1:
        assert plan1 == plan0


# ------------------------------------------------------------------------------------------------ 6: the trainer
@pytest.mark.parametrize("L", [1, 2])
def test_trainer_runs_the_key_through_both_phases(L):
    """`world_model_s_rec_coeff: 0.5` in the trainer's config: two world epochs, then two joint epochs, against the oracle's
    trainer loop (same minibatches, same draws).  Epoch losses within 2e-4 relative (test_gpu_helper_training.py's bound
    for fused steps against the oracle's graph + torch.optim.Adam)."""
    data = R.synth_demo(0, 3, 40, 7, 3, kind="dynamics")
    X, Y = R.build_windows(data, lookahead=L)
    sd = R.perturb_biases(R.init_state_dict(ARCH, seed=1), seed=3)
    es = R.eps_stream(2, ARCH["Z"])
    ref = R.RefTrainer(ARCH, sd, X, Y, 32, max_iter_world_model=2, coeff_cfg={"s_rec_coeff": S_REC}, eps_fn=es)
    tr = make_trainer(ARCH, data, 32, m_world=2, device=DEV, eps_fn=es, extra={"lookahead": L, "world_model_s_rec_coeff": S_REC})
    tr.model.load_state_dict(sd)
    for epoch in range(4):
        want = ref.step()["mean_train_loss"]
        got = tr.train()["mean_train_loss"]
        print("lookahead %d epoch %d: ours %.8g oracle %.8g" % (L, epoch, got, want))
        assert got == pytest.approx(want, rel=2e-4), epoch
        if epoch >= 2:
            assert tr.s_rec_coeff == S_REC and tr.last_loss_terms[3] > 0
            assert tr.last_loss_terms[3] == pytest.approx(ref.last_terms["loss_s"], rel=2e-4)
            assert tr.last_loss_terms[1] > 0                      # (and the joint phase's own terms are there)
    wm_ref = {k: v for k, v in ref.model.state_dict().items() if k.startswith("_world_model")}
    for k, v in wm_ref.items():
        assert max_err_scaled(tr.model.state_dict()[k].cpu(), v) < 2e-3, k
    # the test loop (run_epoch(train=False)) carries the term as well
    ev = tr.run_epoch(tr.train_loader, train=False)
    assert bool((ev[:, 3] > 0).all())
    assert torch.allclose(ev[:, 0], tr.a_rec_coeff * ev[:, 1] + tr.vae_kl_coeff * ev[:, 2] + S_REC * ev[:, 3] + tr.vae_cycle_coeff * ev[:, 4],
                          rtol=1e-5)


# ------------------------------------------------------------------------------------------------ 7: data parallel
WORKER = r'''
import os, sys, io, contextlib, torch
root = sys.argv[1]; out = sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from physicsvae_amd import parallel
rank, world, _ = parallel.init_from_env(backend="gloo")
from oracle import refpath as R
from util import make_trainer
arch = R.make_arch(7, 3, latent=4, te=(32, 2), md=(32, 2), wm=(32, 2))
data = R.synth_demo(0, 3, 40, 7, 3, kind="dynamics")            # 114 windows of 2 steps
with contextlib.redirect_stdout(io.StringIO()):
    tr = make_trainer(arch, data, int(sys.argv[3]), m_world=0, device="cuda:0", eps_fn=R.eps_stream(2, 4),
                      extra={"lookahead": 2, "world_model_s_rec_coeff": 0.5})
tr.model.load_state_dict(R.perturb_biases(R.init_state_dict(arch, 1), 3))
losses, terms = [], []
for _ in range(2):
    losses.append(tr.train()["mean_train_loss"])
    terms.append(tr.last_loss_terms)
sd = {k: v.cpu() for k, v in tr.model.state_dict().items()}
torch.save({"sd": sd, "losses": losses, "terms": terms, "steps": dict(tr.optimizer.net_steps)}, out + ".%d" % rank)
if world > 1:
    torch.distributed.barrier()
print("DONE", rank, losses)
'''


def _run(tmp_path, world, per_gpu, tag):
    script = tmp_path / "srec_dp_worker.py"
    script.write_text(WORKER)
    out = str(tmp_path / tag)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", WORLD_SIZE=str(world), PVAE_DP_EXCHANGE="default")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, out, str(per_gpu)], env=dict(env, RANK=str(r), LOCAL_RANK="0"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [torch.load(out + ".%d" % r) for r in range(world)]


def test_two_ranks_equal_one_process_with_the_global_batch(tmp_path):
    """Joint phase from the first epoch, lookahead 2, two ranks x 16 rows on the gloo transport: global batch 32, ragged
    tail 114 % 32 = 18 (16 + 2 rows)."""
    a, b = _run(tmp_path, 2, 16, "dp")
    single = _run(tmp_path, 1, 32, "single")[0]
    for k in a["sd"]:
        assert torch.equal(a["sd"][k], b["sd"][k]), k               # replicas stay bit-identical
    assert a["steps"] == single["steps"] and a["steps"].get(_lib.NET_WM, 0) == 0
    assert a["losses"] == pytest.approx(single["losses"], rel=1e-5)
    for e in range(2):
        assert a["terms"][e] == pytest.approx(single["terms"][e], rel=1e-5) and a["terms"][e][3] > 0
    for k, v in single["sd"].items():
        if k.startswith("_world_model"):
            assert torch.equal(a["sd"][k], v), k                    # frozen in every process
