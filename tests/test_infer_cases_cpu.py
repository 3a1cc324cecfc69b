"""What tests/test_gpu_infer_shapes.py claims, checked without a GPU: the mix of shapes of tests/infer_cases.py is the one
stated; every directed case reaches the path it is there for, by the host's own tile rules (tests/tile_rules.py) and layout
arithmetic (`pvae_layer`, which needs no GPU); the float32 twin of every case stays within ONE QUARTER of every bound the GPU
file asserts against the float64 twin (rollout values 2e-5, the value 1e-4, autograd forward values 1e-5, gradients 1e-4), so
those bounds rest on the reference's own error alone; no compared gradient tensor is all-zero by accident; every pool meets
its drop cap; at most one case in eight was replaced; the twin agrees with the oracle's restatement of PhysicsVAE
(oracle/refpath.py RefModel, itself pinned to captures of the reference) on every prior kind, on input subsets and on the
helper; and the twin's hand-written sampler backward is torch autograd's.

Run time on the development machine: 12 s for the file (8 s of it the float32 twins of all 42 cases at every row count),
against 10 s for tests/test_vae_ppo_cases_cpu.py."""
import pytest
import torch

import infer_cases as I
import tile_rules as T
from oracle import refpath as R
from physicsvae_amd import _lib
from ppo_cases import KINK
from util import max_err_scaled

CASES = I.CASE_IDS


def pad32(n):
    return (n + 31) // 32 * 32


def pad64(n):
    return (n + 63) // 64 * 64


def layers_of(c, net):
    return [l for l in I.module_for(c, "cpu").engine.layers if l["net"] == net]


def test_the_mix_is_as_stated():
    cases = I.all_cases()
    random = cases[:I.N_RANDOM]
    assert [c.name for c in cases] == CASES and len(random) == I.N_RANDOM == 32 and len(cases) == 42
    for i, c in enumerate(random):
        assert c.Db in I.DBS and c.Da in I.DAS and c.Z in I.ZS and c.mh is None
        assert c.prior == I.PRIOR_KINDS[i % 4] and c.noise == I.NOISE_MODES[i % 3] and c.max_batch == I.MAX_BATCHES[(i // 3) % 3]
        assert (c.pr is not None) == (c.prior == I.STATE_MEAN)
        for key in ("te", "md", "wm", "vb") + (("pr",) if c.pr else ()):
            widths, acts = getattr(c, key)
            assert 1 <= len(widths) <= 4 and set(widths) <= set(I.WIDTHS) and set(acts) <= set(I.ACT_NAMES)
    arena = lambda c: [getattr(c, key) for key in ("te", "md", "wm", "pr") if getattr(c, key) is not None]      # noqa: E731
    assert {c.Db for c in random} == set(I.DBS) and {c.Da for c in random} == set(I.DAS) and {c.Z for c in random} == set(I.ZS)
    assert {w for c in random for widths, _ in arena(c) for w in widths} == set(I.WIDTHS)
    assert {a for c in random for _, acts in arena(c) for a in acts} == set(I.ACT_NAMES)
    assert {len(widths) for c in random for widths, _ in arena(c)} == {1, 2, 3, 4}
    assert {c.prior for c in random} == set(I.PRIOR_KINDS) and {c.noise for c in random} == set(I.NOISE_MODES)
    assert {(c.te_inputs, c.md_inputs) for c in random} == set(I.PAIRS) and len(I.PAIRS) == 9
    assert {c.log_std_type for c in random} == set(I.LOG_STD_TYPES) and {c.max_batch for c in random} == set(I.MAX_BATCHES)
    # every prior kind meets every noise mode, and a state-independent log-std meets both parities of the index
    assert {(c.prior, c.noise) for c in random} == {(p, n) for p in I.PRIOR_KINDS for n in I.NOISE_MODES}
    assert {(c.log_std_type, i % 2) for i, c in enumerate(random)} == {(k, p) for k in I.LOG_STD_TYPES for p in (0, 1)}
    # the row counts: every listed one runs on some case; a case's rollout rows stop at its max_batch
    assert {r for c in cases for r in I.rollout_rows(c)} == set(I.ROLLOUT_ROWS) | {32}
    assert all(max(I.rollout_rows(c)) == min(33, c.max_batch) and I.rollout_rows(c)[:5] == (1, 2, 3, 4, 5) for c in cases)
    assert all(set(I.AUTOGRAD_ROWS) <= set(I.autograd_rows(c)) for c in cases)
    assert I.autograd_rows(I.case("chunk64"))[-2:] == (128, 131) and {33, 65, 97} <= set(I.autograd_rows(I.case("chunk32")))
    for c in cases:
        need = max(I.autograd_rows(c))
        assert c.obs.shape == (need, 2 * c.Db) and c.eps.shape == (need, c.Z) and c.dz.shape == (need, c.Z)
        assert set(c.dy) == set(I.nets_of(c)) and all(c.dy[key].shape == (need, I.out_width(c, key)) for key in c.dy)
        assert I.relu_units(I.shape_of(c.name)) <= (I.RELU_BUDGET if c.name.startswith("random") else 64) + (17 if c.mh is not None else 0)
    assert 4 * sum(I.relu_units(I.shape_of(c.name)) > 0 for c in cases) >= 3 * len(cases) and len({a for c in cases for a in c.te[1] + c.md[1] + c.wm[1]}) == 5
    # the rollout server's cases: priors it serves
    assert len(I.SERVER_CASES) == 6 and all(I.case(n).prior != I.SPHERE for n in I.SERVER_CASES)
    assert {I.case(n).prior for n in I.SERVER_CASES} == {I.ZERO_MEAN, I.STATE_MEAN, False}


def test_every_directed_case_reaches_its_path():
    d = {name: I.case(name) for name in I.DIRECTED}
    # wide_k: the second layer of every stack reads more than 1024 columns -- gemv_rollout_kernel's tail loop iterates
    for net in (_lib.NET_TE, _lib.NET_MD, _lib.NET_WM):
        lays = layers_of(d["wide_k"], net)
        assert lays[1]["ld"] == 1088 > 1024 and lays[1]["n_out"] == 64 and lays[0]["ld"] <= 64
    # wide_obs: the encoder's first layer does, and input kinds 2 / 3 take Ka = 520 columns of the observation
    assert layers_of(d["wide_obs"], _lib.NET_TE)[0]["ld"] == 1088 and d["wide_obs"].Db == 520
    assert layers_of(d["wide_obs"], _lib.NET_MD)[0]["ld"] == pad64(520 + 8) and layers_of(d["wide_obs"], _lib.NET_WM)[0]["ld"] == pad64(520 + 5)
    c = d["ones"]
    assert (c.Db, c.Da, c.Z) == (1, 1, 1) and all(getattr(c, key)[0] == (5,) for key in ("te", "md", "wm"))
    # z130: sampler_bwd_kernel's 64-lane loops make two passes and a bit, under the three kinds of backward
    assert [d["z130_" + k].prior for k in ("zero_mean", "hypersphere", "none")] == [I.ZERO_MEAN, I.SPHERE, False]
    assert all(d["z130_" + k].Z == 130 and 2 * 64 < 130 < 3 * 64 for k in ("zero_mean", "hypersphere", "none"))
    # helper: no fused rollout, so rows <= 4 take the staged path; net_seed_kernel's tanh at a padded width of 128
    c = d["helper"]
    eng = I.module_for(c, "cpu").engine
    assert eng.arch.mh is not None and not eng.fused_rollout and c.mh == ((17, 33), ("relu", "tanh")) and c.Db not in (7,)
    mh = layers_of(c, _lib.NET_MH)
    assert mh[-1]["act"] == _lib.LAYER_ACTS["tanh"] and mh[-1]["n_out"] == c.Da == 65 and mh[-1]["n_out_pad"] == 128
    # pair32: 97 rows pad to 128; 128 x 1024 puts the backward pairs, the forward and the input gradients on 32x32 tiles
    c = d["pair32"]
    assert pad32(97) == 128 == c.max_batch and T.plan_tiles("pair", 128, 1024)[0] == "32x32"
    assert T.plan_tiles("forward", 128, 1024)[0] == "32x32" and T.plan_tiles("dgrad", 128, 1024)[0] == "32x32"
    assert all(l["n_out_pad"] == 1024 for net in (0, 1, 2) for l in layers_of(c, net)[:2])
    # the other cases stay on 16x16 tiles at 33 rows, as the tiny model: pair32 is what adds the geometry
    assert T.plan_tiles("pair", 64, 320)[0] == "16x16"
    # chunk64: chunks of 64 rows accumulate on 32x32 weight-gradient tiles, the 3-row tail of 131 is a GEMV forward
    # chunk32: chunks of 32 rows accumulate on 64x64 tiles, the tails of 33 / 65 / 97 are one row
    from physicsvae_amd.autograd import chunks
    for name, geometry, tails in (("chunk64", 1, {128: 64, 131: 3}), ("chunk32", 0, {33: 1, 65: 1, 97: 1})):
        c = d[name]
        for rows, tail in tails.items():
            spans = chunks(rows, c.max_batch)
            assert len(spans) >= 2 and spans[-1][1] - spans[-1][0] == tail and spans[0][1] == c.max_batch
        for net in (_lib.NET_TE, _lib.NET_MD, _lib.NET_WM):
            for l in layers_of(c, net):
                assert T.plan_wgrad(l["n_out_pad"], l["ld"], pad32(c.max_batch))[0] == geometry, (name, net, l["index"])
                assert T.plan_wgrad(l["n_out_pad"], l["ld"], 32)[0] == 0            # the tail chunk: 32 padded rows


def test_float32_twin_is_within_a_quarter_of_every_bound_and_few_cases_were_replaced():
    worst = {key: (0.0, None) for key in I.QUARTER}
    dropped = []
    for name in CASES:
        c = I.case(name)
        e, zeros = I.twin32_errors(name)
        for key, bound in I.QUARTER.items():
            worst[key] = max(worst[key], (e[key], name))
            assert e[key] <= bound, (name, key, e[key], bound)
        assert not zeros, (name, zeros)
        assert c.dropped <= I.drop_cap(c), (name, c.dropped)
        dropped.append((c.dropped, name))
        # the margin holds on the rows as used: the forward under the case's draws and every stack at its rounded input
        out = I.twin(name, c.obs.shape[0])
        assert float(out.margin.min()) >= KINK
        p64 = I.leaves(c, torch.float64)
        assert all(float(I.run_stack(c, key, p64[key], out.x[key].double())[1].min()) >= KINK for key in I.nets_of(c))
    for key, (e, name) in worst.items():
        print("float32 twin, %-10s worst %.3g (%s)   a quarter of the bound %.3g" % (key, e, name, I.QUARTER[key]))
    print("largest dropped share %.3f (%s); cases with no ReLU on a gradient path: %d" % (max(dropped) + (sum(d == 0.0 for d, _ in dropped),)))
    print("replaced cases: %d of %d %s" % (len(I.RESEED), len(CASES), sorted(I.RESEED)))
    assert set(I.RESEED) <= set(CASES) and all(v > 0 for v in I.RESEED.values())
    assert 8 * len(I.RESEED) <= len(CASES)


@pytest.mark.parametrize("name", ["random0", "random1", "random2", "random3", "random7", "helper"])
def test_twin_agrees_with_the_oracles_restatement(name):
    """RefModel (float32) on the case's state dict against the float64 twin: the action, the prediction, the code, the
    value and the learned prior's mean at 1e-5, every gradient of the policy loss at 1e-4."""
    c = I.case(name)
    assert {"random0": c.prior == I.ZERO_MEAN and c.te_inputs == c.md_inputs == I.TASK, "random1": c.prior == I.STATE_MEAN and c.md_inputs == I.BODY,
            "random2": c.prior == I.SPHERE and c.te_inputs == I.BODY, "random3": c.prior is False, "random7": c.prior is False
            and c.te_inputs == I.TASK, "helper": c.mh is not None}[name]
    ref = R.RefModel(c.arch)
    ref.load_state_dict(c.sd)
    rows = 33
    obs, eps = c.obs[:rows], c.eps[:rows]
    noise = c.noise != "off"
    ref.eps_source = lambda shape: eps
    ref.latent_prior_noise = noise
    logits = ref(obs)
    want = I.policy_twin(c, obs, eps, noise)
    got = {"a": logits[:, :c.Da], "s2": ref.cur_future_state, "z": ref.cur_z, "value": ref.cur_value}
    if c.prior == I.STATE_MEAN:
        got["prior_mu"] = ref.cur_prior_mu
    e = {key: max_err_scaled(t.detach(), getattr(want.out, key).detach()) for key, t in got.items()}
    loss = (logits[:, :c.Da] ** 2).sum() + (ref.cur_future_state ** 2).sum()
    if c.prior == I.STATE_MEAN:
        loss = loss + (ref.cur_prior_mu ** 2).sum()
    loss.backward()
    assert abs(float(loss.detach()) - float(want.loss)) <= 1e-5 * abs(float(want.loss))
    e_grad = 0.0
    for key in I.nets_of(c):
        mod = getattr(ref, I.NET_KEYS[key])
        for i, pair in enumerate(want.grads[key]):
            lin = mod._model[i]._model[0]
            for p, g in zip((lin.weight, lin.bias), pair):
                if I.structurally_zero(c, key):
                    assert (p.grad is None or float(p.grad.abs().max()) == 0.0) and (g is None or float(g.abs().max()) == 0.0)
                    continue
                e_grad = max(e_grad, max_err_scaled(p.grad, g))
    print(name, {k: "%.3g" % v for k, v in e.items()}, "gradients %.3g" % e_grad)
    assert all(v < 1e-5 for v in e.values()) and e_grad < 1e-4


@pytest.mark.parametrize("prior", I.PRIOR_KINDS, ids=["zero_mean", "state_mean", "hypersphere", "none"])
def test_sampler_backward_is_autograd_of_the_sampler(prior):
    g = torch.Generator().manual_seed(11)
    for Z in (1, 3, 130):
        c = I.spec(4, 2, Z, I.T64, I.T64, I.T64, prior=prior)
        h = torch.randn(9, I.te_out(c), generator=g, dtype=torch.float64)
        eps, dz = (torch.randn(9, Z, generator=g, dtype=torch.float64) for _ in range(2))
        for noise in (True, False):
            hg = h.clone().requires_grad_(True)
            (I.sampler(c, hg, eps, noise) * dz).sum().backward()
            got = I.sampler_backward(c, h, eps, noise, dz)
            assert got.shape == h.shape
            assert float((got - hg.grad).abs().max()) <= 1e-13 * max(1.0, float(hg.grad.abs().max())), (prior, Z, noise)
            if prior in (I.ZERO_MEAN, I.STATE_MEAN) and not noise:
                assert float(got[:, Z:].abs().max()) == 0.0
