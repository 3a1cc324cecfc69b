"""What tests/test_gpu_ppo_vae_shapes.py claims, checked without a GPU: the twin of tests/vae_ppo_cases.py agrees with the
`Twin` of tests/test_gpu_ppo_vae.py and, on cases with input subsets and both priors, with the oracle's restatement of
PhysicsVAE (oracle/refpath.py RefModel, itself pinned to captures of the reference) on the state dict the module hands out;
every case meets its drop cap and, from 31 rows up, the coverage conditions; the mix of shapes is the one stated; the float32
twin of every case stays within ONE QUARTER of every bound the GPU file asserts against the float64 twin, so those bounds
(stats 2e-4, gradients 1e-4, moments 2e-4 / 4e-4, parameters 2e-3, evaluate columns 1e-5) rest on the reference's own error
alone; no trained gradient tensor is all-zero by accident; at most one case in eight was replaced; and the two grid-cap cases
cross their caps (the arithmetic of pvae_ppo.hip restated here: whoever changes a cap learns from this file that the sweep
must follow)."""
import pytest
import torch

import fc_cases as F
import vae_ppo_cases as V
from oracle import refpath as R
from ppo_cases import KINK
from test_gpu_ppo_vae import TINY, Twin, build
from util import max_err_scaled

CASES = V.CASE_IDS


def test_twin_agrees_with_the_twin_of_the_ppo_tests_on_tiny():
    m = build(TINY, device="cpu")
    old = Twin(m)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    c = V.spec(TINY["dim_body"], TINY["dim_action"], TINY["latent"], 40, 40, ((64,) * TINY["te"][1], ("relu",) * TINY["te"][1]),
               ((64,) * TINY["md"][1], ("relu",) * TINY["md"][1]), ((32,) * TINY["vb"][1], ("relu",) * TINY["vb"][1]))
    c.params = {net: [(sd["%s._model.%d._model.0.weight" % (net, i)], sd["%s._model.%d._model.0.bias" % (net, i)])
                      for i in range(len(st[0]) + 1)] for net, st in zip(V.NETS, (c.te, c.md, c.vb))}
    g = torch.Generator().manual_seed(3)
    obs, eps = torch.randn(40, 26, generator=g).double(), torch.randn(40, 3, generator=g).double()
    c1, c2 = torch.randn(40, 5, generator=g).double(), torch.randn(40, generator=g).double()
    params = V.leaves(c, torch.float64)
    mean, ls, value, _, _ = V.forward(c, params, m._als.log_std.double(), obs, eps)
    a, ls_old, v = old(obs, eps)
    ((mean * c1).sum() + (value * c2).sum()).backward()
    ((a * c1).sum() + (v * c2).sum()).backward()
    assert max_err_scaled(mean.detach(), a.detach()) < 1e-12 and max_err_scaled(value.detach(), v.detach()) < 1e-12
    assert torch.equal(ls, ls_old.detach())
    for net in V.NETS:
        for i, (w, b) in enumerate(params[net]):
            assert max_err_scaled(w.grad, old.by["%s._model.%d._model.0.weight" % (net, i)].grad) < 1e-12, (net, i)
            assert max_err_scaled(b.grad, old.by["%s._model.%d._model.0.bias" % (net, i)].grad) < 1e-12, (net, i)


@pytest.mark.parametrize("name", ["random2", "random0", "subsets_task_task_5"])
def test_twin_agrees_with_the_oracles_restatement_under_subsets_and_both_priors(name):
    """The case's weights go into `PhysicsVAE(device="cpu")` (keys and shapes must be the module's: a subset's first layer is
    as narrow as its window) and what the module's state dict hands out goes into RefModel, which runs in float32: 1e-5 on the
    mean and the value, as tests/test_ppo_vae_prepare_cpu.py holds the older twin."""
    c = V.case(name)
    assert {"random2": not c.prior and c.te_inputs == V.BODY, "random0": c.prior and not c.noise and c.md_inputs == V.TASK,
            "subsets_task_task_5": c.prior and c.noise and c.te_inputs == c.md_inputs == V.TASK}[name]
    m = V.module_for(c, "cpu")
    assert m.engine.arch.te_out == V.te_out(c) and m._ppo_train_mask() == c.mask
    pairs = lambda st: [(w, a) for w, a in zip(*st)]                                 # noqa: E731
    arch = R.with_inputs(R.make_arch(c.Db, c.Da, latent=c.Z, te=pairs(c.te), md=pairs(c.md), wm=[(8, "relu")], vb=pairs(c.vb),
                                     prior=c.prior), c.te_inputs, c.md_inputs)
    ref = R.RefModel(arch)
    missing, unexpected = ref.load_state_dict(m.state_dict(), strict=False)
    assert not missing and all(k.endswith("log_std") for k in unexpected), (missing, unexpected)
    ro, eps, want = V.rollout(name)
    ref.eps_source = lambda shape: eps
    ref.latent_prior_noise = c.noise
    with torch.no_grad():
        logits = ref(ro["obs"])
    e = (max_err_scaled(logits[:, :c.Da], want["old_dist"][:, :c.Da]), max_err_scaled(ref.cur_value, want["vf_preds"]))
    print(name, "mean %.3g value %.3g" % e)
    assert e[0] < 1e-5 and e[1] < 1e-5
    assert torch.equal(want["old_dist"][:, c.Da:], m._als.log_std.detach().double().reshape(1, -1).expand(len(eps), -1))


def test_every_case_meets_its_drop_cap_and_coverage():
    cases = V.all_cases()
    print("largest dropped fraction %.4f (%s)" % max((c.dropped, c.name) for c in cases))
    for c in cases:
        assert c.dropped <= (V.DROP_CAP if c.rows >= 5 else V.DROP_CAP_FEW_ROWS), (c.name, c.dropped)
        assert c.used["obs"].shape == (c.rows, 2 * c.Db) and c.eps.shape == (c.rows, c.Z) and c.max_batch >= c.rows
        assert c.coverage["kink"] > KINK and V.covered(c)
        if c.rows >= 31:
            assert all(c.coverage[key] >= 0.10 for key in F.COVERAGE_KEYS), (c.name, c.coverage)
        assert (c.index is not None) == (c.first > 0) == c.gathered
        if c.index is not None:                                  # the minibatch is the used rows
            sel = c.index[c.first: c.first + c.rows].long()
            assert all(torch.equal(c.batch[key][sel], c.used[key]) for key in c.used)
        with torch.no_grad():
            margin = V.forward(c, V.leaves(c, torch.float64, 0), c.ls_vec.double(), c.used["obs"].double(), c.eps.double())[3]
        assert float(margin.min()) > F.RELU_MARGIN
        assert c.rows <= 130 and max(c.te[0] + c.md[0] + c.vb[0]) <= 300          # (the sweep stays small)


def test_the_mix_is_as_stated():
    cases = V.all_cases()
    random = cases[:V.N_RANDOM]
    assert [c.name for c in cases] == V.CASE_IDS and len(random) == V.N_RANDOM == 40
    for i, c in enumerate(random):
        assert c.Db in V.DBS and c.Da in V.DAS and c.Z in V.ZS and c.rows == V.ROWS[i % len(V.ROWS)] and c.mask == 1 + i % 7
        assert c.max_batch - c.rows in (0, 1, 30) and c.gathered == bool(i % 2)
        for widths, acts in (c.te, c.md, c.vb):
            assert 1 <= len(widths) <= 4 and set(widths) <= set(F.WIDTHS) and set(acts) <= set(F.ACT_NAMES)
    assert {c.rows for c in random} == set(V.ROWS) and {c.mask for c in random} == set(range(1, 8))
    assert {a for c in random for _, acts in (c.te, c.md, c.vb) for a in acts} == set(F.ACT_NAMES)
    assert {c.prior for c in random} == {V.ZERO_MEAN, False} and 3 * sum(not c.prior for c in random) >= len(random) - 2
    assert 4 * sum(not c.noise for c in random) == len(random)
    assert {c.log_std_type for c in random} == {"constant", "state_independent"}
    assert 2 * sum(c.log_std_type == "constant" for c in random) == len(random)
    assert {(c.te_inputs, c.md_inputs) for c in random} == set(V.PAIRS)
    assert 4 * sum(len(set(c.depths)) > 1 for c in random) >= len(random)
    # noise off meets the zero-mean prior (the logvar half must then have no gradient) and a trained encoder
    assert any(c.prior and not c.noise and c.mask & 1 for c in random)
    for kind in ("constant", "state_independent"):
        assert {c.gathered for c in random if c.log_std_type == kind} == {True, False}
    d = {name: V.case(name) for name in V.DIRECTED}
    assert [d["masks_%d" % k].mask for k in range(1, 8)] == list(range(1, 8))
    assert [d["gemv_%d" % r].rows for r in range(1, 5)] == [1, 2, 3, 4]
    for group in ("masks_", "gemv_"):                             # one model each, of three unequal depths
        same = [c for name, c in d.items() if name.startswith(group)]
        assert all(len(set(c.depths)) == 3 for c in same)
        assert all(torch.equal(a, b) for c in same for net in V.NETS for pa, pb in zip(c.params[net], same[0].params[net])
                   for a, b in zip(pa, pb))
    assert d["decoder_body_only"].md_inputs == V.BODY and d["decoder_body_only"].mask == 7
    assert d["no_prior_odd"].prior is False and d["no_prior_odd"].Z == 33 and d["no_prior_odd"].log_std_type == "state_independent"
    assert d["noise_off"].prior == V.ZERO_MEAN and not d["noise_off"].noise and d["noise_off"].mask == 1
    for rows in (5, 64):
        assert (d["subsets_task_task_%d" % rows].te_inputs, d["subsets_task_task_%d" % rows].md_inputs) == (V.TASK, V.TASK)
        assert (d["subsets_body_task_%d" % rows].te_inputs, d["subsets_body_task_%d" % rows].md_inputs) == (V.BODY, V.TASK)
        assert d["subsets_body_task_%d" % rows].rows == rows
    for name in CASES:                                            # the rollouts: chunks of max_batch, max_batch and 1..4 rows
        ro, eps, _ = V.rollout(name)
        c, n = V.case(name), ro["obs"].shape[0]
        assert 1 <= n - 2 * c.max_batch <= 4 and eps.shape == (n, c.Z)
        s = ro["seg_done"].numel()
        assert s == min(5, n) and int(ro["seg_start"][-1]) == n and bool((ro["seg_start"][1:] > ro["seg_start"][:-1]).all())
        assert s < 3 or (bool(ro["seg_done"].any()) and not bool(ro["seg_done"].all()))


def test_float32_twin_is_within_a_quarter_of_every_bound_and_few_cases_were_replaced():
    worst = {key: (0.0, None) for key in V.QUARTER}
    for name in CASES:
        e = V.twin32_errors(name)
        for key, bound in V.QUARTER.items():
            worst[key] = max(worst[key], (e[key], name))
            assert e[key] <= bound, (name, key, e[key], bound)
        assert not V.zero_gradients(name), (name, V.zero_gradients(name))
    for key, (e, name) in worst.items():
        print("float32 twin, %-12s worst %.3g (%s)   a quarter of the bound %.3g" % (key, e, name, V.QUARTER[key]))
    print("replaced cases: %d of %d %s" % (len(V.RESEED), len(CASES), sorted(V.RESEED)))
    assert set(V.RESEED) <= set(CASES) and all(v > 0 for v in V.RESEED.values())
    assert 8 * len(V.RESEED) <= len(CASES)


def test_structural_zeros_of_the_twin_are_where_the_gpu_file_asserts_them():
    """The exact zeros the GPU file asserts are exact in the float64 twin too: the encoder's whole gradient under a decoder
    that reads the body alone, and the logvar half of the encoder's output layer with the noise off."""
    seen = [0, 0]
    for name in CASES:
        c = V.case(name)
        if not c.mask & 1:
            continue
        grads = V.step_twin(c).grads["_task_encoder"]
        if V.structurally_zero(c, "_task_encoder"):
            assert all(float(t.abs().max()) == 0.0 for pair in grads for t in pair), name
            seen[0] += 1
        elif c.prior and not c.noise:
            dw, db = grads[-1]
            assert float(dw[c.Z:].abs().max()) == 0.0 and float(db[c.Z:].abs().max()) == 0.0 and float(dw[:c.Z].abs().max()) > 0, name
            seen[1] += 1
    assert seen[0] >= 2 and seen[1] >= 2, seen


def pad32(n):
    return (n + 31) // 32 * 32


def pad64(n):
    return (n + 63) // 64 * 64


def copy_in_grid(c):                         # pvae_ppo.hip ppo_copy_in: gx = (rows_pad * ldmax + 255) / 256, capped at 256
    ldmax = max(pad64(2 * c.Db), pad64(c.Db + c.Z))      # the encoder's and the value stack's panel, the decoder's
    return (pad32(c.rows) * ldmax + 255) // 256


def sampler_bwd_grid(c):                     # pvae_ppo.hip ppo_grad_half: gx = (rows_pad * te_last.n_out_pad + 255) / 256, capped at 256
    return (pad32(c.rows) * pad64(V.te_out(c)) + 255) // 256


def test_the_grid_cap_cases_cross_their_caps():
    a, b = V.case("copy_in_loops"), V.case("sampler_bwd_loops")
    assert copy_in_grid(a) > 256 and a.mask == 7
    assert (pad32(a.rows) - 32) * pad64(2 * a.Db) <= 65536           # the smallest rows_pad at this width that loops
    assert sampler_bwd_grid(b) > 256 and b.prior == V.ZERO_MEAN and b.mask & 1 and b.rows == 97
    assert (pad32(b.rows) - 32) * pad64(V.te_out(b)) <= 65536
    # the padded widths restated above are the library's own
    for c in (a, b):
        layers = V.module_for(c, "cpu").engine.layers
        te = [l for l in layers if l["net"] == 0]
        md = [l for l in layers if l["net"] == 1]
        assert te[0]["ld"] == pad64(2 * c.Db) and md[0]["ld"] == pad64(c.Db + c.Z) and te[-1]["n_out_pad"] == pad64(V.te_out(c))
    crossing = [name for name in CASES if copy_in_grid(V.case(name)) > 256 or (V.case(name).mask & 1 and sampler_bwd_grid(V.case(name)) > 256)]
    print("cases past a grid cap:", crossing)
    assert set(crossing) >= {"copy_in_loops", "sampler_bwd_loops"}
