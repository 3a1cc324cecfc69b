"""What tests/test_gpu_fc_shapes.py claims, checked without a GPU: every case of tests/fc_cases.py meets its drop cap and
its coverage conditions; the cases reach every class of the tile selectors of pvae_gemm_launch.h (restated in
tile_rules.py: whoever retunes a selector learns from this file that the sweep must follow); the float32 torch restatement of every computation stays
within ONE QUARTER of the bound the GPU test asserts against the float64 twin, so the standing bounds (outputs and stats
1e-5, gradients 1e-4, GAE columns 1e-5) carry over from the reference's own error alone; and the twin agrees with the
`Twin` of tests/test_gpu_fcnn.py, the oracle already trusted."""
import numpy as np
import pytest
import torch

import fc_cases as F
from physicsvae_amd import ppo as P
from physicsvae_amd.spaces import Box
from ppo_cases import KINK, coverage
from test_gpu_fcnn import Twin
from test_gpu_gae import dense_case, dense_want
from test_gpu_ppo import check_stats
from tile_rules import dgrad_uses_16x16, forward_uses_16x16, wgrad_uses_32x32    # pvae_gemm_launch.h's selectors at the default options
from util import max_err_scaled

OUT_BOUND, GRAD_BOUND = 1e-5, 1e-4           # what the GPU test asserts; a float32 restatement must stay under a quarter


def test_every_stack_case_meets_its_drop_cap_and_the_mix_is_as_stated():
    cases = F.all_stack_cases()
    random = cases[:F.N_RANDOM]
    assert [c.name for c in cases] == F.STACK_CASE_IDS
    worst = max(c.dropped for c in cases)
    print("stack cases: largest dropped fraction %.4f" % worst)
    for c in cases:
        assert c.dropped <= F.STACK_DROP_CAP, (c.name, c.dropped)
        assert c.x.shape == (c.rows, c.n_in) and c.max_batch >= c.rows and 1 <= len(c.stacks) <= 4
        assert float(F.twin64(c, c.x).margin.min()) > F.RELU_MARGIN
    for c in random:
        assert c.rows in F.ROWS and c.n_in in F.N_INS
        for widths, acts, n_out in c.stacks:
            assert 1 <= len(widths) <= 4 and set(widths) <= set(F.WIDTHS) and set(acts) <= set(F.ACT_NAMES) and n_out in F.N_OUTS
    assert {c.rows for c in random} == set(F.ROWS)
    assert {a for c in random for _, acts, _ in c.stacks for a in acts} == set(F.ACT_NAMES)
    assert {len(c.stacks) for c in random} == {1, 2, 3, 4}
    assert 4 * sum(len(set(c.depths)) > 1 for c in random) >= len(random)
    assert sum(len(c.stacks) == 1 and c.stacks[0][2] == 1 for c in cases) >= 4               # fc_value_stack's shape
    gemv = [F.directed_case("gemv_%d" % r) for r in (1, 2, 3, 4)]
    assert [c.rows for c in gemv] == [1, 2, 3, 4] and all(len(set(c.depths)) == 3 and c.stacks == gemv[0].stacks for c in gemv)


def test_the_cases_reach_every_class_of_the_tile_selectors():
    reached = {}
    for c in F.all_stack_cases():
        classes = set()
        if c.rows <= 4:
            classes.add("gemv R=%d" % (c.rows if c.rows <= 2 else 4))
        fwd, dgrad, wgrad = F.layer_problems(c)
        if c.rows > 4:
            for which, m, n in fwd:
                classes.add("forward %s %s" % (which, "16x16" if forward_uses_16x16(m, n) else "32x32"))
        for m, k_in in dgrad:
            classes.add("dgrad %s" % ("16x16" if dgrad_uses_16x16(m, k_in) else "32x32"))
        for n, k_in, m in wgrad:
            if wgrad_uses_32x32(n, k_in, m):
                classes.add("wgrad narrow")
            else:
                classes.add("wgrad wide by rows" if m % 64 else "wgrad wide by size")
        for k in classes:
            reached.setdefault(k, []).append(c.name)
    print({k: len(v) for k, v in sorted(reached.items())})
    want = ["forward first 16x16", "forward first 32x32", "forward deep 16x16", "forward deep 32x32", "dgrad 16x16", "dgrad 32x32",
            "wgrad narrow", "wgrad wide by rows", "wgrad wide by size", "gemv R=1", "gemv R=2", "gemv R=4"]
    assert set(reached) == set(want)
    for k in want:
        assert len(reached[k]) >= 3, (k, reached[k])
    # the directed cases are where their comments say
    for name in ("concat32_a", "concat32_b", "concat32_c"):
        assert name in reached["forward first 32x32"]
    for name in ("deep32_a", "deep32_b", "deep32_c"):
        assert name in reached["forward deep 32x32"] and name in reached["dgrad 32x32"]
    for name in ("wide_by_size_a", "wide_by_size_b", "wide_by_size_c"):
        assert name in reached["wgrad wide by size"]
    for name in ("wide_by_rows_31", "wide_by_rows_32", "wide_by_rows_130"):
        assert name in reached["wgrad wide by rows"]
    assert {F.directed_case("gemv_3").rows, F.directed_case("gemv_4").rows} == {3, 4}        # both through R = 4


def test_float32_restatement_of_every_stack_case_is_within_a_quarter_of_the_bound():
    worst = [0.0, 0.0]
    for c in F.all_stack_cases():
        w64, w32 = F.twin64(c, c.x, c.dys), F.twin64(c, c.x, c.dys, dtype=torch.float32)
        e_out = max(max_err_scaled(a, b) for a, b in zip(w32.outs, w64.outs))
        e_grad = max([max_err_scaled(w32.dx, w64.dx)] + [max_err_scaled(a, b) for l32, l64 in zip(w32.grads, w64.grads)
                                                          for p32, p64 in zip(l32, l64) for a, b in zip(p32, p64)])
        worst = [max(worst[0], e_out), max(worst[1], e_grad)]
        assert e_out <= OUT_BOUND / 4 and e_grad <= GRAD_BOUND / 4, (c.name, e_out, e_grad)
    print("float32 restatement of the stack cases: outputs %.3g, gradients %.3g" % tuple(worst))


def test_every_ppo_step_case_meets_its_caps_and_coverage():
    cases = [F.ppo_step_case(seed, kind) for seed, kind in F.PPO_CASE_IDS]
    print("PPO step cases: largest dropped fraction %.4f" % max(c.dropped for c in cases))
    for c in cases:
        assert c.dropped <= F.PPO_DROP_CAP, (c.name, c.dropped)
        assert c.k in F.K_VALUES and c.rows in F.PPO_ROWS and c.max_batch >= c.rows
        assert [n for _, _, n in c.stacks] == [c.k, 1] + ([c.k] if c.kind == "state_dependent" else [])
        assert c.coverage["kink"] > KINK
        if c.rows >= 64:
            assert all(c.coverage[key] >= 0.10 for key in F.COVERAGE_KEYS), (c.name, c.coverage)
        assert (c.index is not None) == (c.first > 0) == bool(c.seed % 2)
        if c.index is not None:                                  # the minibatch is the used rows
            sel = c.index[c.first: c.first + c.rows].long()
            assert all(torch.equal(c.batch[key][sel], c.used[key]) for key in c.used)
    assert {c.k for c in cases} == set(F.K_VALUES) and {c.rows for c in cases} == set(F.PPO_ROWS)
    assert any(c.rows >= 64 for c in cases if c.kind == "state_independent")
    assert 2 * sum(c.index is not None for c in cases) == len(cases)
    for kind in F.KINDS:                                         # the train_mask cases sit on unequal depths
        assert all(len(set(F.ppo_step_case(seed, kind).depths)) > 1 for seed in range(4)), kind


def test_float32_restatement_of_every_ppo_step_is_within_a_quarter_of_the_bound():
    worst = [0.0, 0.0]
    for seed, kind in F.PPO_CASE_IDS:
        c = F.ppo_step_case(seed, kind)
        w64, w32 = F.step_twin(c), F.step_twin(c, dtype=torch.float32)
        check_stats(w32.stats[0], w64.stats[0], OUT_BOUND / 4, c.name)
        errs = [max_err_scaled(a, b) for l32, l64 in zip(w32.grads, w64.grads) for p32, p64 in zip(l32, l64) for a, b in zip(p32, p64)]
        if kind == "state_independent":
            errs.append(max_err_scaled(w32.ls_grad, w64.ls_grad))
        worst[1] = max(worst[1], max(errs))
        assert max(errs) <= GRAD_BOUND / 4, (c.name, max(errs))
    print("float32 restatement of the PPO steps: gradients %.3g" % worst[1])


@pytest.mark.parametrize("kind", F.KINDS)
def test_head_seeds_meet_the_coverage_assertions_and_float32_is_within_a_quarter(kind):
    assert set(F.HEAD_SEEDS) == {(k, kd) for k in F.HEAD_KS for kd in F.KINDS} | {(F.WAVE_CAP_K, F.WAVE_CAP_KIND)}
    for k in F.HEAD_KS:
        cur, batch, cfg = F.head_case(k, kind)
        cov = coverage(cur, batch, cfg)
        assert F.head_covered(cov), (k, kind, cov)
        for rows, with_index, idx in F.head_runs(k, kind):
            a, b = F.head_twin(k, kind, idx, torch.float32), F.head_twin(k, kind, idx)
            check_stats(a[0], b[0], OUT_BOUND / 4, (k, kind, rows, with_index))
            e = [max_err_scaled(x, y) for x, y in zip(a[1:], b[1:])]
            print(k, kind, rows, with_index, "float32 restatement: d_mean %.3g d_value %.3g d_log_std %.3g" % tuple(e))
            assert max(e) <= GRAD_BOUND / 4


def test_wave_cap_case_is_covered_and_its_float32_restatement_is_within_a_quarter():
    k, kind = F.WAVE_CAP_K, F.WAVE_CAP_KIND
    assert F.head_covered(coverage(*F.head_case(k, kind)))
    for rows in F.WAVE_CAP_ROWS:
        assert rows > 2 * 4096                                     # ppo_head_kernel: 4096 waves at most, two rows each
        idx = F.wave_cap_index(rows)
        assert idx.numel() == rows and int(idx.max()) < F.HEAD_ROWS and idx.unique().numel() == F.HEAD_ROWS
        a, b = F.head_twin(k, kind, idx, torch.float32), F.head_twin(k, kind, idx)
        check_stats(a[0], b[0], OUT_BOUND / 4, (k, kind, rows))
        assert max(max_err_scaled(x, y) for x, y in zip(a[1:], b[1:])) <= GRAD_BOUND / 4


@pytest.mark.parametrize("table", ["many_segments", "many_rows"])
def test_gae_tables_and_their_float32_restatement(table):
    lengths, done = getattr(F, table)()
    n = sum(lengths)
    if table == "many_segments":
        assert len(lengths) == 4200 and n == 8736 and lengths[1000] == 200 and lengths[4150] == 131
        assert all(1 <= v <= 3 for i, v in enumerate(lengths) if i not in (1000, 4150))
    else:
        assert len(lengths) == 2100 and n > 262144 and 1 <= min(lengths) and max(lengths) <= 300
    assert 0.2 < sum(done) / len(done) < 0.8
    rewards, vf, last, seg_start, seg_done = dense_case(lengths, done)
    last0 = last * (1 - seg_done.float())
    for gamma, lambda_ in ((0.98, 0.95), (1.0, 1.0), (0.9, 0.0)):
        want_adv, want_vt, want_std = dense_want(gamma, lambda_, lengths, done)
        adv, vt = P.gae_torch(rewards, vf, last0, seg_start, gamma, lambda_)
        e = (max_err_scaled(adv, want_adv), max_err_scaled(vt, want_vt), max_err_scaled(P.standardize_torch(adv), want_std))
        print(table, n, "rows, gamma %g lambda %g: float32 restatement adv %.3g value_targets %.3g standardised %.3g" % ((gamma, lambda_) + e))
        assert max(e) <= OUT_BOUND / 4


def test_twin64_agrees_with_the_twin_of_the_fcnn_tests():
    """One default-configuration policy (256x2 tanh / 64x2 ... stacks as FullyConnectedPolicy builds them): its weights
    into a case, `twin64` in float32 against `Twin`, the nn.Linear restatement the fcnn tests trust."""
    from physicsvae_amd import FullyConnectedPolicy
    torch.manual_seed(3)
    cmc = {"log_std_type": "state_dependent", "sample_std": 0.6, "device": "cpu"}
    m = FullyConnectedPolicy(Box(np.zeros(22), np.zeros(22)), Box(np.zeros(5), np.zeros(5)), 10, {"custom_model_config": cmc}, "fcnn")
    twin = Twin(m, cmc)
    cfg = dict(FullyConnectedPolicy.DEFAULT_CONFIG)
    stacks, params = [], []
    for key, seq in (("policy_fn_layers", twin.pol), ("value_fn_layers", twin.val), ("log_std_fn_layers", twin.ls)):
        lins = [x for x in seq if isinstance(x, torch.nn.Linear)]
        hidden = cfg[key][:len(lins) - 1]
        stacks.append((tuple(l["hidden_size"] for l in hidden), tuple(l["activation"] or "linear" for l in hidden), lins[-1].out_features))
        params.append([(l.weight.detach().clone(), l.bias.detach().clone()) for l in lins])
    case = F.types.SimpleNamespace(stacks=tuple(stacks), params=params)
    x = torch.randn(40, 22, generator=torch.Generator().manual_seed(1))
    c1, c2 = torch.randn(40, 10, generator=torch.Generator().manual_seed(2)), torch.randn(40, generator=torch.Generator().manual_seed(3))
    xr = x.clone().requires_grad_(True)
    logits = twin(xr)
    ((logits * c1).sum() + (twin.cur_value * c2).sum()).backward()
    got = F.twin64(case, x, [c1[:, :5], c2.reshape(40, 1), c1[:, 5:]], dtype=torch.float32)
    assert max_err_scaled(got.outs[0], logits[:, :5].detach()) <= 1e-6
    assert max_err_scaled(twin.base + got.outs[2], logits[:, 5:].detach()) <= 1e-6
    assert max_err_scaled(got.outs[1].squeeze(1), twin.cur_value.detach()) <= 1e-6
    assert max_err_scaled(got.dx, xr.grad) <= 1e-5
    for seq, layers in zip((twin.pol, twin.val, twin.ls), got.grads):
        lins = [l for l in seq if isinstance(l, torch.nn.Linear)]
        assert len(lins) == len(layers)
        for lin, (gw, gb) in zip(lins, layers):
            assert max_err_scaled(gw, lin.weight.grad) <= 1e-5 and max_err_scaled(gb, lin.bias.grad) <= 1e-5
