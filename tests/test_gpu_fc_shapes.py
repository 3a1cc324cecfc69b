"""Randomised-shape sweep of the stack set (pvae_fc.hip) and the PPO learner's launches (pvae_ppo_core.hip) against float64:
(a) the grouped forward / backward on random and directed stack sets -- unequal depths, per-layer widths and activations,
every tile geometry the selectors of pvae_gemm_launch.h choose, every GEMV instantiation; (b) the fused PPO step at action
counts K = 1 .. 130, few rows, every train_mask, and the SGD loop; (c) the loss head alone at K up to 200 and past its wave
cap; (d) GAE and the standardisation past their grid caps; (e) evaluate and prepare at K = 1 / 65 / 130 and in chunks
larger than the epilogue's and the copy's grids; (f) a stack without a hidden layer.  The cases come from
tests/fc_cases.py; tests/test_fc_cases_cpu.py checks without a GPU that they reach what is claimed here and that the
float32 restatement of each stays within a quarter of these bounds.

Bounds, the suite's standing ones, against a float64 oracle that reads the kernels' own float32 inputs: outputs and stats
1e-5 (the stats by `check_stats` of tests/test_gpu_ppo.py); gradients and dx 1e-4 by max_err_scaled; GAE columns,
vf_preds, old_dist and last_value 1e-5; old_logp 1e-5 max(1, |want|) per row.  Parameters and Adam's moments after three
steps: PARAM_BOUND and MOMENT_BOUNDS of tests/test_gpu_ppo.py."""
import types

import pytest
import torch

import fc_cases as F
from physicsvae_amd import engine as E
from physicsvae_amd import ppo as P
from physicsvae_amd.engine import Stack, StackSetEngine, make_ppo_batch, ppo_loss, set_fc_per_stack
from ppo_cases import coverage
from test_gpu_gae import SENTINEL, dense_want, guarded, guards_intact, logp_err, run_dense
from test_gpu_ppo import MOMENT_BOUNDS, PARAM_BOUND, arena_pads, check_stats, ls_grad_from_moment
from util import max_err_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUT_BOUND, GRAD_BOUND = 1e-5, 1e-4


@pytest.fixture(autouse=True)
def grouped_by_default():
    set_fc_per_stack(False)
    yield
    set_fc_per_stack(False)


def hidden(widths, acts):
    if widths:
        return Stack(widths, acts)
    st = Stack.__new__(Stack)                    # no hidden layer: past Stack's own check, as a raw pvae_fc_config allows
    st.widths, st.acts = (), ()
    return st


def engine_for(case):
    """The stack set of a case, holding its weights; `.m` is what the helpers of test_gpu_ppo.py take (an object with .engine)."""
    eng = StackSetEngine(case.n_in, [(hidden(w, a), n) for w, a, n in case.stacks], case.max_batch, device=DEV)
    for s, layers in enumerate(case.params):
        for (w, b), (w0, b0) in zip(eng.views(s), layers):
            w.copy_(w0.to(DEV))
            b.copy_(b0.to(DEV))
    eng.m = types.SimpleNamespace(engine=eng)
    return eng


def stack_span(eng, s):
    """[(offset, floats)] of stack s in a buffer of the arena's layout, pads included."""
    return [span for l in eng.stack_layers(s) for span in ((l["w_offset"], l["n_out_pad"] * l["ld"]), (l["b_offset"], l["n_out_pad"]))]


def grad_errors(eng, arena, want_grads, stacks):
    return [max_err_scaled(got.cpu(), want) for s in stacks
            for pair, wpair in zip(eng.views(s, arena), want_grads[s]) for got, want in zip(pair, wpair)]


# ---------------------------------------------------------------------------------------
# (a) stack-set forward and backward
# ---------------------------------------------------------------------------------------
def run_all(eng, x, dys, full):
    """forward, store-mode backward and accumulate over ones, each on a workspace full of NaN."""
    nan = float("nan")
    eng.workspace.fill_(nan)
    outs = eng.forward(x)
    eng.workspace.fill_(nan)
    grad = torch.full((eng.arena_floats,), nan, device=DEV)
    dx = eng.backward(x, dys, True, grad, grad_mask=full)
    eng.workspace.fill_(nan)
    acc = torch.ones(eng.arena_floats, device=DEV)
    eng.backward(x, dys, False, acc, grad_mask=full, accumulate=True)
    return outs, dx, grad, acc


@pytest.mark.parametrize("name", F.STACK_CASE_IDS)
def test_stack_set_matches_the_float64_twin(name):
    c = F.stack_case_by_id(name)
    eng = engine_for(c)
    S, full = len(c.stacks), (1 << len(c.stacks)) - 1
    g = torch.Generator().manual_seed(c.seed)
    flip = lambda: bool(torch.randint(2, (1,), generator=g))                         # noqa: E731
    x, dys = c.x.to(DEV), [d.to(DEV) for d in c.dys]
    want = F.twin64(c, c.x, c.dys)
    outs, dx, grad, acc = run_all(eng, x, dys, full)
    # forward: all stacks, and one random subset
    e_out = max(max_err_scaled(o.cpu(), w) for o, w in zip(outs, want.outs))
    sub = [flip() for _ in range(S)]
    sub[int(torch.randint(S, (1,), generator=g))] = True
    eng.workspace.fill_(float("nan"))
    part = eng.forward(x, want=sub)
    assert all((p is not None) == w for p, w in zip(part, sub))
    e_sub = max(max_err_scaled(p.cpu(), w) for p, w in zip(part, want.outs) if p is not None)
    # backward, store mode
    e_dx = max_err_scaled(dx.cpu(), want.dx)
    e_grad = max(grad_errors(eng, grad, want.grads, range(S)))
    print(name, c.stacks, "rows", c.rows, "outputs %.3g subset %s %.3g dx %.3g gradients %.3g" % (e_out, sub, e_sub, e_dx, e_grad))
    assert e_out <= OUT_BOUND and e_sub <= OUT_BOUND and e_dx <= GRAD_BOUND and e_grad <= GRAD_BOUND
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(dx).all()) and all(bool(torch.isfinite(o).all()) for o in outs)
    assert float(arena_pads(eng.m, grad).abs().max()) == 0.0                         # every pad entry exactly zero
    # accumulate: read-add-write of the same tile sums
    assert torch.equal(acc, grad + 1.0)
    # backward of a proper subset: some stacks without an output gradient, some not trained, dx wanted or not
    ran = [flip() for _ in range(S)]
    ran[int(torch.randint(S, (1,), generator=g))] = True
    if S > 1 and all(ran):
        ran[int(torch.randint(S, (1,), generator=g))] = False
    want_dx = flip()
    mask = [flip() for _ in range(S)]
    if not want_dx and not any(r and m for r, m in zip(ran, mask)):
        mask[ran.index(True)] = True
    if S == 1 and want_dx:
        mask = [False]                                                                # (one stack: dx alone is its proper subset)
    runs = [r and (want_dx or m) for r, m in zip(ran, mask)]                          # has a gradient and a consumer
    trained = [r and m for r, m in zip(ran, mask)]
    wsub = F.twin64(c, c.x, [d if r else None for d, r in zip(c.dys, runs)])
    eng.workspace.fill_(float("nan"))
    buf = torch.full((eng.arena_floats,), SENTINEL, device=DEV)
    dxs = eng.backward(x, [d if r else None for d, r in zip(dys, ran)], want_dx, buf, grad_mask=sum(1 << s for s in range(S) if mask[s]))
    errs = grad_errors(eng, buf, wsub.grads, [s for s in range(S) if trained[s]])
    if want_dx:
        errs.append(max_err_scaled(dxs.cpu(), wsub.dx))                               # the sum over the stacks that ran
    else:
        assert dxs is None
    print(name, "subset: ran", ran, "mask", mask, "want_dx", want_dx, "largest error %.3g" % max(errs + [0.0]))
    assert all(e <= GRAD_BOUND for e in errs)
    for s in range(S):
        for off, n in stack_span(eng, s):
            blk = buf[off: off + n]
            if trained[s]:
                assert bool(torch.isfinite(blk).all()) and not bool((blk == SENTINEL).any()), (s, off)
            else:
                assert bool((blk == SENTINEL).all()), (s, off)                        # untouched
    # both schedules at the directed shapes: the same bits, now at shapes where both are also compared with the twin
    if name in F.DIRECTED:
        set_fc_per_stack(True)
        outs2, dx2, grad2, acc2 = run_all(eng, x, dys, full)
        assert all(torch.equal(a, b) for a, b in zip(outs, outs2))
        assert torch.equal(dx, dx2) and torch.equal(grad, grad2) and torch.equal(acc, acc2)


# ---------------------------------------------------------------------------------------
# (b) the fused PPO step
# ---------------------------------------------------------------------------------------
CFG = P.PPOConfig(lr=1e-4, **F.LOSS)


def bound_engine(c):
    eng = engine_for(c)
    ls = None if c.kind == "state_dependent" else c.ls_vec.to(DEV).clone()
    eng.ppo_bind(ls, c.kind == "state_independent")
    eng.ls = ls
    index = c.index.to(DEV) if c.index is not None else None
    return eng, eng.ppo_batch({k: v.to(DEV) for k, v in c.batch.items()}), index


def step_params(c, t, mask=0):
    return CFG.params(c.kind, F.LS_BASE if c.kind == "state_dependent" else 0.0, adam_t=t, train_mask=mask)


def dirty(eng):
    for buf in (eng.workspace, eng.ppo_scratch, eng.ppo_grad):
        buf.fill_(float("nan"))


@pytest.mark.parametrize("seed,kind", F.PPO_CASE_IDS)
def test_fused_ppo_step_matches_the_float64_twin(seed, kind):
    c = F.ppo_step_case(seed, kind)
    eng, batch, index = bound_engine(c)
    S = len(c.stacks)
    want = F.step_twin(c, steps=3, lr=CFG.lr)
    dirty(eng)
    stats = eng.ppo_step(batch, step_params(c, 1), c.first, c.rows, index).cpu()
    print(c.name, "K", c.k, "rows", c.rows, c.stacks, "index" if index is not None else "in order")
    check_stats(stats, want.stats[0], OUT_BOUND, c.name)
    errs = grad_errors(eng, eng.ppo_grad, want.grads, range(S))
    if kind == "state_independent":
        errs.append(max_err_scaled(ls_grad_from_moment(eng.m), want.ls_grad))
    print(c.name, "largest gradient error %.3g" % max(errs))
    assert max(errs) <= GRAD_BOUND
    for arena in (eng.ppo_grad, eng.ppo_m, eng.ppo_v, eng.params):
        assert float(arena_pads(eng.m, arena).abs().max()) == 0.0 and bool(torch.isfinite(arena).all())
    for t in (2, 3):
        stats = eng.ppo_step(batch, step_params(c, t), c.first, c.rows, index)
    assert bool(torch.isfinite(stats).all())
    e_p, e_m, e_v = [], [], []
    for s in range(S):
        for i, (pair, wpair) in enumerate(zip(eng.views(s), want.params[s])):
            mom = (eng.views(s, eng.ppo_m)[i], eng.views(s, eng.ppo_v)[i])
            for j, (got, leaf) in enumerate(zip(pair, wpair)):
                state = want.opt.state[leaf]
                e_p.append(max_err_scaled(got.cpu(), leaf.detach()))
                e_m.append(max_err_scaled(mom[0][j].cpu(), state["exp_avg"]))
                e_v.append(max_err_scaled(mom[1][j].cpu(), state["exp_avg_sq"]))
    if kind == "state_independent":
        state = want.opt.state[want.ls_vec]
        e_p.append(max_err_scaled(eng.ls.cpu(), want.ls_vec.detach()))
        e_m.append(max_err_scaled(eng.ppo_ls_m.cpu(), state["exp_avg"]))
        e_v.append(max_err_scaled(eng.ppo_ls_v.cpu(), state["exp_avg_sq"]))
    print(c.name, "after three steps: parameters %.3g m %.3g v %.3g" % (max(e_p), max(e_m), max(e_v)))
    assert max(e_p) < PARAM_BOUND and max(e_m) < MOMENT_BOUNDS[0] and max(e_v) < MOMENT_BOUNDS[1]
    assert float(arena_pads(eng.m, eng.params).abs().max()) == 0.0


@pytest.mark.parametrize("kind", F.KINDS)
def test_every_train_mask_on_unequal_depths(kind):
    """Every proper subset of the stacks trained, each on a set of unequal depths: the step is not refused (the Adam launch
    takes the trained parts of the arena as at most kAdamSegs merged segments), the stats and the trained stacks' gradients
    are those of the twin, and a frozen stack's parameters and moments are the bits they were."""
    S = 3 if kind == "state_dependent" else 2
    for mask in range(1, (1 << S) - 1):
        c = F.ppo_step_case(mask % 4, kind)
        assert len(set(c.depths)) > 1
        eng, batch, index = bound_engine(c)
        before = eng.params.clone()
        want = F.step_twin(c)
        dirty(eng)
        stats = eng.ppo_step(batch, step_params(c, 1, mask), c.first, c.rows, index).cpu()       # raises if refused
        check_stats(stats, want.stats[0], OUT_BOUND, (c.name, mask))
        trained = [s for s in range(S) if (mask >> s) & 1]
        errs = grad_errors(eng, eng.ppo_grad, want.grads, trained)
        print(c.name, "depths", c.depths, "train_mask", mask, "largest gradient error %.3g" % max(errs))
        assert max(errs) <= GRAD_BOUND
        for s in range(S):
            for off, n in stack_span(eng, s):
                if s in trained:
                    assert bool(torch.isfinite(eng.params[off: off + n]).all())
                else:
                    assert torch.equal(eng.params[off: off + n], before[off: off + n])
                    assert float(eng.ppo_m[off: off + n].abs().max()) == 0.0 and float(eng.ppo_v[off: off + n].abs().max()) == 0.0
            if s in trained and float(want.grads[s][0][0].abs().max()) > 0:           # (a one-row batch may leave a stack no gradient)
                assert not torch.equal(eng.views(s)[0][0], eng.views(s, before)[0][0]), (mask, s)
        assert float(arena_pads(eng.m, eng.params).abs().max()) == 0.0


@pytest.mark.parametrize("seed,kind", [(6, "constant"), (2, "state_dependent")])
def test_sgd_loop_over_a_ragged_batch_equals_the_steps_one_by_one(seed, kind):
    c = F.ppo_step_case(seed, kind)
    assert c.rows == 97 and c.index is None
    a, batch_a, _ = bound_engine(c)
    b, batch_b, _ = bound_engine(c)
    n, mb, passes = c.rows, 40, 2                                                    # minibatches of 40, 40 and 17 rows
    perm = torch.stack([torch.randperm(n, generator=torch.Generator().manual_seed(40 + p)) for p in range(passes)]).to(torch.int32).to(DEV)
    stats = a.ppo_sgd(batch_a, step_params(c, 1), mb, passes, perm=perm)
    assert stats.shape == (6, 5) and bool(torch.isfinite(stats).all())
    t = 0
    for p in range(passes):
        for first in range(0, n, mb):
            t += 1
            one = b.ppo_step(batch_b, step_params(c, t), first, min(mb, n - first), perm[p])
            assert torch.equal(one, stats[t - 1]), (p, first)
    assert torch.equal(a.params, b.params) and torch.equal(a.ppo_m, b.ppo_m) and torch.equal(a.ppo_v, b.ppo_v)


# ---------------------------------------------------------------------------------------
# (c) the loss head alone
# ---------------------------------------------------------------------------------------
def head_run(k, kind, idx, with_index, cur, dbatch, params, what):
    rows = idx.numel()
    stats, d_mean, d_value, d_leaf = F.head_twin(k, kind, idx)
    if kind == "state_dependent":
        ls_dev = cur["log_std"][idx].to(DEV)
    else:
        ls_dev = cur["log_std"][0].to(DEV).reshape(1, k).expand(rows, k)             # row stride 0
    index = idx.to(DEV, torch.int32) if with_index else None
    args = (cur["mean"][idx].to(DEV), ls_dev, cur["value"][idx].to(DEV), dbatch, params, index)
    got = ppo_loss(*args)
    again = ppo_loss(*args)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                       # fixed summation order
    g_stats, g_mean, g_ls, g_value = (t.cpu() for t in got)
    got_ls = g_ls if kind == "state_dependent" else g_ls.double().sum(0)
    e = [max_err_scaled(g_stats, stats), max_err_scaled(g_mean, d_mean), max_err_scaled(g_value, d_value), max_err_scaled(got_ls, d_leaf)]
    print(what, "stats %.3g d_mean %.3g d_value %.3g d_log_std %.3g" % tuple(e))
    assert e[0] < OUT_BOUND and e[1] < GRAD_BOUND and e[2] < GRAD_BOUND and e[3] < GRAD_BOUND
    check_stats(g_stats, stats, OUT_BOUND, what)
    assert bool(torch.isfinite(g_ls).all())


def head_setup(k, kind):
    cur, batch, cfg = F.head_case(k, kind)
    assert F.head_covered(coverage(cur, batch, cfg))
    params = P.PPOConfig(**F.LOSS).params(kind)
    return cur, make_ppo_batch({key: v.to(DEV) for key, v in batch.items()}, DEV, k), params


@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("k", F.HEAD_KS)
def test_head_matches_the_float64_restatement_at_every_action_count(k, kind):
    cur, dbatch, params = head_setup(k, kind)
    for rows, with_index, idx in F.head_runs(k, kind):
        head_run(k, kind, idx, with_index, cur, dbatch, params, (k, kind, rows, with_index))


def test_head_past_its_wave_cap():
    k, kind = F.WAVE_CAP_K, F.WAVE_CAP_KIND
    cur, dbatch, params = head_setup(k, kind)
    for rows in F.WAVE_CAP_ROWS:
        head_run(k, kind, F.wave_cap_index(rows), True, cur, dbatch, params, (k, kind, rows, "gathered"))


# ---------------------------------------------------------------------------------------
# (d) GAE and the standardisation
# ---------------------------------------------------------------------------------------
def gae_check(lengths, done, gamma, lambda_, raw):
    want_adv, want_vt, want_std = dense_want(gamma, lambda_, lengths, done)
    what = "%d segments, %d rows, gamma %g lambda %g" % (len(lengths), sum(lengths), gamma, lambda_)
    if raw:
        adv, vt, launches = run_dense(gamma, lambda_, False, lengths, done)          # (run_dense checks the guard rows)
        e = (max_err_scaled(adv.cpu(), want_adv), max_err_scaled(vt.cpu(), want_vt))
        print(what, "raw: adv %.3g value_targets %.3g" % e)
        assert launches == 1 and e[0] <= OUT_BOUND and e[1] <= OUT_BOUND
    sadv, svt, launches = run_dense(gamma, lambda_, True, lengths, done)
    s64 = sadv.double().cpu()
    e = (max_err_scaled(s64, want_std), max_err_scaled(svt.cpu(), want_vt), abs(float(s64.mean())), abs(float(s64.std(unbiased=False)) - 1.0))
    print(what, "standardised: err %.3g value_targets %.3g |mean| %.3g |std - 1| %.3g" % e)
    assert launches == 2 and all(x <= OUT_BOUND for x in e)
    again = run_dense(gamma, lambda_, True, lengths, done)
    assert torch.equal(again[0], sadv) and torch.equal(again[1], svt)               # the same inputs give the same bits


@pytest.mark.parametrize("gamma,lambda_", [(0.98, 0.95), (1.0, 1.0), (0.9, 0.0)])
def test_gae_with_more_segments_than_one_pass_of_the_grid(gamma, lambda_):
    gae_check(*F.many_segments(), gamma, lambda_, True)


@pytest.mark.parametrize("gamma,lambda_", [(0.98, 0.95), (1.0, 1.0)])
def test_gae_with_more_rows_than_one_pass_of_the_standardisation(gamma, lambda_):
    gae_check(*F.many_rows(), gamma, lambda_, False)


def test_constant_advantage_meets_the_floor_not_a_rounding_residue():
    lengths = (1, 99, 200, 150, 250, 37, 263)
    n = sum(lengths)
    assert n == 1000
    (abuf, adv), (vbuf, vt) = guarded(n), guarded(n)
    E.gae(torch.full((n,), 0.5, device=DEV), torch.zeros(n, device=DEV), torch.zeros(len(lengths), device=DEV),
          F.seg_start_of(lengths), 0.0, 0.95, standardize=True, out=(adv, vt))
    torch.cuda.synchronize()
    assert guards_intact(abuf) and guards_intact(vbuf)
    print("constant advantage: largest |standardised| %.3g" % float(adv.abs().max()))
    assert bool(torch.isfinite(adv).all()) and float(adv.abs().max()) <= 1e-6        # (0.5 - mean) / 1e-4, not / a residue
    assert torch.equal(vt, torch.full_like(vt, 0.5))


# ---------------------------------------------------------------------------------------
# (e) evaluate and prepare at the edges
# ---------------------------------------------------------------------------------------
def learner_case(kind, k, n_in, rows, max_batch, seed):
    stacks = [((8, 8), ("relu", "tanh"), k), ((8,), ("relu",), 1)] + ([((8,), ("elu",), k)] if kind == "state_dependent" else [])
    c = F.build_case("learner", n_in, stacks, rows, max_batch, seed)
    c.kind, c.k = kind, k
    g = torch.Generator().manual_seed(seed + 1)
    c.ls_vec = None if kind == "state_dependent" else F.LS_BASE + 0.2 * torch.randn(k, generator=g)
    if kind == "state_dependent":
        w, b = c.params[2][-1]
        c.params[2][-1] = (0.2 * w, 0.2 * b)
    return c, g


def want_columns(c, ro, gamma, lambda_, standardize):
    """The host path in float64, as `want_columns` of tests/test_gpu_gae.py: the twin over the rows and the bootstrap rows,
    then gae_torch and standardize_torch."""
    with torch.no_grad():
        params = F.leaves(c.params, torch.float64)
        ls_vec = None if c.ls_vec is None else c.ls_vec.double()
        mean, ls, value, _ = F.step_outputs(c, params, ls_vec, ro["obs"].double())
        _, _, boot, _ = F.step_outputs(c, params, ls_vec, ro["boot_obs"].double())
    last = boot * (~ro["seg_done"]).double()
    adv, vt = P.gae_torch(ro["rewards"].double(), value, last, ro["seg_start"], gamma, lambda_)
    return {"vf_preds": value, "old_dist": torch.cat([mean, ls], 1), "old_logp": F.logp_of(mean, ls, ro["actions"].double()),
            "last_value": last, "advantages": P.standardize_torch(adv) if standardize else adv, "value_targets": vt}


def rollout(c, g, lengths, done):
    n, s = sum(lengths), len(lengths)
    return {"obs": torch.randn(n, c.n_in, generator=g), "actions": 0.5 * torch.randn(n, c.k, generator=g),
            "rewards": torch.rand(n, generator=g), "boot_obs": torch.randn(s, c.n_in, generator=g),
            "seg_start": F.seg_start_of(lengths), "seg_done": torch.tensor(done, dtype=torch.bool)}


def column_errors(got, want):
    e = {key: max_err_scaled(got[key].cpu(), want[key]) for key in got if key != "old_logp"}
    if "old_logp" in got:
        e["old_logp"] = logp_err(got["old_logp"], want["old_logp"])
    return e


@pytest.mark.parametrize("kind", F.KINDS)
def test_evaluate_and_the_first_step_after_prepare_at_the_action_counts(kind):
    lengths, done = (30, 1, 2, 37), (True, False, False, True)                       # 70 rows: chunks of 32, 32 and 6
    for k in (1, 65, 130):
        c, g = learner_case(kind, k, 7, 70, 32, 9000 + k)
        eng, gp = engine_for(c), P.make_gae_params(0.98, 0.95, True, kind, F.LS_BASE if kind == "state_dependent" else 0.0)
        ls = None if c.ls_vec is None else c.ls_vec.to(DEV)
        eng.ppo_bind(ls, kind == "state_independent")
        ro = rollout(c, g, lengths, done)
        dro = {key: v.to(DEV) for key, v in ro.items()}
        want = want_columns(c, ro, 0.98, 0.95, True)
        eng.workspace.fill_(float("nan"))
        got = eng.ppo_evaluate({key: dro[key] for key in ("obs", "actions", "seg_done", "boot_obs")}, gp)
        e = column_errors(got, want)
        print(kind, "K", k, "evaluate", {key: "%.3g" % v for key, v in e.items()})
        assert set(e) == {"vf_preds", "old_dist", "old_logp", "last_value"} and all(v <= OUT_BOUND for v in e.values())
        batch = eng.ppo_prepare(dro, gp)
        assert all(torch.equal(batch[key], got[key]) for key in got)
        e = column_errors(batch, want)
        print(kind, "K", k, "prepare", {key: "%.3g" % v for key, v in e.items()})
        assert all(v <= OUT_BOUND for v in e.values())
        # the learner's first step sees its own distribution: old_logp is the head's logp of the same rows TO THE BIT, so
        # the ratio is exactly 1 and the policy term is -mean(adv); the KL is that of a distribution to itself, a sum of k
        # terms each 0 but for the rounding of exp(2 l) * 0.5 exp(-l)^2 - 0.5 (a few ulp of 0.5: under 2e-7 a term)
        cols = dict({key: batch[key] for key in ("old_dist", "old_logp", "advantages", "value_targets", "vf_preds")},
                    obs=dro["obs"], actions=dro["actions"])
        stats = eng.ppo_step(cols, CFG.params(kind, gp.log_std_base, adam_t=1), 0, 32).cpu()
        mean_adv = float(batch["advantages"][:32].double().mean())
        print(kind, "K", k, "first step: policy %.9g -mean(adv) %.9g kl %.3g" % (float(stats[1]), -mean_adv, float(stats[3])))
        assert abs(float(stats[1]) + mean_adv) <= 1e-6 and abs(float(stats[3])) <= 2e-7 * k


def test_prepare_in_chunks_larger_than_the_epilogue_and_copy_grids():
    lengths, done = F.many_segments()
    kind, k, max_batch = "constant", 3, 4160
    assert sum(lengths) == 2 * max_batch + 416 and max_batch > 4096 and max_batch * 64 > 262144 and len(lengths) > max_batch
    c, g = learner_case(kind, k, 5, 8, max_batch, 9500)
    eng, gp = engine_for(c), P.make_gae_params(0.98, 0.95, True, kind, 0.0)
    eng.ppo_bind(c.ls_vec.to(DEV), False)
    ro = rollout(c, g, lengths, done)
    n, s = sum(lengths), len(lengths)
    bufs = {"vf_preds": guarded(n), "old_dist": guarded(n, 2 * k), "old_logp": guarded(n), "last_value": guarded(s),
            "advantages": guarded(n), "value_targets": guarded(n)}
    eng.workspace.fill_(float("nan"))
    got = eng.ppo_prepare({key: v.to(DEV) for key, v in ro.items()}, gp, out={key: v[1] for key, v in bufs.items()})
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b, _ in bufs.values())
    # evaluate: three chunks of copy-in + three layer depths + epilogue; then two bootstrap chunks of copy-in + two depths +
    # epilogue, the GAE launch and the rescale
    assert eng.gae_launches() == (3 * 5, 2 * 4 + 2)
    e = column_errors(got, want_columns(c, ro, 0.98, 0.95, True))
    print("prepare of %d rows in %d segments:" % (n, s), {key: "%.3g" % v for key, v in e.items()})
    assert len(e) == 6 and all(v <= OUT_BOUND for v in e.values())
    done_t = ro["seg_done"]
    assert bool((got["last_value"].cpu()[done_t] == 0.0).all())


# ---------------------------------------------------------------------------------------
# (f) a stack without a hidden layer
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [5, 40])
def test_a_stack_without_a_hidden_layer_matches_the_twin(rows):
    """depth[s] == 0: the stack is its linear output layer alone, inside the shared first-layer GEMM (its dense result stored
    from a column segment of that GEMM's epilogue, its output gradient seeded into the shared first-layer gradient panel)."""
    c = F.build_case("depth0", 22, (((17, 31), ("relu", "tanh"), 7), ((), (), 3)), rows, 40, 9700 + rows)
    eng = engine_for(c)
    assert eng.cfg.depth[1] == 0 and len(eng.stack_layers(1)) == 1
    x, dys = c.x.to(DEV), [d.to(DEV) for d in c.dys]
    want = F.twin64(c, c.x, c.dys)
    for per_stack in (False, True):
        set_fc_per_stack(per_stack)
        outs, dx, grad, acc = run_all(eng, x, dys, 3)
        e = (max(max_err_scaled(o.cpu(), w) for o, w in zip(outs, want.outs)), max_err_scaled(dx.cpu(), want.dx),
             max(grad_errors(eng, grad, want.grads, range(2))))
        print("depth 0, rows", rows, "per stack" if per_stack else "grouped", "outputs %.3g dx %.3g gradients %.3g" % e)
        assert e[0] <= OUT_BOUND and e[1] <= GRAD_BOUND and e[2] <= GRAD_BOUND
        assert float(arena_pads(eng.m, grad).abs().max()) == 0.0 and torch.equal(acc, grad + 1.0)
    # the stack alone, forward and backward: the first-layer range is that one block
    eng.workspace.fill_(float("nan"))
    alone = eng.forward(x, want=[False, True])
    assert max_err_scaled(alone[1].cpu(), want.outs[1]) <= OUT_BOUND
    w1 = F.twin64(c, c.x, [None, c.dys[1]])
    buf = torch.full((eng.arena_floats,), SENTINEL, device=DEV)
    dx1 = eng.backward(x, [None, dys[1]], True, buf, grad_mask=2)
    assert max_err_scaled(dx1.cpu(), w1.dx) <= GRAD_BOUND and max(grad_errors(eng, buf, w1.grads, [1])) <= GRAD_BOUND
    assert all(bool((buf[off: off + n] == SENTINEL).all()) for off, n in stack_span(eng, 0))
