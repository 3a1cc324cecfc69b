"""Global-norm gradient clipping inside the fused PPO learners on the GPU (include/pvae.h "Gradient clipping inside the PPO
learners"; physicsvae_amd/ppo.py `ClippedPPOConfig`, `clip_coef_torch`), for a stack set and for PhysicsVAE:

  (1) the bit-exact decomposition: a clipped step with diagnostics bound gives coef in entry 6; from the same start
      `*_ppo_grad` with no clip bound and `*_ppo_apply(grad_scale = coef)` give the same parameters, moments, log-std vector
      and stats, bit for bit; so do `*_ppo_grad` WITH the clip bound (the gradient left behind is the unclipped one times
      coef, element by element) and `*_ppo_apply(1.0)`.  Threshold: half the raw norm;
  (2) the numbers: entry 5 against `grad_gnorm_torch` of the unclipped gradient the device holds, entry 6 against
      `clip_coef_torch` of it, entry 4 <= max_norm and = entry 5 x entry 6 -- all within the bound of the existing
      gradient-norm test (tests/ppo_diag_cases.py GNORM_RTOL);
  (3) a threshold that never bites (1e30): every output bit-identical to the unbound step, one launch more; after unbinding
      the launches and the bits are the plain step's;
  (4) masks: with the value stack frozen its gradient does not enter the norm and its parameters and moments stay; the
      trained log-std vector enters the norm and is scaled (through (1));
  (5) `*_ppo_sgd` over 2 passes x 3 minibatches: every diagnostics row obeys the relations, the same call from the same state
      gives the same bits, and the steps one by one give them too;
  (6) three steps of `ppo_learn(ClippedPPOConfig(...))` against the float64 twin -- `ppo_loss_torch`, autograd,
      `clip_grad_norm_`, torch.optim.Adam -- at the bounds of the unclipped twin tests (tests/test_gpu_ppo.py,
      tests/test_gpu_ppo_vae.py; tests/test_gpu_ppo_vae_shapes.py for the cases of tests/vae_ppo_cases.py).
Shapes: tests/ppo_clip_cases.py; PhysicsVAE at the tiny dims of tests/vae_ppo_cases.py."""
import math

import pytest
import torch

import fc_cases as F
import ppo_clip_cases as CC
import ppo_diag_cases as D
import vae_ppo_cases as V
from physicsvae_amd import fcnn
from physicsvae_amd import ppo as P
from ppo_cases import KINK, coverage
from ppo_clip_cases import same_bits
from test_gpu_fc_shapes import bound_engine, dirty, stack_span, step_params
from test_gpu_fcnn import Twin, policy
from test_gpu_ppo import MOMENT_BOUNDS, PARAM_BOUND, check_stats
from test_gpu_ppo_diag import fc_state, moved, nan_rows
from util import max_err_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = D.GNORM_RTOL
NEVER = 1e30


def c32(x):
    return torch.tensor(float(x), dtype=torch.float32, device=DEV)


# ---------------------------------------------------------------------------------------
# the stack set
# ---------------------------------------------------------------------------------------
def trained_grads(eng, trained):
    return [eng.ppo_grad[off: off + n] for s in trained for off, n in stack_span(eng, s)]


@pytest.mark.parametrize("name,mask,first,rows", [("small", 0, 0, 16), ("short", 0, 32, 9), ("wide", 0, 16, 16), ("small", 1, 16, 16)])
def test_clipped_step_is_grad_then_apply_with_the_coefficient(name, mask, first, rows):
    c = CC.fc_case(name)
    if name == "wide":
        assert c.float4 > 4 * CC.CLIP_GRID_FLOAT4                                    # the grid-stride loop runs five times
    trained = [s for s in range(2) if not mask or (mask >> s) & 1]
    p1 = step_params(c, 1, mask)
    (a, batch_a, _), (b, batch_b, _), (e, batch_e, _) = bound_engine(c), bound_engine(c), bound_engine(c)
    rows_abe = []
    for eng in (a, b, e):
        dirty(eng)
        eng.ppo_grad.fill_(1e6)                                                      # a frozen stack's part must not show
        rows_abe.append(nan_rows(1))
        eng.ppo_diag(rows_abe[-1])
    row_a, row_b, row_e = rows_abe
    before = fc_state(a)
    # the unclipped first half on b: the gradient the device holds, its float64 norm
    st_b, ls_b = b.ppo_grad_step(batch_b, p1, first, rows)
    launches_grad = b.ppo_launches()
    assert float(row_b[0, 5:].abs().max()) == 0.0                                    # no clip bound: the reserved entries stay 0
    grads = [g.clone() for g in trained_grads(b, trained)] + [ls_b.clone()]
    raw = float(P.grad_gnorm_torch(grads))
    policy_only = float(P.grad_gnorm_torch([b.ppo_grad[off: off + n] for off, n in stack_span(b, 0)] + [ls_b]))
    max_norm = 0.5 * raw
    want_norm, want_coef = P.clip_coef_torch(grads, max_norm)
    # the clipped step on a
    a.ppo_grad_clip(max_norm)
    st_a = a.ppo_step(batch_a, p1, first, rows)
    got = row_a[0].cpu().clone()
    coef = float(got[6])
    print(c.name, "mask", mask, "rows", rows, "raw", float(got[5]), "float64", raw, "coef", coef, "want", float(want_coef),
          "grad_gnorm", float(got[4]), "max_norm", max_norm)
    assert 0.4 < coef < 0.51
    assert abs(float(got[5]) - raw) <= RTOL * raw and abs(float(got[5]) - float(want_norm)) <= RTOL * raw
    assert abs(coef - float(want_coef)) <= RTOL * float(want_coef)
    CC.check_row(got, max_norm, RTOL, c.name)
    if mask == 1:
        assert raw == policy_only                                                    # the frozen value stack does not enter
    # b: apply(coef) on the unclipped gradient -- the same step, bit for bit
    b.ppo_apply(p1, coef, ls_b)
    assert same_bits(st_a, st_b) and not moved(fc_state(a), fc_state(b)), moved(fc_state(a), fc_state(b))
    assert same_bits(row_a[0, :5], row_b[0, :5])
    assert moved(before, fc_state(a))
    # e: the first half WITH the clip bound leaves the clipped gradient, apply(1.0) does not clip again
    e.ppo_grad_clip(max_norm)
    st_e, ls_e = e.ppo_grad_step(batch_e, p1, first, rows)
    assert e.ppo_launches() == launches_grad + 2
    for g_e, g_b in zip(trained_grads(e, trained) + [ls_e], grads):
        assert same_bits(g_e, g_b * c32(coef))
    half = row_e[0].cpu().clone()
    assert math.isnan(float(half[4])) and same_bits(half[5:], got[5:]) and same_bits(half[:4], got[:4])
    e.ppo_apply(p1, 1.0, ls_e)
    assert same_bits(st_e, st_a) and not moved(fc_state(a), fc_state(e)), moved(fc_state(a), fc_state(e))
    assert same_bits(row_e[0].cpu(), got)
    # a frozen stack: parameters and moments untouched, its part of the gradient arena never written
    for s in range(2):
        if s not in trained:
            for off, n in stack_span(a, s):
                assert same_bits(a.params[off: off + n], before["params"][off: off + n])
                assert float(a.ppo_m[off: off + n].abs().max()) == 0.0 and float(a.ppo_v[off: off + n].abs().max()) == 0.0
                assert float((a.ppo_grad[off: off + n] - 1e6).abs().max()) == 0.0


@pytest.mark.parametrize("name,first,rows", [("small", 0, 16), ("short", 32, 9), ("wide", 16, 16)])
def test_a_threshold_that_never_bites_and_unbinding(name, first, rows):
    c = CC.fc_case(name)
    p1, p2 = step_params(c, 1), step_params(c, 2)
    (a, batch_a, _), (b, batch_b, _) = bound_engine(c), bound_engine(c)
    for eng in (a, b):
        dirty(eng)
    st_a = a.ppo_step(batch_a, p1, first, rows)
    plain = a.ppo_launches()
    if name != "wide":
        assert plain == 9
    b.ppo_grad_clip(NEVER)
    assert b.ppo_grad_clip_bound() == NEVER
    st_b = b.ppo_step(batch_b, p1, first, rows)
    assert b.ppo_launches() == plain + 1
    assert same_bits(st_a, st_b) and not moved(fc_state(a), fc_state(b)), moved(fc_state(a), fc_state(b))
    # with diagnostics too: one launch more again, entries 0..4 the unclipped step's, coef exactly 1
    row_a, row_b = nan_rows(1), nan_rows(1)
    a.ppo_diag(row_a)
    b.ppo_diag(row_b)
    assert same_bits(a.ppo_step(batch_a, p2, first, rows), b.ppo_step(batch_b, p2, first, rows))
    assert a.ppo_launches() == plain + 1 and b.ppo_launches() == plain + 2
    assert same_bits(row_a[0, :5], row_b[0, :5]) and float(row_a[0, 5:].abs().max()) == 0.0
    assert float(row_b[0, 6]) == 1.0 and float(row_b[0, 7]) == 0.0
    assert abs(float(row_b[0, 5]) - float(row_b[0, 4])) <= RTOL * float(row_b[0, 4])
    assert not moved(fc_state(a), fc_state(b))
    # unbound: the launches and the bits are the plain step's, and nothing writes entries 5 and 6 any more
    b.ppo_grad_clip(None)
    assert b.ppo_grad_clip_bound() is None
    row_b.fill_(float("nan"))
    p3 = step_params(c, 3)
    assert same_bits(a.ppo_step(batch_a, p3, first, rows), b.ppo_step(batch_b, p3, first, rows))
    assert b.ppo_launches() == plain + 1 and same_bits(row_a, row_b) and float(row_b[0, 5:].abs().max()) == 0.0
    a.ppo_diag(None)
    b.ppo_diag(None)
    p4 = step_params(c, 4)
    assert same_bits(a.ppo_step(batch_a, p4, first, rows), b.ppo_step(batch_b, p4, first, rows))
    assert b.ppo_launches() == plain and not moved(fc_state(a), fc_state(b))


@pytest.mark.parametrize("name", ["small", "short"])
def test_sgd_rows_obey_the_relations_and_repeat(name):
    c = CC.fc_case(name)
    n, mb, passes = c.rows, CC.MINIBATCH, 2
    assert -(-n // mb) == 3
    perm = torch.stack([torch.randperm(n, generator=torch.Generator().manual_seed(90 + p)) for p in range(passes)]).to(torch.int32).to(DEV)
    engines = [bound_engine(c) for _ in range(3)]
    (a, batch_a, _), (b, batch_b, _), (e, batch_e, _) = engines
    # the threshold: half the first minibatch's raw norm, from the device's own unclipped gradient
    _, ls = e.ppo_grad_step(batch_e, step_params(c, 1), 0, mb, perm[0])
    max_norm = 0.5 * float(P.grad_gnorm_torch(trained_grads(e, (0, 1)) + [ls]))
    out = []
    for eng, batch in ((a, batch_a), (b, batch_b)):
        dirty(eng)
        diag = nan_rows(6)
        eng.ppo_diag(diag)
        eng.ppo_grad_clip(max_norm)
        out.append((eng.ppo_sgd(batch, step_params(c, 1), mb, passes, perm=perm), diag))
        assert eng.ppo_launches() == 9 + 2
    (stats_a, diag_a), (stats_b, diag_b) = out
    assert same_bits(stats_a, stats_b) and same_bits(diag_a, diag_b) and not moved(fc_state(a), fc_state(b))
    assert bool(torch.isfinite(diag_a).all()) and bool(torch.isfinite(stats_a).all())
    rows = diag_a.cpu()
    for i in range(6):
        CC.check_row(rows[i], max_norm, RTOL, (c.name, i))
    print(c.name, "coef per step", rows[:, 6].tolist())
    assert float(rows[0, 6]) < 1.0
    # the steps one by one
    one = nan_rows(1)
    e.ppo_diag(one)
    e.ppo_grad_clip(max_norm)
    t = 0
    for p in range(passes):
        for first in range(0, n, mb):
            st = e.ppo_step(batch_e, step_params(c, t + 1), first, min(mb, n - first), perm[p])
            assert same_bits(st, stats_a[t]) and same_bits(one[0], diag_a[t]), (p, first)
            t += 1
    assert not moved(fc_state(a), fc_state(e))


def fc_model(seed=31):
    torch.manual_seed(seed)
    cmc = {"log_std_type": "state_independent", "sample_std": 0.3, "policy_fn_layers": fcnn.DEFAULT_FC_64X2,
           "value_fn_layers": fcnn.DEFAULT_FC_64X2}
    m = policy(cmc, obs=CC.N_IN, num_outputs=2 * CC.K, max_batch=CC.MINIBATCH)
    with torch.no_grad():                        # biases off zero
        for k, p in m.named_parameters():
            if k.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(3)).to(DEV))
    return m, cmc


def fc_batch(twin, n, seed):
    """tests/test_gpu_ppo.py `sample_batch` at this file's shapes, around the float64 twin's outputs."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)                                    # noqa: E731
    obs, k = rn(n, CC.N_IN), CC.K
    with torch.no_grad():
        logits = twin(obs.double()).float()
        value = twin.cur_value.float()
    mean, ls = logits[:, :k], logits[:, k:]
    actions = mean + torch.exp(ls) * rn(n, k)
    return {"obs": obs, "actions": actions, "action_dist_inputs": torch.cat([mean + 0.02 * rn(n, k), ls + 0.05 * rn(n, k)], 1),
            "action_logp": F.logp_of(mean, ls, actions) - 0.35 * rn(n), "advantages": rn(n), "value_targets": value + rn(n),
            "vf_preds": value + rn(n)}, {"mean": mean, "log_std": ls, "value": value}


def test_three_steps_of_ppo_learn_match_the_clipped_float64_twin():
    hyper = dict(clip_param=0.2, kl_coeff=0.3, entropy_coeff=0.01, vf_clip_param=0.7, vf_loss_coeff=0.5, lr=1e-4,
                 sgd_minibatch_size=CC.MINIBATCH, num_sgd_iter=1)
    m, cmc = fc_model()
    twin = Twin(m, cmc).double()
    n, mb, k = 48, CC.MINIBATCH, CC.K
    batch, cur = fc_batch(twin, n, seed=7)
    cols = {key: v for key, v in P.batch_columns(batch).items() if key != "obs"}
    for i in range(3):                                                               # no row of a minibatch sits at a kink of the loss
        sl = slice(i * mb, (i + 1) * mb)
        cov = coverage({key: v[sl] for key, v in cur.items()}, {key: v[sl] for key, v in cols.items()}, P.PPOConfig(**hyper))
        assert cov["kink"] > KINK, (i, cov)

    def twin_backward(idx):
        c64 = {key: v[idx].double() for key, v in P.batch_columns(batch).items()}
        logits = twin(c64.pop("obs"))
        total, stats = P.ppo_loss_torch(logits[:, :k], logits[:, k:], twin.cur_value, cfg=cfg, **c64)
        twin.zero_grad(set_to_none=True)
        total.backward()
        return stats.detach()
    cfg = P.PPOConfig(**hyper)
    twin_backward(torch.arange(mb))
    max_norm = 0.5 * float(P.grad_gnorm_torch([p.grad for p in twin.parameters()]))  # half the twin's own first norm
    cfg = P.ClippedPPOConfig(grad_clip=max_norm, **hyper)
    opt = torch.optim.Adam(twin.parameters(), lr=cfg.lr)
    diag = P.diag_buffer(n, cfg, DEV)
    got = m.ppo_learn({key: v.to(DEV) for key, v in batch.items()}, cfg, diag_out=diag).cpu()
    assert got.shape == (3, 5) and m.engine.ppo_launches() == 9 + 2
    assert m.engine.ppo_grad_clip_bound() is None and m.engine.ppo_diag_bound() is None       # bound for the call alone
    rows = diag.cpu()
    for step in range(3):
        want = twin_backward(torch.arange(step * mb, (step + 1) * mb))
        norm = float(torch.nn.utils.clip_grad_norm_(twin.parameters(), max_norm))
        opt.step()
        coef = min(1.0, max_norm / (norm + 1e-6))
        print("step", step, got[step].tolist(), want.tolist(), "raw", float(rows[step, 5]), norm, "coef", float(rows[step, 6]), coef)
        assert float(got[step, 0]) == pytest.approx(float(want[0]), rel=2e-4), step
        assert max_err_scaled(got[step], want) < 2e-4
        check_stats(got[step], want, 2e-4, ("clipped", step))
        assert abs(float(rows[step, 5]) - norm) <= 1e-4 * norm and abs(float(rows[step, 6]) - coef) <= 1e-4 * coef
        CC.check_row(rows[step], max_norm, RTOL, step)
    assert float(rows[0, 6]) < 0.51
    names, mine = twin.named_like(m), dict(m.named_parameters())
    assert set(names) == set(mine)
    for key, q in names.items():
        e = max_err_scaled(mine[key].detach().cpu(), q.detach())
        assert e < PARAM_BOUND, (key, e)
    from test_gpu_ppo import LS_KEY, arena_views
    moments = {key: (mm, vv) for (key, mm), vv in zip(arena_views(m, m.engine.ppo_m).items(), arena_views(m, m.engine.ppo_v).values())}
    moments[LS_KEY] = (m.engine.ppo_ls_m, m.engine.ppo_ls_v)
    assert set(moments) == set(names)
    for key, (mm, vv) in moments.items():
        state = opt.state[names[key]]
        e = (max_err_scaled(mm.cpu(), state["exp_avg"]), max_err_scaled(vv.cpu(), state["exp_avg_sq"]))
        print(key, "m %.3g v %.3g" % e)
        assert e[0] < MOMENT_BOUNDS[0] and e[1] < MOMENT_BOUNDS[1], (key, e)
    # the next call under the plain config is the plain learner again
    m.ppo_learn({key: v.to(DEV) for key, v in batch.items()}, P.PPOConfig(**hyper))
    assert m.engine.ppo_launches() == 9


# ---------------------------------------------------------------------------------------
# PhysicsVAE
# ---------------------------------------------------------------------------------------
VAE_CASES = ("masks_7", "masks_3", "no_prior_odd")       # all trained | the value branch frozen | no prior, odd widths


def vae_grads(TS, m, c, ls_grad):
    bit = {n: b for b, n in zip((1, 2, 4), V.NETS)}
    g = [t for key, t in TS.buffers(m, "grad").items() if c.mask & bit[key.split(".")[0]]]
    return g + ([ls_grad] if c.log_std_type == "state_independent" else [])


@pytest.mark.parametrize("name", VAE_CASES)
def test_physics_vae_clipped_step(name):
    import test_gpu_ppo_vae_shapes as TS
    c = V.case(name)
    assert c.log_std_type == "state_independent" and (name != "masks_3" or c.mask == 3)
    (ma, a, _), (mb, b, _), (me, e, _), (mf, f, _) = TS.setup(c), TS.setup(c), TS.setup(c), TS.setup(c)
    cols = a.ppo_batch({key: v.to(DEV) for key, v in c.batch.items()})
    index = c.index.to(DEV) if c.index is not None else None
    kw = dict(eps=c.eps.to(DEV), noise=c.noise, offset=1)
    p1 = TS.params_of(c, ma, 1)
    before = TS.state(ma)
    row_a, row_b, row_e = nan_rows(1), nan_rows(1), nan_rows(1)
    for eng, row in ((a, row_a), (b, row_b), (e, row_e)):
        eng.ppo_diag(row)
    # the unclipped first half on b
    for t in TS.buffers(mb, "grad").values():
        t.fill_(1e6)
    st_b, ls_b = b.ppo_grad_step(cols, p1, c.first, c.rows, index, **kw)
    launches_grad = b.ppo_launches()
    assert float(row_b[0, 5:].abs().max()) == 0.0
    grads = [g.clone() for g in vae_grads(TS, mb, c, ls_b)]
    raw = float(P.grad_gnorm_torch(grads))
    max_norm = 0.5 * raw
    want_norm, want_coef = P.clip_coef_torch(grads, max_norm)
    # the clipped step on a
    a.ppo_grad_clip(max_norm)
    st_a = a.ppo_step(cols, p1, c.first, c.rows, index, **kw)
    assert a.ppo_launches() == TS.launches(c) + 2
    got = row_a[0].cpu().clone()
    coef = float(got[6])
    print(name, "mask", c.mask, "raw", float(got[5]), "float64", raw, "coef", coef, "want", float(want_coef), "grad_gnorm", float(got[4]))
    assert 0.4 < coef < 0.51
    assert abs(float(got[5]) - raw) <= RTOL * raw and abs(coef - float(want_coef)) <= RTOL * float(want_coef)
    CC.check_row(got, max_norm, RTOL, name)
    b.ppo_apply(p1, coef, ls_b)
    assert same_bits(st_a, st_b) and not TS.same_state(TS.state(ma), TS.state(mb)), TS.same_state(TS.state(ma), TS.state(mb))
    assert same_bits(row_a[0, :5], row_b[0, :5]) and TS.same_state(before, TS.state(ma))
    # the first half with the clip bound, then apply(1.0)
    e.ppo_grad_clip(max_norm)
    st_e, ls_e = e.ppo_grad_step(cols, p1, c.first, c.rows, index, **kw)
    assert e.ppo_launches() == launches_grad + 2
    for g_e, g_b in zip(vae_grads(TS, me, c, ls_e), grads):
        assert same_bits(g_e, g_b * c32(coef))
    e.ppo_apply(p1, 1.0, ls_e)
    assert same_bits(st_e, st_a) and not TS.same_state(TS.state(ma), TS.state(me))
    assert same_bits(row_e[0].cpu(), got)
    if name == "masks_3":                                                            # the frozen value branch
        ve, now = ma.__dict__["_value_engine"], TS.state(ma)
        assert same_bits(now["value params"], before["value params"])
        assert float(ve.ppo_m.abs().max()) == 0.0 and float(ve.ppo_v.abs().max()) == 0.0
        policy_only = [t for key, t in TS.buffers(mb, "grad").items() if not key.startswith("_value_branch")] + [ls_b]
        assert raw == float(P.grad_gnorm_torch(policy_only))
    # a threshold that never bites on f against the unbound step on a fifth module; then unbound
    mg, g, _ = TS.setup(c)
    f.ppo_grad_clip(NEVER)
    assert same_bits(f.ppo_step(cols, p1, c.first, c.rows, index, **kw), g.ppo_step(cols, p1, c.first, c.rows, index, **kw))
    assert g.ppo_launches() == TS.launches(c) and f.ppo_launches() == TS.launches(c) + 1
    assert not TS.same_state(TS.state(mf), TS.state(mg))
    f.ppo_grad_clip(None)
    p2, kw2 = TS.params_of(c, mf, 2), dict(kw, offset=2)
    assert same_bits(f.ppo_step(cols, p2, c.first, c.rows, index, **kw2), g.ppo_step(cols, p2, c.first, c.rows, index, **kw2))
    assert f.ppo_launches() == TS.launches(c) and not TS.same_state(TS.state(mf), TS.state(mg))


def test_physics_vae_sgd_rows_obey_the_relations_and_repeat():
    import test_gpu_ppo_vae_shapes as TS
    c = V.case("masks_7")
    n, mb, passes = c.rows, 11, 2                                                    # 33 rows: three minibatches of 11
    gen = torch.Generator().manual_seed(c.seed + 21)
    perm = torch.stack([torch.randperm(n, generator=gen) for _ in range(passes)]).to(torch.int32).to(DEV)
    leps = torch.randn(6, mb, c.Z, generator=gen).to(DEV)
    batch = {key: v.to(DEV) for key, v in c.used.items()}
    (ma, a, _), (mb_, b, _), (me, e, _) = TS.setup(c), TS.setup(c), TS.setup(c)
    _, ls = e.ppo_grad_step(e.ppo_batch(batch), TS.params_of(c, me, 1), 0, mb, perm[0].contiguous(), eps=leps[0], noise=c.noise, offset=1)
    max_norm = 0.5 * float(P.grad_gnorm_torch(vae_grads(TS, me, c, ls)))
    out = []
    for m, eng in ((ma, a), (mb_, b)):
        diag = nan_rows(6)
        eng.ppo_diag(diag)
        eng.ppo_grad_clip(max_norm)
        out.append((eng.ppo_sgd(eng.ppo_batch(batch), TS.params_of(c, m, 1), mb, passes, perm, eps=leps, noise=c.noise, offset=1), diag))
        assert eng.ppo_launches() == TS.launches(c) + 2
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1]) and not TS.same_state(TS.state(ma), TS.state(mb_))
    rows = out[0][1].cpu()
    assert bool(torch.isfinite(rows).all())
    for i in range(6):
        CC.check_row(rows[i], max_norm, RTOL, ("vae", i))
    print("vae coef per step", rows[:, 6].tolist())
    assert float(rows[0, 6]) < 1.0


def clipped_vae_twin(c, max_norm, steps):
    """tests/vae_ppo_cases.py `step_twin` in float64 with `clip_grad_norm_` between backward and Adam."""
    params = V.leaves(c, torch.float64, c.mask)
    ls_vec = c.ls_vec.double().clone().requires_grad_(True)
    trained = [t for bit, net in zip((1, 2, 4), V.NETS) if c.mask & bit for pair in params[net] for t in pair] + [ls_vec]
    opt = torch.optim.Adam(trained, lr=V.LR)
    used = {key: t.double() for key, t in c.used.items()}
    stats, norms = [], []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        mean, ls, value, _, h = V.forward(c, params, ls_vec, used["obs"], c.eps.double())
        total, st = P.ppo_loss_torch(mean, ls, value, cfg=c.cfg, **{key: used[key] for key in used if key != "obs"})
        (total + 0.0 * h.sum()).backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(trained, max_norm)))
        opt.step()
        stats.append(st.detach())
    return stats, norms, params, ls_vec, opt


def test_physics_vae_ppo_learn_matches_the_clipped_float64_twin():
    import test_gpu_ppo_vae_shapes as TS
    c = V.case("masks_7")
    first = V.step_twin(c, steps=1)
    raw = float(P.grad_gnorm_torch([g for net in first.grads.values() for pair in net for g in pair] + [first.ls_grad]))
    max_norm = 0.5 * raw                                                             # half the twin's own first norm
    stats, norms, params, ls_vec, opt = clipped_vae_twin(c, max_norm, 3)
    m, eng, ve = TS.setup(c)
    cfg = P.ClippedPPOConfig(lr=V.LR, sgd_minibatch_size=c.rows, num_sgd_iter=3, grad_clip=max_norm, **F.LOSS)
    rllib = {theirs: c.used[ours].to(DEV) for theirs, ours in P.SAMPLE_BATCH_KEYS.items()}
    diag = P.diag_buffer(c.rows, cfg, DEV)
    got = m.ppo_learn(rllib, cfg, eps=c.eps.to(DEV).repeat(3, 1, 1), diag_out=diag).cpu()
    assert got.shape == (3, 5) and eng.ppo_launches() == TS.launches(c) + 2 and eng.ppo_grad_clip_bound() is None
    rows = diag.cpu()
    for step in range(3):
        coef = min(1.0, max_norm / (norms[step] + 1e-6))
        print("vae step", step, got[step].tolist(), stats[step].tolist(), "raw", float(rows[step, 5]), norms[step], "coef", float(rows[step, 6]), coef)
        check_stats(got[step], stats[step], V.STATS_BOUND, ("vae clipped", step))
        assert abs(float(rows[step, 5]) - norms[step]) <= V.GRAD_BOUND * norms[step]
        assert abs(float(rows[step, 6]) - coef) <= V.GRAD_BOUND * coef
        CC.check_row(rows[step], max_norm, RTOL, ("vae twin", step))
    assert float(rows[0, 6]) < 0.51
    now, mom_m, mom_v = TS.views_of(m), TS.buffers(m, "m"), TS.buffers(m, "v")
    e_p, e_m, e_v = [], [], []
    for net in V.NETS:
        for i, pair in enumerate(params[net]):
            for kind, leaf in zip(("weight", "bias"), pair):
                key = TS.KEY % (net, i, kind)
                wm, wv = V.state_of(opt, leaf)
                e_p.append(max_err_scaled(now[key].cpu(), leaf.detach()))
                e_m.append(max_err_scaled(mom_m[key].cpu(), wm))
                e_v.append(max_err_scaled(mom_v[key].cpu(), wv))
    wm, wv = V.state_of(opt, ls_vec)
    e_p.append(max_err_scaled(m._als.log_std.detach().cpu(), ls_vec.detach()))
    e_m.append(max_err_scaled(eng.ppo_ls_m.cpu(), wm))
    e_v.append(max_err_scaled(eng.ppo_ls_v.cpu(), wv))
    print("vae after three clipped steps: parameters %.3g m %.3g v %.3g" % (max(e_p), max(e_m), max(e_v)))
    assert max(e_p) < V.PARAM_BOUND and max(e_m) < V.MOMENT_BOUNDS[0] and max(e_v) < V.MOMENT_BOUNDS[1]
