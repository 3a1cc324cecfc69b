"""The learner diagnostics without a GPU (include/pvae.h "Learner diagnostics"; physicsvae_amd/ppo.py `DIAG`): the
specification `learner_diag_torch` on a hand case, its float32 restatement over the loss-head cases the GPU tests use,
the host helpers, and what the new entry points refuse before they touch a device."""
import ctypes as C
import math
import types

import pytest
import torch

import fc_cases as F
import ppo_diag_cases as D
from physicsvae_amd import _lib
from physicsvae_amd import ppo as P
from ppo_cases import coverage


def hand_case(dtype=torch.float64):
    """4 rows, k = 1, log_std 0, actions = mean: logp = -0.5 log(2 pi), and old_logp is chosen so that the ratios are
    exactly 1.5, 0.5, 1.1 and 0.95.  clip_param 0.2: rows 0 and 1 are clipped.  value - vf_preds = 1, -1, 0.25, 0: with
    vf_clip_param 0.5 rows 0 and 1 are value-clipped.  y = 1, 2, 3, 6 and y - v = 1, -1, 1, -1."""
    ratios = torch.tensor([1.5, 0.5, 1.1, 0.95], dtype=dtype)
    mean = torch.zeros(4, 1, dtype=dtype)
    ls = torch.zeros(4, 1, dtype=dtype)
    y = torch.tensor([1.0, 2.0, 3.0, 6.0], dtype=dtype)
    value = y - torch.tensor([1.0, -1.0, 1.0, -1.0], dtype=dtype)
    cols = {"actions": mean.clone(), "old_dist": torch.zeros(4, 2, dtype=dtype),
            "old_logp": -0.5 * math.log(2 * math.pi) - torch.log(ratios), "advantages": torch.ones(4, dtype=dtype),
            "value_targets": y, "vf_preds": value - torch.tensor([1.0, -1.0, 0.25, 0.0], dtype=dtype)}
    cfg = types.SimpleNamespace(clip_param=0.2, vf_clip_param=0.5, vf_loss_coeff=1.0, kl_coeff=0.0, entropy_coeff=0.0)
    return mean, ls, value, cols, cfg


def test_known_answer():
    mean, ls, value, cols, cfg = hand_case()
    d = P.learner_diag_torch(mean, ls, value, cfg=cfg, **cols)
    # Var(y) = (1 + 4 + 9 + 36) / 4 - 9 = 3.5, Var(y - v) = 1 - 0 = 1
    assert abs(float(d[0]) - (1 - 1 / 3.5)) < 1e-12
    assert float(d[1]) == 0.5 and float(d[2]) == 0.5
    assert abs(float(d[3]) - 0.5) < 1e-12
    # the quotient is the same with torch.var's n - 1
    y, e = cols["value_targets"], cols["value_targets"] - value
    assert abs(float(1 - e.var(unbiased=True) / y.var(unbiased=True)) - float(d[0])) < 1e-12
    # one row, and constant targets: exactly -1
    one = P.learner_diag_torch(mean[:1], ls[:1], value[:1], cfg=cfg, **{k: v[:1] for k, v in cols.items()})
    assert float(one[0]) == -1.0 and float(one[1]) == 1.0 and float(one[3]) == 0.5
    const = dict(cols, value_targets=torch.full((4,), 7.25, dtype=torch.float64))
    assert float(P.learner_diag_torch(mean, ls, value, cfg=cfg, **const)[0]) == -1.0
    # a residual larger than the targets' spread stops at the floor
    assert float(P.learner_diag_torch(mean, ls, 100 * value, cfg=cfg, **cols)[0]) == -1.0
    assert P.DIAG == ("vf_explained_var", "clip_frac", "vf_clip_frac", "ratio_max_dev", "grad_gnorm") and P.PPO_DIAG == 8


def test_float32_restatement_of_the_head_cases():
    worst, min_var, runs, floor = D.head_restatement()
    print("vf_explained_var, float32 against float64: worst %.3g, min Var(y) %.3g, %d runs, %d on the floor" % (worst, min_var, runs, floor))
    assert runs == 150
    assert worst <= 1e-5
    assert floor <= D.FLOOR_CAP * runs, "more than 10 %% of the runs sit on the -1 floor, where a comparison shows little"


def test_offset_targets_need_the_pivot():
    for rows in (2, 33, 256):
        mean, ls, value, cols, cfg = D.offset_case(rows)
        got = P.learner_diag_torch(mean, ls, value, cfg=cfg, **cols)
        want = P.learner_diag_torch(mean.double(), ls.double(), value.double(), cfg=cfg, **{k: v.double() for k, v in cols.items()})
        raw = D.raw_sums_explained_var(value, cols["value_targets"])
        print(rows, "pivoted %.3g raw %.3g" % (abs(float(got[0]) - float(want[0])), abs(raw - float(want[0]))))
        assert float(want[0]) > -1.0 and abs(float(got[0]) - float(want[0])) <= 1e-6
        assert abs(raw - float(want[0])) > 1e-4                           # (the case does tell the two apart)


def test_every_row_of_every_head_run_is_off_the_kinks():
    for k, kind, rows, _, idx in D.all_head_runs():
        D.assert_kink_free(k, kind, idx)
    for (k, kind) in F.HEAD_SEEDS:                                         # neither fraction is trivially 0 at 256 rows
        cov = coverage(*F.head_case(k, kind))
        assert cov["above"] >= 0.10 and cov["below"] >= 0.10 and cov["vclip_active"] >= 0.10
    for rows in F.WAVE_CAP_ROWS:
        D.assert_kink_free(F.WAVE_CAP_K, F.WAVE_CAP_KIND, F.wave_cap_index(rows))


def test_counts_of_the_float32_restatement_are_exact():
    for k, kind, rows, _, idx in D.all_head_runs():
        a, b = D.head_diag(k, kind, idx, torch.float32).double(), D.head_diag(k, kind, idx, torch.float64)
        for i in (1, 2):
            assert round(float(a[i]) * rows) == round(float(b[i]) * rows), (k, kind, rows, i)


def test_learner_info():
    cfg = P.PPOConfig(kl_coeff=0.3, entropy_coeff=0.01, lr=2e-4)
    stats = torch.tensor([[1.0, 2.0, 3.0, 4.0, 5.0], [3.0, 2.0, 1.0, 0.0, -1.0]])
    diag = torch.zeros(2, P.PPO_DIAG)
    diag[0, :5] = torch.tensor([0.5, 0.25, 0.0, 0.125, 2.0])
    diag[1, :5] = torch.tensor([-1.0, 0.75, 0.5, 0.75, 4.0])
    info = P.learner_info(stats, diag, cfg)
    assert set(info) == {"total_loss", "policy_loss", "vf_loss", "vf_explained_var", "kl", "entropy", "cur_kl_coeff", "cur_lr",
                         "entropy_coeff", "clip_frac", "vf_clip_frac", "grad_gnorm", "ratio_max_dev"}
    assert info["total_loss"] == 2.0 and info["policy_loss"] == 2.0 and info["vf_loss"] == 2.0 and info["kl"] == 2.0 and info["entropy"] == 2.0
    assert info["vf_explained_var"] == -0.25 and info["clip_frac"] == 0.5 and info["vf_clip_frac"] == 0.25 and info["grad_gnorm"] == 3.0
    assert info["ratio_max_dev"] == 0.75                                    # the max over the steps, not the mean
    assert info["cur_kl_coeff"] == 0.3 and info["cur_lr"] == 2e-4 and info["entropy_coeff"] == 0.01
    with pytest.raises(AssertionError):
        P.learner_info(stats, diag[:1], cfg)


def test_update_kl_coeff():
    assert P.update_kl_coeff(0.2, 0.021) == pytest.approx(0.3)              # above 2 * target
    assert P.update_kl_coeff(0.2, 0.004) == pytest.approx(0.1)              # below 0.5 * target
    assert P.update_kl_coeff(0.2, 0.01) == 0.2
    assert P.update_kl_coeff(0.2, 0.02) == 0.2 and P.update_kl_coeff(0.2, 0.005) == 0.2        # the two boundaries stay
    assert P.update_kl_coeff(0.2, 0.5, kl_target=1.0) == pytest.approx(0.2)
    assert P.update_kl_coeff(0.2, 0.4, kl_target=1.0) == pytest.approx(0.1)
    assert P.update_kl_coeff(0.0, 1.0) == 0.0


def test_diag_buffer_and_gnorm():
    cfg = P.PPOConfig(sgd_minibatch_size=16, num_sgd_iter=2)
    buf = P.diag_buffer(33, cfg, "cpu")
    assert tuple(buf.shape) == (P.dp_steps(33, 16, 2), P.PPO_DIAG) == (6, 8) and buf.dtype == torch.float32
    assert float(buf.abs().max()) == 0.0
    g = [torch.tensor([3.0, 0.0]), torch.tensor([[4.0]], dtype=torch.float64)]
    assert float(P.grad_gnorm_torch(g)) == 5.0


def test_check_diag_names_what_it_got_and_what_it_wants():
    from physicsvae_amd import engine_ppo as E
    E.check_diag(torch.zeros(6, 8), 6, "cpu")
    for bad in (torch.zeros(5, 8), torch.zeros(6, 5), torch.zeros(6, 8, dtype=torch.float64), torch.zeros(8, 6).t(), [0.0] * 8):
        with pytest.raises(ValueError) as e:
            E.check_diag(bad, 6, "cpu")
        assert "[>= 6, 8] on cpu" in str(e.value) and "got" in str(e.value)


def test_abi_refusals():
    """What the new entry points refuse on the host: null handles, a missing or misaligned scratch, too few bytes, a
    capacity below 1, an SGD call of more steps than the bound rows (nothing is launched: the refusal comes before the first
    step); diag == NULL unbinds with no scratch."""
    from physicsvae_amd.engine import Stack, StackSetEngine
    lib = _lib.load()
    err = lambda: lib.pvae_last_error()                                     # noqa: E731
    fake = lambda i=1: C.c_void_p(0x10000 * i)                              # noqa: E731
    assert lib.pvae_fc_ppo_diag(None, fake(), 4, fake(2), 1 << 20) < 0
    assert lib.pvae_ppo_diag(None, fake(), 4, fake(2), 1 << 20) < 0
    assert lib.pvae_fc_ppo_diag_bytes(None, 1) == 0 and lib.pvae_ppo_diag_bytes(None, 1) == 0
    assert lib.pvae_ppo_loss_diag(None, None, 0, None, None, None, 4, None, None, None, None, None, None, None) < 0
    cfg = StackSetEngine(22, [(Stack((64, 64), "relu"), 7), (Stack((64, 64), "relu"), 1)], 16, device="cpu").cfg
    need = lib.pvae_fc_ppo_diag_bytes(C.byref(cfg), 6)
    assert need >= 2049 * 8 + 16 * 8 * 4 and need % 16 == 0
    assert lib.pvae_fc_ppo_diag_bytes(C.byref(cfg), 0) == 0 and b"steps" in err()
    ctx = C.c_void_p()
    assert lib.pvae_fc_create(C.byref(cfg), C.byref(ctx)) == 0
    try:
        assert lib.pvae_fc_ppo_diag(ctx, fake(), 0, fake(2), need) < 0 and b"capacity" in err()
        assert lib.pvae_fc_ppo_diag(ctx, fake(), 4, None, need) < 0 and b"scratch" in err()
        assert lib.pvae_fc_ppo_diag(ctx, fake(), 4, C.c_void_p(0x20004), need) < 0 and b"aligned" in err()
        assert lib.pvae_fc_ppo_diag(ctx, fake(), 4, fake(2), need - 16) < 0 and b"too small" in err()
        assert lib.pvae_fc_bind(ctx, fake(5), fake(6), 1 << 30) == 0
        assert lib.pvae_fc_ppo_bind(ctx, fake(1), fake(2), fake(3), fake(4), 1 << 20, fake(7), None, None) == 0
        b = _lib.FcPpoBatch()
        for i, (name, _) in enumerate(_lib.FcPpoBatch._fields_[:7]):
            setattr(b, name, 0x100000 * (i + 1))
        b.n_rows, b.k = 33, 7
        p = P.PPOConfig().params("constant")
        assert lib.pvae_fc_ppo_diag(ctx, fake(8), 5, fake(2), need) == 0
        assert lib.pvae_fc_ppo_sgd(ctx, C.byref(b), None, 16, 2, C.byref(p), fake(9), None) < 0 and b"6 steps" in err() and b"5 rows" in err()
        assert lib.pvae_fc_ppo_diag(ctx, None, 0, None, 0) == 0
    finally:
        lib.pvae_fc_destroy(ctx)
