"""Gradient exchange between workers inside the fused PPO learners (include/pvae.h "Gradient exchange between workers",
physicsvae_amd/ppo.py), the parts that need no GPU: the new entry points are declared, exported and bound at ABI 12; bad or
unbound arguments are negative codes that touch no GPU; an unopened exchange reports world 0; `dp_mean_torch` is the
rank-order float32 formula; in float64 the mean of equal shards' gradients is the gradient of the concatenated minibatch,
and with unequal shards it is the mean of the workers' means, not the row-weighted mean; `dp_steps` and the error that names
the ranks."""
import ctypes as C
import os
import re

import pytest
import torch

from physicsvae_amd import _lib
from physicsvae_amd import ppo as P
from ppo_cases import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"pvae_fc_ppo_grad", "pvae_fc_ppo_apply", "pvae_ppo_grad", "pvae_ppo_apply",
       "pvae_fc_ppo_peer_export", "pvae_fc_ppo_peer_open", "pvae_fc_ppo_peer_close", "pvae_fc_ppo_peer_status",
       "pvae_ppo_peer_export", "pvae_ppo_peer_open", "pvae_ppo_peer_close", "pvae_ppo_peer_status"}


def fake(n=1):
    """An aligned non-null address that the argument checks never dereference."""
    return C.c_void_p(0x10000 * n)


def fc_config(max_batch=8, k=54):
    cfg = _lib.FcConfig()
    cfg.n_in, cfg.n_stacks, cfg.max_batch = 20, 2, max_batch
    for s, n_out in enumerate((k, 1)):
        cfg.depth[s], cfg.n_out[s] = 2, n_out
        for i in range(2):
            cfg.width[s][i], cfg.act[s][i] = 32, 1
    return cfg


def full_batch(n_rows=8, k=54):
    b = _lib.FcPpoBatch()
    for i, (name, _) in enumerate(_lib.FcPpoBatch._fields_[:7]):
        setattr(b, name, 0x100000 * (i + 1))
    b.n_rows, b.k = n_rows, k
    return b


def test_new_symbols_are_declared_exported_and_bound_at_abi_12():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "pvae.h")).read()
    stripped = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pvae_[a-z0-9_]+)\s*\(", stripped))
    assert NEW <= declared and NEW <= set(_lib.EXPORTS) and declared == set(_lib.EXPORTS)
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.pvae_abi_version() == _lib.ABI_VERSION == 12 and "#define PVAE_ABI_VERSION 12" in header
    # the spec lines the header cites for a feature that has no reference counterpart
    assert "loco_imitation.yaml:1,35" in header and "loco_runtime_physics_vae.yaml:1,36" in header


def test_null_and_unbound_arguments_are_negative_codes_and_touch_no_gpu():
    lib = _lib.load()
    err = lambda: lib.pvae_last_error()                         # noqa: E731
    p, b = P.PPOConfig().params("state_independent"), full_batch()
    blob = C.create_string_buffer(_lib.P2P_BLOB_BYTES)
    # null contexts
    assert lib.pvae_fc_ppo_grad(None, C.byref(b), None, 0, 4, C.byref(p), fake(), fake(2), None) < 0 and b"null" in err()
    assert lib.pvae_fc_ppo_apply(None, C.byref(p), 1.0, fake(), None) < 0 and b"null" in err()
    assert lib.pvae_ppo_grad(None, C.byref(b), None, 0, 4, C.byref(p), None, 1, 0, 0, fake(), fake(2), None) < 0
    assert lib.pvae_ppo_apply(None, C.byref(p), 1.0, fake(), None) < 0
    for name in ("pvae_fc_ppo_peer_export", "pvae_ppo_peer_export"):
        assert getattr(lib, name)(None, blob) < 0, name
    for name in ("pvae_fc_ppo_peer_open", "pvae_ppo_peer_open"):
        assert getattr(lib, name)(None, 0, 1, blob) < 0, name
    for name in ("pvae_fc_ppo_peer_close", "pvae_ppo_peer_close"):
        assert getattr(lib, name)(None) < 0, name
    for name in ("pvae_fc_ppo_peer_status", "pvae_ppo_peer_status"):
        assert getattr(lib, name)(None, None, None, None, None) < 0, name
    # a stack set that exists but is not bound, then bound without the PPO buffers, then fully bound
    ctx = C.c_void_p()
    assert lib.pvae_fc_create(C.byref(fc_config()), C.byref(ctx)) == 0
    try:
        grad = lambda bb, pp, st=fake(9), ls=fake(8): lib.pvae_fc_ppo_grad(ctx, bb, None, 0, 4, pp, st, ls, None)   # noqa: E731
        assert grad(C.byref(b), C.byref(p)) == -2 and b"pvae_fc_bind" in err()
        assert lib.pvae_fc_ppo_apply(ctx, C.byref(p), 1.0, fake(), None) == -2 and b"pvae_fc_bind" in err()
        assert lib.pvae_fc_ppo_peer_export(ctx, blob) == -2 and b"pvae_fc_ppo_bind" in err()
        assert lib.pvae_fc_ppo_peer_open(ctx, 0, 1, blob) == -2
        assert lib.pvae_fc_bind(ctx, fake(5), fake(6), 1 << 30) == 0
        assert grad(C.byref(b), C.byref(p)) == -2 and b"pvae_fc_ppo_bind" in err()
        assert lib.pvae_fc_ppo_apply(ctx, C.byref(p), 1.0, fake(), None) == -2 and b"pvae_fc_ppo_bind" in err()
        assert lib.pvae_fc_ppo_bind(ctx, fake(1), fake(2), fake(3), fake(4), 1 << 20, fake(7), fake(10), fake(11)) == 0
        assert grad(None, C.byref(p)) < 0 and grad(C.byref(b), None) < 0
        assert grad(C.byref(b), C.byref(p), st=None) < 0 and b"stats_out" in err()
        assert grad(C.byref(b), C.byref(p), ls=None) < 0 and b"ls_grad" in err()         # a trained vector needs its slot
        assert lib.pvae_fc_ppo_grad(ctx, C.byref(b), None, 6, 4, C.byref(p), fake(9), fake(8), None) < 0      # rows past the batch
        assert lib.pvae_fc_ppo_apply(ctx, None, 1.0, fake(), None) < 0
        assert lib.pvae_fc_ppo_apply(ctx, C.byref(p), 1.0, None, None) < 0 and b"ls_grad" in err()
        q = P.PPOConfig().params("state_independent", adam_t=0)
        assert lib.pvae_fc_ppo_apply(ctx, C.byref(q), 1.0, fake(), None) < 0 and b"adam_t" in err()
        q = P.PPOConfig().params("state_dependent")
        assert lib.pvae_fc_ppo_apply(ctx, C.byref(q), 1.0, None, None) < 0 and b"log_std_kind" in err()
        q = P.PPOConfig().params("constant", train_mask=4)
        assert lib.pvae_fc_ppo_apply(ctx, C.byref(q), 1.0, None, None) < 0 and b"train_mask" in err()
        assert lib.pvae_fc_ppo_peer_export(ctx, None) < 0 and lib.pvae_fc_ppo_peer_open(ctx, 0, 1, None) < 0
        assert lib.pvae_fc_ppo_peer_open(ctx, 0, 1, blob) == -2 and b"export first" in err()
        assert lib.pvae_fc_ppo_peer_open(ctx, 1, 1, blob) < 0 and lib.pvae_fc_ppo_peer_open(ctx, 0, 9, blob) < 0
        n = C.c_int32(-1)
        assert lib.pvae_fc_ppo_launches(ctx, C.byref(n)) == 0 and n.value == 0          # nothing was launched
    finally:
        lib.pvae_fc_destroy(ctx)


def test_status_of_an_unopened_exchange_reports_world_zero():
    lib = _lib.load()
    ctx = C.c_void_p()
    assert lib.pvae_fc_create(C.byref(fc_config()), C.byref(ctx)) == 0
    try:
        r, w, t = C.c_int(7), C.c_int(7), C.c_uint32(7)
        assert lib.pvae_fc_ppo_peer_status(ctx, C.byref(r), C.byref(w), C.byref(t), None) == 0
        assert (r.value, w.value, t.value) == (0, 0, 0)
        assert lib.pvae_fc_ppo_peer_close(ctx) == 0                                      # closing what is not open is no error
    finally:
        lib.pvae_fc_destroy(ctx)
    cfg = _lib.Config(13, 5, 3, 64, 2, 64, 3, 32, 2, 64, 1)
    assert lib.pvae_create(C.byref(cfg), C.byref(ctx)) == 0
    try:
        r, w, t = C.c_int(7), C.c_int(7), C.c_uint32(7)
        assert lib.pvae_ppo_peer_status(ctx, C.byref(r), C.byref(w), C.byref(t), None) == 0
        assert (r.value, w.value, t.value) == (0, 0, 0)
        blob = C.create_string_buffer(_lib.P2P_BLOB_BYTES)
        assert lib.pvae_ppo_peer_export(ctx, blob) == -2 and b"pvae_ppo_bind" in lib.pvae_last_error()
        assert lib.pvae_ppo_peer_open(ctx, 0, 1, blob) == -2
        p = P.PPOConfig().params("constant")
        assert lib.pvae_ppo_apply(ctx, C.byref(p), 1.0, None, None) == -2
        assert lib.pvae_ppo_grad(ctx, C.byref(full_batch(k=5)), None, 0, 4, C.byref(p), None, 1, 0, 0, fake(), None, None) == -2
    finally:
        lib.pvae_destroy(ctx)


def test_dp_mean_torch_is_the_rank_order_float32_formula():
    # three ranks where float32 order matters: (1 + 2^-24) rounds back to 1 (ties to even), so ((g0 + g1) + g2) = 1, while
    # g0 + (g1 + g2) = 1 + 2^-23; by hand: 1 * float32(1/3)
    e = 2.0 ** -24
    g = [torch.tensor([1.0, 3.0], dtype=torch.float32), torch.tensor([e, 1.0], dtype=torch.float32),
         torch.tensor([e, -1.0], dtype=torch.float32)]
    third = torch.tensor(1.0 / 3.0, dtype=torch.float32)
    got = P.dp_mean_torch(g)
    assert got.dtype == torch.float32
    assert torch.equal(got, torch.stack([torch.tensor(1.0) * third, torch.tensor(3.0) * third]))
    other_order = (g[0] + (g[1] + g[2])) * third
    assert float(other_order[0]) != float(got[0])                # the case does tell the orders apart
    assert float(got[0]) == float(third)
    # one rank: g_0 bit for bit (also a negative zero and a denormal), and a new tensor
    one = torch.tensor([-0.0, 1e-41, 3.25, float("inf")], dtype=torch.float32)
    got = P.dp_mean_torch([one])
    assert torch.equal(got.view(torch.int32), one.view(torch.int32)) and got.data_ptr() != one.data_ptr()
    # two ranks: the sum then an exact halving
    a, b = torch.randn(1000, generator=torch.Generator().manual_seed(1)), torch.randn(1000, generator=torch.Generator().manual_seed(2))
    assert torch.equal(P.dp_mean_torch([a, b]), (a + b) * 0.5)


def shard_grads(cur, batch, cfg, bounds):
    """d total / d (mean, value, log-std vector) of `ppo_loss_torch` on the rows [lo, hi) of every shard, float64."""
    out = []
    for lo, hi in bounds:
        mean = cur["mean"][lo:hi].clone().requires_grad_(True)
        value = cur["value"][lo:hi].clone().requires_grad_(True)
        vec = cur["log_std"][0].clone().requires_grad_(True)
        total, _ = P.ppo_loss_torch(mean, vec.reshape(1, -1).expand(hi - lo, -1), value, cfg=cfg,
                                    **{k: v[lo:hi] for k, v in batch.items()})
        total.backward()
        out.append((mean.grad, value.grad, vec.grad))
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_equal_shards_mean_of_shard_gradients_is_the_gradient_of_the_concatenated_minibatch(world):
    rows = 24 * world
    cur, batch, cfg = make_case(rows, 5, 11, kind="state_independent", vf_clip_param=0.7, kl_coeff=0.3, entropy_coeff=0.01)
    bounds = [(r * 24, (r + 1) * 24) for r in range(world)]
    whole = shard_grads(cur, batch, cfg, [(0, rows)])[0]
    parts = shard_grads(cur, batch, cfg, bounds)
    # per-row gradients: a shard's are those of the whole minibatch scaled by rows / shard rows; the vector's: the mean
    for i in (0, 1):
        got = torch.cat([g[i] for g in parts]) / world
        assert torch.allclose(got, whole[i], rtol=1e-12, atol=1e-15)
    got = P.dp_mean_torch([g[2] for g in parts])
    assert got.dtype == torch.float64 and torch.allclose(got, whole[2], rtol=1e-12, atol=1e-15)


def test_unequal_shards_give_the_mean_of_means_not_the_row_weighted_mean():
    cur, batch, cfg = make_case(40, 5, 12, kind="state_independent", vf_clip_param=0.7, kl_coeff=0.3, entropy_coeff=0.01)
    bounds = [(0, 30), (30, 40)]
    whole = shard_grads(cur, batch, cfg, [(0, 40)])[0][2]                 # the row-weighted mean
    parts = [g[2] for g in shard_grads(cur, batch, cfg, bounds)]
    got = P.dp_mean_torch(parts)
    assert torch.allclose(got, 0.5 * parts[0] + 0.5 * parts[1], rtol=1e-14, atol=0)
    weighted = 0.75 * parts[0] + 0.25 * parts[1]
    assert torch.allclose(weighted, whole, rtol=1e-12, atol=1e-15)
    assert float((got - whole).abs().max()) > 1e-3 * float(whole.abs().max())        # and the two are not the same thing


def test_dp_steps_and_the_error_that_names_the_ranks():
    assert P.dp_steps(131, 64, 2) == 6 and P.dp_steps(128, 64, 2) == 4 and P.dp_steps(1, 64, 1) == 1
    assert P.dp_steps(150, 64, 1) == 3 and P.dp_steps(64, 64, 30) == 30
    assert P.dp_check_steps([131, 185], 64, 2) == 6                       # different rows (last minibatches 3 and 57), the same steps
    with pytest.raises(ValueError, match=r"rank\(s\) 1 "):
        P.dp_check_steps([131, 121], 64, 2)                               # 64 + 64 + 3 against 64 + 57: three steps a pass, and two
    assert P.dp_check_steps([150], 64, 1) == 3
    with pytest.raises(ValueError, match=r"rank\(s\) 1, 3 ") as info:
        P.dp_check_steps([131, 64, 150, 200], 64, 2)
    assert "[131, 64, 150, 200]" in str(info.value) and "[6, 2, 6, 8]" in str(info.value)
    from physicsvae_amd.parallel import PPODataParallel
    dp = PPODataParallel(0, 1, transport="torch")
    cfg = P.PPOConfig(sgd_minibatch_size=64, num_sgd_iter=2)
    assert dp.check_steps(131, cfg, "cpu") == 6
    with pytest.raises(ValueError, match="transport"):
        PPODataParallel(0, 1, transport="rccl")
