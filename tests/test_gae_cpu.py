"""Train-batch preparation for the PPO learner (include/pvae.h "Train-batch preparation", physicsvae_amd/ppo.py), the parts
that need no GPU: the header, the binding and the library name the same symbols and agree on the struct sizes; bad
arguments are negative codes with messages; the torch restatement of GAE equals a per-row Python loop in float64; the
standardisation's floor; the config's new keys; the segment table from RLlib's columns."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from physicsvae_amd import _lib
from physicsvae_amd import ppo as P
from physicsvae_amd.engine import Stack, StackSetEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAE_NAMES = {"pvae_gae", "pvae_fc_ppo_evaluate", "pvae_fc_ppo_prepare", "pvae_fc_gae_workspace_bytes", "pvae_fc_gae_launches",
             "pvae_gae_sizeof"}
STRUCTS = (("pvae_gae_params", _lib.GaeParams), ("pvae_fc_rollout", _lib.FcRollout), ("pvae_fc_prepared", _lib.FcPrepared))


def test_header_binding_and_library_name_the_gae_symbols():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "pvae.h")).read()
    for name, _ in STRUCTS:
        assert "typedef struct %s" % name in header
    stripped = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pvae_[a-z0-9_]+)\s*\(", stripped))
    assert GAE_NAMES <= declared and GAE_NAMES <= set(_lib.EXPORTS)
    assert declared == set(_lib.EXPORTS)
    for name in GAE_NAMES:
        assert hasattr(lib, name), name
    assert lib.pvae_abi_version() == _lib.ABI_VERSION == 12 and "#define PVAE_ABI_VERSION 12" in header
    # the PPO step's structs and their self-check are as they were
    assert lib.pvae_fc_ppo_sizeof(0) == C.sizeof(_lib.FcPpoParams) and lib.pvae_fc_ppo_sizeof(2) < 0


def test_ctypes_structs_have_the_sizes_the_library_sees():
    lib = _lib.load()
    for which, (_, cls) in enumerate(STRUCTS):
        assert lib.pvae_gae_sizeof(which) == C.sizeof(cls), cls
    assert lib.pvae_gae_sizeof(3) < 0 and lib.pvae_gae_sizeof(-1) < 0


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_ctypes_structs_have_the_sizes_a_c_compiler_sees(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "pvae.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(pvae_gae_params), sizeof(pvae_fc_rollout), '
                   'sizeof(pvae_fc_prepared), __builtin_offsetof(pvae_gae_params, log_std_base), '
                   '__builtin_offsetof(pvae_fc_rollout, n_rows), __builtin_offsetof(pvae_fc_rollout, seg_last)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I", os.path.join(ROOT, "include"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.GaeParams), C.sizeof(_lib.FcRollout), C.sizeof(_lib.FcPrepared),
                   _lib.GaeParams.log_std_base.offset, _lib.FcRollout.n_rows.offset, _lib.FcRollout.seg_last.offset]


def test_scratch_size_query():
    lib = _lib.load()
    sizes = [lib.pvae_fc_gae_workspace_bytes(s) for s in (1, 4, 5, 1000, 4096, 100000)]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[0] == sizes[1] == 16 and sizes[2] == 32                    # two doubles per workgroup of four segments
    assert sizes[-1] == sizes[-2]                                          # capped: the waves stride over the segments
    assert lib.pvae_fc_gae_workspace_bytes(0) == 0 and b"n_segs" in lib.pvae_last_error()


def fake(n=1):
    """An aligned non-null address that the argument checks never dereference."""
    return C.c_void_p(0x10000 * n)


def fc_config(max_batch, stacks=(((32, 32), 6), ((32, 32), 1))):
    return StackSetEngine(22, [(Stack(w, "relu"), n) for w, n in stacks], max_batch, device="cpu").cfg


def full_rollout(n_rows=10, n_segs=3, k=6, sampler=False):
    r = _lib.FcRollout()
    for i, (name, _) in enumerate(_lib.FcRollout._fields_[:9 if sampler else 6]):
        setattr(r, name, 0x100000 * (i + 1))
    r.n_rows, r.n_segs, r.k, r.seg_first, r.seg_last = n_rows, n_segs, k, 0, n_rows
    return r


def full_out():
    o = _lib.FcPrepared()
    for i, (name, _) in enumerate(_lib.FcPrepared._fields_):
        setattr(o, name, 0x1000000 * (i + 1))
    return o


def test_bad_arguments_are_negative_codes_with_messages_and_launch_nothing():
    lib = _lib.load()
    err = lambda: lib.pvae_last_error()                         # noqa: E731
    p = P.PPOConfig(gamma=0.98, lambda_=0.95).gae_params("constant")
    # the dense form
    def dense(n_rows=10, n_segs=3, first=0, last=10, pp=C.byref(p), rewards=fake(1), adv=fake(6), scratch=fake(8), nbytes=1 << 14):
        return lib.pvae_gae(rewards, fake(2), fake(3), fake(4), fake(5), n_rows, n_segs, first, last, pp, adv, fake(7), scratch,
                            nbytes, None)
    assert dense(pp=None) < 0 and b"null params" in err()
    assert dense(rewards=None) < 0 and b"null" in err()
    assert dense(adv=None) < 0 and b"output" in err()
    assert dense(n_rows=0, last=0) < 0 and b"n_rows" in err()
    assert dense(n_segs=0) < 0 and b"n_segs must be >= 1" in err()
    assert dense(n_segs=11) < 0 and b"at least one row" in err()
    assert dense(first=1) < 0 and b"seg_start must run from 0 to n_rows" in err()
    assert dense(last=9) < 0 and b"seg_start must run from 0 to n_rows" in err()
    assert dense(scratch=None) < 0 and b"scratch is null" in err()
    assert dense(scratch=C.c_void_p(0x10008)) < 0 and b"aligned" in err()
    assert dense(nbytes=8) < 0 and b"scratch too small" in err()
    for field, value in (("gamma", 1.5), ("gamma", -0.1), ("lambda_", 2.0), ("gamma", float("nan"))):
        q = P.PPOConfig().gae_params("constant")
        setattr(q, field, value)
        assert dense(pp=C.byref(q)) < 0 and b"gamma and lambda" in err(), field
    # on a stack set
    ro, out = full_rollout(), full_out()
    assert lib.pvae_fc_ppo_prepare(None, C.byref(ro), C.byref(p), C.byref(out), fake(8), 1 << 14, None) < 0 and b"null stack set" in err()
    ctx = C.c_void_p()
    assert lib.pvae_fc_create(C.byref(fc_config(64)), C.byref(ctx)) == 0
    try:
        def prep(r=ro, pp=p, o=out, scratch=fake(8), nbytes=1 << 14):
            return lib.pvae_fc_ppo_prepare(ctx, C.byref(r) if r is not None else None, C.byref(pp) if pp is not None else None,
                                           C.byref(o) if o is not None else None, scratch, nbytes, None)

        def evaluate(r=ro, pp=p, o=out):
            return lib.pvae_fc_ppo_evaluate(ctx, C.byref(r) if r is not None else None, C.byref(pp), C.byref(o), None)
        assert prep() == -2 and b"pvae_fc_bind" in err()
        assert evaluate() == -2 and b"pvae_fc_bind" in err()
        assert lib.pvae_fc_bind(ctx, fake(5), fake(6), 1 << 30) == 0
        assert prep() == -2 and b"log_std vector not bound" in err()                  # the unbound buffer
        assert evaluate() == -2 and b"log_std vector not bound" in err()
        assert lib.pvae_fc_ppo_bind(ctx, fake(1), fake(2), fake(3), fake(4), 1 << 20, fake(7), None, None) == 0
        assert prep(r=None) < 0 and prep(pp=None) < 0 and prep(o=None) < 0
        assert evaluate(r=None) < 0 and b"null" in err()
        for field, value, msg in (("n_segs", 0, b"n_segs must be >= 1"), ("seg_first", 2, b"seg_start must run from 0"),
                                  ("seg_last", 11, b"seg_start must run from 0"), ("n_rows", 0, b"n_rows"),
                                  ("k", 5, b"rollout k 5"), ("obs", None, b"obs or actions"), ("rewards", None, b"rewards"),
                                  ("seg_start", None, b"seg_start"), ("seg_done", None, b"boot_obs or seg_done"),
                                  ("boot_obs", None, b"boot_obs or seg_done")):
            r = full_rollout()
            setattr(r, field, value)
            assert prep(r=r) < 0 and msg in err(), (field, err())
        r = full_rollout(sampler=True)
        r.old_logp = None
        assert prep(r=r) < 0 and b"all three or none" in err()
        for field, msg in (("vf_preds", b"evaluate output"), ("last_value", b"last_value"), ("advantages", b"advantages")):
            o = full_out()
            setattr(o, field, None)
            assert prep(o=o) < 0 and msg in err(), field
        assert prep(scratch=None) < 0 and b"scratch is null" in err()
        assert prep(nbytes=8) < 0 and b"scratch too small" in err()
        for kind, msg in ((3, b"log_std_kind"), (2, b"does not fit 2 stacks")):
            q = P.PPOConfig().gae_params(kind)
            assert prep(pp=q) < 0 and msg in err(), kind
        o = _lib.FcPrepared()
        assert evaluate(o=o) < 0 and b"nothing to compute" in err()
        e, r = C.c_int32(-1), C.c_int32(-1)
        assert lib.pvae_fc_gae_launches(ctx, C.byref(e), C.byref(r)) == 0 and (e.value, r.value) == (0, 0)      # nothing was launched
        assert lib.pvae_fc_gae_launches(None, C.byref(e), C.byref(r)) < 0
    finally:
        lib.pvae_fc_destroy(ctx)
    # stack sets that are not [policy, value(, log-std)]
    for stacks, msg in (((((16,), 6),), b"got 1"), ((((16,), 6), ((16,), 6)), b"wrong order"),
                        ((((16,), 6), ((16,), 1), ((16,), 4)), b"wrong order"),
                        ((((16,), 6), ((16,), 1), ((16,), 6), ((16,), 6)), b"got 4")):
        ctx = C.c_void_p()
        assert lib.pvae_fc_create(C.byref(fc_config(8, stacks)), C.byref(ctx)) == 0
        try:
            assert lib.pvae_fc_bind(ctx, fake(5), fake(6), 1 << 30) == 0
            q = P.PPOConfig().gae_params("state_dependent" if len(stacks) >= 3 else "constant")
            assert lib.pvae_fc_ppo_prepare(ctx, C.byref(ro), C.byref(q), C.byref(out), fake(8), 1 << 14, None) < 0
            assert msg in err(), (stacks, err())
        finally:
            lib.pvae_fc_destroy(ctx)


# ---------------------------------------------------------------------------------------
# the specification
# ---------------------------------------------------------------------------------------
def gae_loop(rewards, vf_preds, last_values, seg_start, gamma, lambda_):
    """The recurrence row by row, in Python floats (float64)."""
    n = len(rewards)
    adv, vt = [0.0] * n, [0.0] * n
    for s in range(len(last_values)):
        nxt_adv, nxt_v = 0.0, float(last_values[s])
        for t in range(int(seg_start[s + 1]) - 1, int(seg_start[s]) - 1, -1):
            delta = float(rewards[t]) + gamma * nxt_v - float(vf_preds[t])
            adv[t] = delta + gamma * lambda_ * nxt_adv
            vt[t] = adv[t] + float(vf_preds[t])
            nxt_adv, nxt_v = adv[t], float(vf_preds[t])
    return torch.tensor(adv, dtype=torch.float64), torch.tensor(vt, dtype=torch.float64)


LENGTHS = (1, 2, 7, 7, 1, 2)
DONE = (True, False, True, False, False, True)                 # lengths 1, 2 and 7, each done and not done


def spec_case(seed=0):
    g = torch.Generator().manual_seed(seed)
    n = sum(LENGTHS)
    rewards = torch.rand(n, generator=g, dtype=torch.float64)
    vf = torch.randn(n, generator=g, dtype=torch.float64)
    last = torch.randn(len(LENGTHS), generator=g, dtype=torch.float64) * (~torch.tensor(DONE)).double()
    seg_start = torch.tensor(np.concatenate([[0], np.cumsum(LENGTHS)]), dtype=torch.int32)
    return rewards, vf, last, seg_start


@pytest.mark.parametrize("gamma,lambda_", [(0.98, 0.95), (0.9, 0.0), (1.0, 1.0), (0.0, 0.7)])
def test_gae_torch_equals_the_per_row_loop(gamma, lambda_):
    rewards, vf, last, seg_start = spec_case()
    adv, vt = P.gae_torch(rewards, vf, last, seg_start, gamma, lambda_)
    want_adv, want_vt = gae_loop(rewards, vf, last, seg_start, gamma, lambda_)
    assert adv.dtype == torch.float64 and float((adv - want_adv).abs().max()) < 1e-13
    assert float((vt - want_vt).abs().max()) < 1e-13
    ends = seg_start[1:].long()
    v_next = torch.cat([vf[1:], vf[:1]])
    v_next[ends - 1] = last
    delta = rewards + gamma * v_next - vf
    if gamma * lambda_ == 0:
        assert float((adv - delta).abs().max()) < 1e-14                               # adv == delta
    if gamma == 1.0 and lambda_ == 1.0:
        for s in range(len(LENGTHS)):                                                 # the plain suffix sum of delta
            a, b = int(seg_start[s]), int(seg_start[s + 1])
            suffix = torch.flip(torch.cumsum(torch.flip(delta[a:b], [0]), 0), [0])
            assert float((adv[a:b] - suffix).abs().max()) < 1e-13
    # any dtype: float32 in, float32 out, close to the float64 result
    a32, v32 = P.gae_torch(rewards.float(), vf.float(), last.float(), seg_start, gamma, lambda_)
    assert a32.dtype == torch.float32 and v32.dtype == torch.float32
    assert float((a32.double() - want_adv).abs().max()) < 1e-5 * float(want_adv.abs().max())


def test_gae_torch_refuses_a_table_that_does_not_cover_the_rows():
    rewards, vf, last, seg_start = spec_case()
    bad = seg_start.clone()
    bad[-1] -= 1
    with pytest.raises(AssertionError, match="seg_start"):
        P.gae_torch(rewards, vf, last, bad, 0.9, 0.9)


def test_standardize_torch_floor_and_moments():
    assert float(P.standardize_torch(torch.tensor([3.25], dtype=torch.float64))) == 0.0      # one row: the 1e-4 floor holds
    assert float(P.standardize_torch(torch.tensor([3.25]))) == 0.0
    x = torch.randn(1000, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 3 + 5
    y = P.standardize_torch(x)
    assert abs(float(y.mean())) < 1e-12 and abs(float(y.std(unbiased=False)) - 1) < 1e-12
    tiny = torch.tensor([1.0, 1.0 + 2e-5], dtype=torch.float64)                              # std 1e-5 < the floor
    assert torch.allclose(P.standardize_torch(tiny), torch.tensor([-0.1, 0.1], dtype=torch.float64), atol=1e-9)


def test_ppo_config_reads_gamma_and_lambda():
    spec = {"clip_param": 0.2, "kl_coeff": 0.0, "vf_clip_param": 1000, "num_sgd_iter": 20, "lr": 0.00002,
            "sgd_minibatch_size": 500, "gamma": 0.98, "lambda": 0.95, "train_batch_size": 100000}
    cfg = P.PPOConfig.from_spec(spec)
    assert (cfg.gamma, cfg.lambda_, cfg.standardize) == (0.98, 0.95, True)
    p = cfg.gae_params("state_dependent", -0.5)
    assert p.gamma == pytest.approx(0.98, rel=1e-7) and p.lambda_ == pytest.approx(0.95, rel=1e-7)
    assert (p.standardize, p.log_std_kind) == (1, 2) and p.log_std_base == -0.5
    d = P.PPOConfig()
    assert (d.gamma, d.lambda_, d.standardize) == (0.99, 1.0, True)                           # RLlib's defaults
    assert P.PPOConfig(standardize=False).gae_params().standardize == 0
    # the positional order of the earlier arguments did not move
    assert P.PPOConfig(0.1, 5.0).vf_clip_param == 5.0 and P.PPOConfig.from_spec({"lr": 1e-3}).gamma == 0.99


def test_segment_table_from_rllib_columns():
    # two fragments: [episode 7: 3 rows, done | episode 8: 2 rows, cut by the fragment end] [episode 8 goes on: 2 rows, done |
    # episode 9: 1 row, truncated at the end of the batch]
    eps_id = np.array([7, 7, 7, 8, 8, 8, 8, 9])
    dones = np.array([0, 0, 1, 0, 0, 0, 1, 0], dtype=bool)
    new_obs = np.arange(8 * 3, dtype=np.float64).reshape(8, 3)
    seg_start, seg_done, nxt = P.segment_table(eps_id, dones, new_obs)
    # (the two fragments of episode 8 are adjacent rows of one episode in time order: one segment)
    assert seg_start.dtype == np.int32 and seg_start.tolist() == [0, 3, 7, 8]
    assert seg_done.dtype == np.uint8 and seg_done.tolist() == [1, 1, 0]
    assert nxt.dtype == np.float32 and nxt.shape == (3, 3) and np.array_equal(nxt, new_obs[[2, 6, 7]].astype(np.float32))
    # with the fragment column, as RLlib postprocesses them: episode 8's first fragment is a truncated segment of its own
    seg_start, seg_done, nxt = P.segment_table(eps_id, dones, new_obs, unroll_id=[0, 0, 0, 0, 0, 1, 1, 1])
    assert seg_start.tolist() == [0, 3, 5, 7, 8] and seg_done.tolist() == [1, 0, 1, 0]
    assert np.array_equal(nxt, new_obs[[2, 4, 6, 7]].astype(np.float32))
    # the same episode id straight after its own done row starts a new segment
    s2, d2, _ = P.segment_table([1, 1, 1, 1], [0, 1, 0, 0], np.zeros((4, 2)))
    assert s2.tolist() == [0, 2, 4] and d2.tolist() == [1, 0]
    s3, d3, n3 = P.segment_table([5], [False], np.ones((1, 2, 2)))
    assert s3.tolist() == [0, 1] and d3.tolist() == [0] and n3.shape == (1, 4)


def test_prepare_needs_a_gpu_and_names_what_is_missing():
    from physicsvae_amd import FullyConnectedPolicy
    from physicsvae_amd.spaces import Box
    m = FullyConnectedPolicy(Box(np.zeros(22), np.zeros(22)), Box(np.zeros(6), np.zeros(6)), 12,
                             {"custom_model_config": {"device": "cpu"}}, "fcnn")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.ppo_prepare({}, P.PPOConfig())
