"""The minibatch order of the PPO learners (`ppo_learn(..., perm="philox")`; the rule: physicsvae_amd/ppo.py's module
docstring, include/pvae.h "Minibatch order of the PPO learner"), the parts that need no GPU: `ppo.minibatch_order`'s own
Philox gives Random123's known answers; every pass is a permutation, a function of its arguments, and another one for
another pass, seed or offset (the high words included); the order at the size of a worker's train batch is within caps a
broken key would not clear; the two entry points are declared, exported and bound at ABI 12 and refuse every bad argument
before any HIP call; the Python surface names the accepted values and has no CPU fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from physicsvae_amd import _lib
from physicsvae_amd import ppo as P
from ppo_order_cases import CASES, LAUNCHES, OFFSET, SEED, SIZES, SWITCH, TILE, equal_keys, oracle
from test_ppo_cpu import fake
from test_ppo_vae_cpu import model as vae_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"pvae_ppo_order_workspace_bytes", "pvae_ppo_order"}


# 1. the rule in numpy
def test_philox_reproduces_the_known_answers():
    # Random123's kat_vectors, philox4x32 10 rounds
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        assert tuple(int(x) for x in P.philox4x32(counter, key)) == want
    # and vectorised over one counter word, as minibatch_keys calls it
    w = P.philox4x32((0, 0, np.arange(3, dtype=np.uint64), 0), (0, 0))
    assert tuple(int(x[0]) for x in w) == kat[0][2] and all(x.shape == (3,) and x.dtype == np.uint64 for x in w)


def test_keys_follow_the_rule_word_by_word():
    n, passes, seed, offset = 11, 2, (5 << 32) | 9, (3 << 32) | 4
    keys = P.minibatch_keys(n, passes, seed, offset)
    assert keys.dtype == np.uint64 and keys.shape == (passes, n)
    for p in range(passes):
        for i in range(n):
            w = P.philox4x32((4, 3, i >> 2, 0xC0000000 + p), (9, 5))
            assert int(keys[p, i]) == (int(w[i & 3]) << 32) | i


@pytest.mark.parametrize("n", [1, 2, 3, 257, 6250])
def test_every_pass_is_a_permutation_and_a_function_of_its_arguments(n):
    order = P.minibatch_order(n, 3, SEED, OFFSET)
    assert order.dtype == np.int32 and order.shape == (3, n)
    for p in range(3):
        assert np.array_equal(np.sort(order[p]), np.arange(n))
    assert np.array_equal(order, P.minibatch_order(n, 3, SEED, OFFSET))
    # a pass does not depend on how many passes are drawn
    assert np.array_equal(order[:2], P.minibatch_order(n, 2, SEED, OFFSET))


def test_pass_seed_and_offset_each_change_the_order():
    n = 6250
    base = P.minibatch_order(n, 3, SEED, OFFSET)
    moved = lambda a, b: float((a != b).mean())                           # noqa: E731
    assert moved(base[0], base[1]) > 0.999 and moved(base[1], base[2]) > 0.999
    others = {"seed + 1": P.minibatch_order(n, 1, SEED + 1, OFFSET), "seed + 2^32": P.minibatch_order(n, 1, SEED + 2 ** 32, OFFSET),
              "offset + 1": P.minibatch_order(n, 1, SEED, OFFSET + 1), "offset + 2^32": P.minibatch_order(n, 1, SEED, OFFSET + 2 ** 32)}
    for what, other in others.items():
        assert moved(base[0], other[0]) > 0.999, what


def test_order_of_a_worker_batch_is_within_the_randomness_caps():
    """Conditions, not measurements: at n = 6250, 20 passes, seed 1234, offset 1 the rule gives 3 fixed points at most,
    |corr| 0.034 between passes and 0.020 with row order, and a first-half share of 0.452 .. 0.554 in the first 500 rows;
    a key that ignored the row, the pass or a counter word would clear none of the caps below."""
    n, passes = 6250, 20
    order = oracle(n, passes, SEED, OFFSET)
    rows = np.arange(n)
    fixed = max(int((order[p] == rows).sum()) for p in range(passes))
    corr = np.corrcoef(np.vstack([order.astype(np.float64), rows.astype(np.float64)]))
    between = float(np.abs(corr[:passes, :passes] - np.eye(passes)).max())
    with_rows = float(np.abs(corr[passes, :passes]).max())
    share = [float((order[p][:500] < n // 2).mean()) for p in range(passes)]
    print("fixed points %d, |corr| between passes %.3f, with row order %.3f, first-half share %.3f .. %.3f"
          % (fixed, between, with_rows, min(share), max(share)))
    assert fixed <= 8 and between <= 0.08 and with_rows <= 0.08 and 0.40 <= min(share) and max(share) <= 0.60
    assert equal_keys(n, passes, SEED, OFFSET) == 0


def test_cases_straddle_every_size_at_which_the_kernels_change_form():
    src = open(os.path.join(ROOT, "physicsvae_amd", "csrc", "pvae_ppo_core.hip")).read()
    assert "constexpr int kOrderTile = %d;" % TILE in src and "constexpr int kOrderMinPad = 256;" in src
    for n in SWITCH:
        assert {n - 1, n, n + 1} <= set(SIZES)
    assert [LAUNCHES(n) for n in (1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 4 * TILE, 4 * TILE + 1, 8 * TILE, 8 * TILE + 1)] == \
        [1, 1, 2, 2, 3, 3, 4, 4, 5]
    assert all(1 <= n < 2 ** 31 and 1 <= p < 2 ** 30 for n, p, _, _ in CASES)


# 2. header and library
def test_new_symbols_are_declared_exported_and_bound_at_abi_12():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "pvae.h")).read()
    assert "Minibatch order of the PPO learner" in header
    stripped = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pvae_[a-z0-9_]+)\s*\(", stripped))
    assert NEW <= declared and NEW <= set(_lib.EXPORTS) and declared == set(_lib.EXPORTS)
    for name in NEW:
        assert hasattr(lib, name), name
    assert re.search(r"size_t\s+pvae_ppo_order_workspace_bytes\(int64_t n_rows, int32_t num_sgd_iter\);", stripped)
    assert re.search(r"int\s+pvae_ppo_order\(int64_t n_rows, int32_t num_sgd_iter, uint64_t seed, uint64_t offset, int32_t\* perm, "
                     r"void\* scratch,\s+size_t scratch_bytes, void\* stream\);", stripped)
    assert lib.pvae_abi_version() == _lib.ABI_VERSION == 12 and "#define PVAE_ABI_VERSION 12" in header
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "%d entry points" % len(declared) in readme


def test_workspace_size_query():
    lib = _lib.load()
    size = lib.pvae_ppo_order_workspace_bytes
    for n, passes, _, _ in CASES:
        got = size(n, passes)
        assert got > 0 and got % 16 == 0
        assert got == (16 if n <= TILE else (2 * passes * n * 8 + 15) // 16 * 16), (n, passes)
    assert size(2 ** 31 - 1, 1) == ((2 ** 31 - 1) * 16 + 15) // 16 * 16
    err = lambda: lib.pvae_last_error()                                    # noqa: E731
    assert size(0, 1) == 0 and b"n_rows" in err()
    assert size(2 ** 31, 1) == 0 and b"n_rows" in err()
    assert size(8, 0) == 0 and b"num_sgd_iter" in err()
    assert size(8, 2 ** 30) == 0 and b"num_sgd_iter" in err()
    assert size(8, 2 ** 30 - 1) == 16
    assert size(2 ** 31 - 1, 2 ** 30 - 1) == 0 and b"size_t" in err()       # 2^65 bytes of packed keys


def test_bad_arguments_are_negative_codes_with_messages_and_touch_no_gpu():
    lib = _lib.load()
    order, err = lib.pvae_ppo_order, lambda: lib.pvae_last_error()          # noqa: E731
    perm, scratch, big = fake(1), fake(2), 1 << 40
    assert order(0, 1, 1, 1, perm, scratch, big, None) < 0 and b"n_rows" in err()
    assert order(-5, 1, 1, 1, perm, scratch, big, None) < 0 and b"n_rows" in err()
    assert order(2 ** 31, 1, 1, 1, perm, scratch, big, None) < 0 and b"n_rows" in err()
    assert order(70, 0, 1, 1, perm, scratch, big, None) < 0 and b"num_sgd_iter" in err()
    assert order(70, 2 ** 30, 1, 1, perm, scratch, big, None) < 0 and b"num_sgd_iter" in err()
    assert order(70, 3, 1, 1, None, scratch, big, None) < 0 and b"perm is null" in err()
    assert order(70, 3, 1, 1, C.c_void_p(0x10002), scratch, big, None) < 0 and b"4-byte aligned" in err()
    assert order(70, 3, 1, 1, perm, None, big, None) < 0 and b"scratch is null" in err()
    assert order(70, 3, 1, 1, perm, C.c_void_p(0x20008), big, None) < 0 and b"16-byte aligned" in err()
    assert order(70, 3, 1, 1, perm, scratch, 15, None) < 0 and b"scratch too small" in err()
    need = lib.pvae_ppo_order_workspace_bytes(TILE + 1, 3)
    assert order(TILE + 1, 3, 1, 1, perm, scratch, need - 1, None) < 0 and b"scratch too small" in err()


# 3. the Python surface
def cpu_policy():
    from physicsvae_amd import FullyConnectedPolicy
    from physicsvae_amd.spaces import Box
    return FullyConnectedPolicy(Box(np.zeros(22), np.zeros(22)), Box(np.zeros(5), np.zeros(5)), 10,
                                {"custom_model_config": {"device": "cpu"}}, "fcnn")


@pytest.mark.parametrize("make", [cpu_policy, vae_model])
def test_an_unknown_order_is_a_value_error_that_names_the_accepted_values(make):
    m = make()
    assert P.ORDERS == ("philox",)
    with pytest.raises(ValueError, match='"philox"') as e:
        m.ppo_learn({}, P.PPOConfig(), perm="sorted")
    assert "'sorted'" in str(e.value)
    assert m._rng_calls == 0


@pytest.mark.parametrize("make", [cpu_policy, vae_model])
def test_philox_order_has_no_cpu_fallback(make):
    m = make()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.ppo_learn({}, P.PPOConfig(sgd_minibatch_size=32), perm="philox")
    assert m._rng_calls == 0
    from physicsvae_amd import engine_ppo
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine_ppo.ppo_order(70, 3, 1, 1, "cpu")
