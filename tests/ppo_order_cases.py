"""Cases of the minibatch-order tests (tests/test_ppo_order_cpu.py, tests/test_gpu_ppo_order.py; the rule:
physicsvae_amd/ppo.py's module docstring, include/pvae.h "Minibatch order of the PPO learner").

`pvae_ppo_order` changes form at the sizes its head comment in csrc/pvae_ppo_core.hip states -- the GPU tests take each at
n - 1, n and n + 1:
  * 256, 512, 1024, 2048, 4096: the LDS network's padded size (max(256, next power of two)) and with it its stage count;
  * 8192: one workgroup in LDS against tiles + merge launches through the scratch (at 8193 the last tile holds ONE row);
  * 16384, 32768, 65536: the number of merge launches (1 -> 2 -> 3 -> 4);
  * 24576: 3 -> 4 tiles, the smallest odd run count (a run without a sibling is copied) against an even one.
Every n that is no multiple of 8192 has a partial last tile."""
import functools

import numpy as np

from physicsvae_amd import ppo as P

TILE = 8192                                   # kOrderTile
SEED, OFFSET = 1234, 1                        # where the randomness figures of test_ppo_order_cpu.py were measured
SMALL = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 4097, 6250)
SWITCH = (256, 512, 1024, 2048, 4096, 8192, 16384, 24576, 32768, 65536)
SIZES = tuple(sorted(set(SMALL) | {n + d for n in SWITCH for d in (-1, 0, 1)}))
PASSES = (1, 3)
HIGH_SEED, HIGH_OFFSET = (0xDEADBEEF << 32) | 1234, (7 << 32) | 1       # non-zero high words
# (n_rows, num_sgd_iter, seed, offset)
CASES = [(n, p, SEED, OFFSET) for n in SIZES for p in PASSES] + [
    (50000, 20, SEED, OFFSET),                                            # a single learner's batch: equal 32-bit keys occur
    (6250, 3, HIGH_SEED, HIGH_OFFSET), (20000, 2, HIGH_SEED, HIGH_OFFSET)]
LAUNCHES = lambda n: 1 + max(0, int(np.ceil(np.log2(-(-n // TILE)))))     # noqa: E731


def case_id(case):
    return "n%d-p%d-s%x-o%x" % case


@functools.lru_cache(maxsize=None)
def oracle(n_rows, num_sgd_iter, seed, offset):
    """`ppo.minibatch_order`, computed once per case and shared (read-only)."""
    order = P.minibatch_order(n_rows, num_sgd_iter, seed, offset)
    order.setflags(write=False)
    return order


def equal_keys(n_rows, num_sgd_iter, seed, offset):
    """Rows whose 32-bit key another row of the same pass holds too: where the tie-break by row decides."""
    key32 = P.minibatch_keys(n_rows, num_sgd_iter, seed, offset) >> np.uint64(32)
    return sum(n_rows - len(np.unique(key32[p])) for p in range(num_sgd_iter))
