"""Cases of the stack-set / PPO-learner sweep (tests/test_gpu_fc_shapes.py, checked without a GPU by
tests/test_fc_cases_cpu.py): random and directed stack sets with their float64 twin, PPO step cases, loss-head cases and
the segment tables of the GAE tests.  Everything is built on the CPU from a seed, once (lru_cache), and left unchanged.

The float64 twin reads the kernels' own float32 inputs.  Rows whose smallest |pre-activation| over the ReLU layers is
within RELU_MARGIN of the kink are not used (tests/test_gpu_shapes.py uses the same figure for the same reason: there a
float32 pre-activation may fall on the other side of 0 than the float64 one, and the gradient jumps); PPO step rows within
ppo_cases.KINK of a kink of the loss are not used either.  Each generator draws `2 rows + 8` candidate rows, keeps the
first `rows` good ones and records the fraction it dropped; the CPU test holds that fraction under its cap."""
import functools
import itertools
import math
import types

import torch

from physicsvae_amd import ppo as P
from ppo_cases import KINK, coverage, make_case
from test_gpu_fcnn import ACTS

WIDTHS = (5, 17, 31, 64, 100, 129, 200, 257)
ACT_NAMES = ("relu", "tanh", "sigmoid", "elu", "linear")
N_INS = (1, 3, 22, 63, 64, 65, 130)
N_OUTS = (1, 2, 7, 54, 64, 65, 130)
ROWS = (1, 2, 3, 4, 5, 31, 32, 33, 64, 97, 130, 256)
RELU_MARGIN = 4e-6
STACK_DROP_CAP, PPO_DROP_CAP = 0.05, 0.10
N_RANDOM = 40
KINDS = ("constant", "state_independent", "state_dependent")
# the `SECOND` block of tests/test_gpu_ppo.py: every term of the loss is live
LOSS = dict(clip_param=0.2, vf_clip_param=0.7, kl_coeff=0.3, entropy_coeff=0.01, vf_loss_coeff=0.5)


def pad32(n):
    return (n + 31) // 32 * 32


def pad64(n):
    return (n + 63) // 64 * 64


# ---------------------------------------------------------------------------------------
# the float64 twin of a stack set
# ---------------------------------------------------------------------------------------
def _apply(name, t):
    return t if name == "linear" else ACTS[name]()(t)


def forward_graph(stacks, params, x):
    """Outputs per stack of `stacks` [(widths, acts, n_out)] holding `params` [[(W [n_out, n_in], b)]] on x, in the dtype of
    the operands, and per row the smallest |pre-activation| over all ReLU layers (inf without one)."""
    outs = []
    margin = torch.full((x.shape[0],), math.inf, dtype=x.dtype)
    for (widths, acts, _), layers in zip(stacks, params):
        h = x
        for i, (w, b) in enumerate(layers):
            h = h @ w.T + b
            if i < len(widths):
                if acts[i] == "relu":
                    margin = torch.minimum(margin, h.detach().abs().min(1).values)
                h = _apply(acts[i], h)
        outs.append(h)
    return outs, margin


def leaves(params, dtype):
    return [[(w.to(dtype).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)) for w, b in layers]
            for layers in params]


def twin64(case, x, cots=None, dtype=torch.float64):
    """The stack set of `case` on x in plain torch (`dtype`: float64, or float32 for the restatement's own error):
    .outs per stack, .margin per row and -- with output cotangents `cots` (an entry None: that stack does not run) -- .dx and
    .grads [[(dW, db)]] (None for a stack that did not run) through autograd."""
    params = leaves(case.params, dtype)
    xg = x.to(dtype).clone().requires_grad_(True)
    outs, margin = forward_graph(case.stacks, params, xg)
    res = types.SimpleNamespace(outs=[o.detach() for o in outs], margin=margin, dx=None, grads=None)
    if cots is not None:
        total = sum((o * c.to(dtype)).sum() for o, c in zip(outs, cots) if c is not None)
        total.backward()
        res.dx = xg.grad
        res.grads = [[(w.grad, b.grad) for w, b in layers] if c is not None else None for layers, c in zip(params, cots)]
    return res


# ---------------------------------------------------------------------------------------
# stack-set cases
# ---------------------------------------------------------------------------------------
def draw_params(g, n_in, stacks):
    """Weights randn / sqrt(fan_in), biases 0.1 randn, float32."""
    params = []
    for widths, _, n_out in stacks:
        layers, prev = [], n_in
        for n in tuple(widths) + (n_out,):
            layers.append((torch.randn(n, prev, generator=g) / math.sqrt(prev), 0.1 * torch.randn(n, generator=g)))
            prev = n
        params.append(layers)
    return params


def build_case(name, n_in, stacks, rows, max_batch, seed):
    g = torch.Generator().manual_seed(seed)
    stacks = tuple((tuple(w), tuple(a), int(n)) for w, a, n in stacks)
    case = types.SimpleNamespace(name=name, n_in=n_in, stacks=stacks, rows=rows, max_batch=max_batch, seed=seed)
    case.params = draw_params(g, n_in, stacks)
    cand = torch.randn(2 * rows + 8, n_in, generator=g)
    keep = twin64(case, cand).margin > RELU_MARGIN
    case.dropped = 1.0 - float(keep.double().mean())
    case.x = cand[keep][:rows].contiguous()
    assert case.x.shape[0] == rows, (name, "too few rows off the ReLU kinks")
    case.dys = [torch.randn(rows, n, generator=g) for _, _, n in stacks]
    case.depths = tuple(len(w) for w, _, _ in stacks)
    return case


def draw_stack(g, n_out, depth=None):
    ri = lambda n: int(torch.randint(n, (1,), generator=g))                          # noqa: E731
    depth = depth or 1 + ri(4)
    return (tuple(WIDTHS[ri(len(WIDTHS))] for _ in range(depth)), tuple(ACT_NAMES[ri(len(ACT_NAMES))] for _ in range(depth)),
            n_out)


@functools.lru_cache(maxsize=None)
def stack_case(seed):
    """A random stack set.  The rows cycle through ROWS with the seed (every row count, hence every GEMV instantiation and
    both parities of rows_pad / 64, comes up N_RANDOM / 12 times); every tenth seed is the value stack as PhysicsVAE's
    learner runs it: one stack, one output."""
    g = torch.Generator().manual_seed(1000 + seed)
    ri = lambda n: int(torch.randint(n, (1,), generator=g))                          # noqa: E731
    rows = ROWS[seed % len(ROWS)]
    n_in = N_INS[ri(len(N_INS))]
    if seed % 10 == 0:
        stacks = [draw_stack(g, 1)]
    else:
        stacks = [draw_stack(g, N_OUTS[ri(len(N_OUTS))]) for _ in range(1 + ri(4))]
    max_batch = rows + (0, 1, 30)[ri(3)]
    return build_case("random%d" % seed, n_in, stacks, rows, max_batch, 2000 + seed)


RELU2 = ("relu", "tanh")
GEMV_SET = (((64, 31, 17), ("relu", "elu", "tanh"), 7), ((100,), ("sigmoid",), 1), ((17, 129), ("relu", "relu"), 65))
DIRECTED = {
    # padded first layers 256 + 256 + 192 = 704: (256 / 32)(704 / 32) >= 128, the concatenated GEMM on 32x32 tiles
    "concat32_a": (22, (((200, 64), RELU2, 54), ((200,), ("relu",), 1), ((129, 31), ("elu", "sigmoid"), 7)), 256, 256),
    "concat32_b": (65, (((200,), ("tanh",), 2), ((200, 17), RELU2, 65), ((129,), ("relu",), 1)), 256, 300),
    "concat32_c": (3, (((257, 5), RELU2, 7), ((200,), ("linear",), 1), ((129, 64), ("sigmoid", "relu"), 64), ((64,), ("elu",), 2)),
                   250, 256),
    # hidden width 257 (padded 320) at rows_pad 512: a deeper layer and its input gradient on 32x32 tiles
    "deep32_a": (22, (((257, 257), RELU2, 7), ((64,), ("relu",), 1)), 500, 512),
    "deep32_b": (63, (((100, 257, 257), ("elu", "relu", "sigmoid"), 54),), 481, 512),
    "deep32_c": (130, (((257, 257), ("relu", "relu"), 1), ((257, 257, 31), ("tanh", "elu", "relu"), 65)), 512, 512),
    # (768 / 64)^2 = 144 > 128: the wide weight-gradient tiles although rows_pad % 64 == 0
    "wide_by_size_a": (22, (((720, 720), RELU2, 7), ((17,), ("relu",), 1)), 64, 64),
    "wide_by_size_b": (5, (((720, 720), ("elu", "relu"), 2),), 33, 64),
    "wide_by_size_c": (64, (((720, 720), ("relu", "sigmoid"), 1), ((31, 5), RELU2, 54)), 100, 128),
    # small layers, rows_pad % 64 != 0: the wide weight-gradient tiles
    "wide_by_rows_31": (22, (((17, 31), RELU2, 7), ((5,), ("relu",), 1), ((64, 64, 17), ("elu", "relu", "sigmoid"), 2)), 31, 32),
    "wide_by_rows_32": (63, (((31,), ("relu",), 54), ((17, 5), RELU2, 1)), 32, 32),
    "wide_by_rows_130": (3, (((64, 17), RELU2, 65), ((100,), ("tanh",), 1), ((5, 5, 5, 5), ("relu",) * 4, 7)), 130, 130),
    # every GEMV instantiation on one unequal-depth three-stack set
    "gemv_1": (65, GEMV_SET, 1, 4), "gemv_2": (65, GEMV_SET, 2, 4), "gemv_3": (65, GEMV_SET, 3, 4), "gemv_4": (65, GEMV_SET, 4, 4),
}


@functools.lru_cache(maxsize=None)
def directed_case(name):
    n_in, stacks, rows, max_batch = DIRECTED[name]
    return build_case(name, n_in, stacks, rows, max_batch, 3000 + sorted(DIRECTED).index(name))


def all_stack_cases():
    return [stack_case(i) for i in range(N_RANDOM)] + [directed_case(n) for n in DIRECTED]


STACK_CASE_IDS = ["random%d" % i for i in range(N_RANDOM)] + list(DIRECTED)


def stack_case_by_id(name):
    return directed_case(name) if name in DIRECTED else stack_case(int(name[len("random"):]))


def layer_problems(case):
    """What the host plan (pvae_fc.hip run_forward / run_backward_layers) hands the tile selectors of pvae_gemm_launch.h
    for the full stack set: [("first" | "deep", M, N)] forward, [(M, Kin)] input gradients of the deeper layers and
    [(N, Kin, M)] weight gradients."""
    m = pad32(case.rows)
    fwd, dgrad, wgrad = [("first", m, sum(pad64(w[0] if w else n) for w, _, n in case.stacks))], [], []
    for widths, _, n_out in case.stacks:
        prev = case.n_in
        for i, n in enumerate(tuple(widths) + (n_out,)):
            if i:
                fwd.append(("deep", m, pad64(n)))
                dgrad.append((m, pad64(prev)))
            wgrad.append((pad64(n), pad64(prev), m))
            prev = n
    return fwd, dgrad, wgrad


# ---------------------------------------------------------------------------------------
# PPO step cases
# ---------------------------------------------------------------------------------------
K_VALUES = (1, 2, 7, 63, 64, 65, 130)
PPO_ROWS = (1, 3, 4, 5, 33, 64, 97)
N_PPO = 8                     # per kind
LS_BASE = -1.0                # log_std_base of a state-dependent case; the vector of the other kinds is drawn around it
COVERAGE_KEYS = ("above", "below", "zero_grad_rows", "adv_pos", "adv_neg", "vclip_active")


def logp_of(mean, ls, actions):
    k = mean.shape[1]
    return -0.5 * (((actions - mean) / torch.exp(ls)) ** 2).sum(1) - ls.sum(1) - 0.5 * k * math.log(2 * math.pi)


def step_outputs(case, params, ls_vec, x):
    """(mean, log_std [rows, K], value [rows], ReLU margin) of a PPO step case from `params` / `ls_vec` in their dtype."""
    outs, margin = forward_graph(case.stacks, params, x)
    if case.kind == "state_dependent":
        ls = LS_BASE + outs[2]
    else:
        ls = ls_vec.reshape(1, -1).expand(x.shape[0], -1)
    return outs[0], ls, outs[1].squeeze(1), margin


def row_kinks(cur, batch, cfg):
    """Per row the distance to the nearest kink of the loss: what `ppo_cases.coverage` takes the minimum of."""
    d = {key: t.double() for key, t in batch.items()}
    mean, ls, value = (cur[key].double() for key in ("mean", "log_std", "value"))
    ratio = torch.exp(logp_of(mean, ls, d["actions"]) - d["old_logp"])
    dist = torch.minimum((ratio - (1 - cfg.clip_param)).abs(), (ratio - (1 + cfg.clip_param)).abs())
    dv = value - d["vf_preds"]
    dist = torch.minimum(dist, (dv.abs() - cfg.vf_clip_param).abs())
    e1 = value - d["value_targets"]
    e2 = d["vf_preds"] + torch.clamp(dv, -cfg.vf_clip_param, cfg.vf_clip_param) - d["value_targets"]
    return torch.where(dv.abs() > cfg.vf_clip_param, torch.minimum(dist, (e1 * e1 - e2 * e2).abs()), dist)


@functools.lru_cache(maxsize=None)
def ppo_step_case(seed, kind):
    """A two- or three-stack set [policy K, value 1, (log-std K)] and a train batch built around the twin's float32
    outputs as `sample_batch` of tests/test_gpu_ppo.py builds it.  The output layer of a log-std stack is scaled by 0.2
    (log-stds of LS_BASE +- a few tenths, as a trained policy has them), and the old distribution lies half a standard
    deviation / half a unit of log-std away: a KL of a few tenths per action, so that at one row and K = 1 too the KL stat
    is a sum of terms of its own size and not the rounding residue of terms of order 1.  Odd seeds: the minibatch is rows
    index[first : first + rows] of a larger batch, first > 0; even seeds: the batch's rows in order."""
    g = torch.Generator().manual_seed(5000 + 17 * seed + KINDS.index(kind))
    ri = lambda n: int(torch.randint(n, (1,), generator=g))                          # noqa: E731
    rn = lambda *s: torch.randn(*s, generator=g)                                    # noqa: E731
    k = K_VALUES[(seed + KINDS.index(kind)) % len(K_VALUES)]
    rows = PPO_ROWS[(seed + 2 * KINDS.index(kind)) % len(PPO_ROWS)]
    n_in = N_INS[ri(len(N_INS))]
    stacks = [draw_stack(g, k), draw_stack(g, 1)] + ([draw_stack(g, k)] if kind == "state_dependent" else [])
    if seed < 4 and len({len(w) for w, _, _ in stacks}) == 1:                        # (the train_mask cases: unequal depths)
        stacks[1] = draw_stack(g, 1, depth=len(stacks[0][0]) % 4 + 1)
    stacks = tuple(stacks)
    case = types.SimpleNamespace(name="ppo%d_%s" % (seed, kind), kind=kind, k=k, rows=rows, n_in=n_in, stacks=stacks,
                                 max_batch=rows + (0, 1, 30)[ri(3)], seed=seed, cfg=types.SimpleNamespace(**LOSS))
    case.depths = tuple(len(w) for w, _, _ in stacks)
    case.params = draw_params(g, n_in, stacks)
    if kind == "state_dependent":
        w, b = case.params[2][-1]
        case.params[2][-1] = (0.2 * w, 0.2 * b)
    case.ls_vec = None if kind == "state_dependent" else (LS_BASE + 0.2 * rn(k))
    n = 2 * rows + 8
    obs = rn(n, n_in)
    with torch.no_grad():
        mean, ls, value, margin = step_outputs(case, case.params, case.ls_vec, obs)           # float32, as sample_batch
    actions = mean + torch.exp(ls) * rn(n, k)
    # value targets at least half a unit from the value: the value loss of a ONE-row minibatch is then not the square of a
    # difference that cancels (its relative error is 2 |error of the value| / |value - target|)
    away = lambda t: t + 0.5 * torch.sign(t)                                        # noqa: E731
    cand = {"actions": actions, "old_dist": torch.cat([mean + 0.5 * torch.exp(ls) * rn(n, k), ls + 0.5 * rn(n, k)], 1),
            "old_logp": logp_of(mean, ls, actions) - 0.35 * rn(n), "advantages": rn(n), "value_targets": value + away(rn(n)),
            "vf_preds": value + rn(n)}
    # the filter reads the float64 twin's outputs: those are what the oracle's branches follow
    with torch.no_grad():
        mean64, ls64, value64, margin64 = step_outputs(case, leaves(case.params, torch.float64),
                                                       None if case.ls_vec is None else case.ls_vec.double(), obs.double())
    keep = (row_kinks({"mean": mean64, "log_std": ls64, "value": value64}, cand, case.cfg) > KINK) & (margin64 > RELU_MARGIN)
    case.dropped = 1.0 - float(keep.double().mean())
    sel = torch.nonzero(keep)[:rows, 0]
    assert sel.numel() == rows, (case.name, "too few rows off the kinks")
    case.cur64 = {"mean": mean64[sel], "log_std": ls64[sel], "value": value64[sel]}
    used = dict({key: t[sel] for key, t in cand.items()}, obs=obs[sel])
    case.used = used
    case.coverage = coverage(case.cur64, {key: used[key] for key in cand}, case.cfg)
    if seed % 2:
        # the used rows scattered over a batch of rows + 7 rows; the other seven are never read
        n_batch, case.first = rows + 7, 3
        perm = torch.randperm(n_batch, generator=g)
        case.index = perm.to(torch.int32)
        case.batch = {key: rn(n_batch, *t.shape[1:]) for key, t in used.items()}
        for key, t in used.items():
            case.batch[key][perm[3: 3 + rows]] = t
    else:
        case.first, case.index, case.batch = 0, None, used
    return case


PPO_CASE_IDS = [(seed, kind) for kind in KINDS for seed in range(N_PPO)]


def step_twin(case, dtype=torch.float64, steps=1, lr=1e-4):
    """`steps` PPO steps on the used rows in plain torch (`dtype`) with torch.optim.Adam from zero moments: per step the
    stats, and of the FIRST step every gradient; .params / .ls_vec are the leaves after the last step, .opt their optimizer."""
    params = leaves(case.params, dtype)
    ls_vec = None
    if case.kind != "state_dependent":
        ls_vec = case.ls_vec.to(dtype).clone().requires_grad_(case.kind == "state_independent")
    trained = [t for layers in params for pair in layers for t in pair] + ([ls_vec] if case.kind == "state_independent" else [])
    opt = torch.optim.Adam(trained, lr=lr)
    used = {key: t.to(dtype) for key, t in case.used.items()}
    res = types.SimpleNamespace(stats=[], params=params, ls_vec=ls_vec, opt=opt)
    for step in range(steps):
        opt.zero_grad(set_to_none=True)
        mean, ls, value, _ = step_outputs(case, params, ls_vec, used["obs"])
        total, stats = P.ppo_loss_torch(mean, ls, value, cfg=case.cfg, **{key: used[key] for key in used if key != "obs"})
        total.backward()
        if step == 0:
            res.grads = [[(w.grad.clone(), b.grad.clone()) for w, b in layers] for layers in params]
            res.ls_grad = ls_vec.grad.clone() if case.kind == "state_independent" else None
        opt.step()
        res.stats.append(stats.detach())
    return res


# ---------------------------------------------------------------------------------------
# loss-head cases
# ---------------------------------------------------------------------------------------
HEAD_KS = (1, 2, 63, 64, 65, 128, 130, 200)
HEAD_ROWS = 256
# (K, kind) -> seed of ppo_cases.make_case at 256 rows under which the coverage assertions of
# test_head_matches_the_float64_restatement hold without filtering (constant and state-independent cases are the same
# draws) and the float32 restatement of every run stays within a quarter of the bounds: the smallest such seed, found with
# `search_head_seed`, checked by tests/test_fc_cases_cpu.py
HEAD_SEEDS = {
    (1, "constant"): 16, (1, "state_independent"): 16, (1, "state_dependent"): 23,
    (2, "constant"): 13, (2, "state_independent"): 13, (2, "state_dependent"): 0,
    (63, "constant"): 9, (63, "state_independent"): 9, (63, "state_dependent"): 8,
    (64, "constant"): 0, (64, "state_independent"): 0, (64, "state_dependent"): 10,
    (65, "constant"): 3, (65, "state_independent"): 3, (65, "state_dependent"): 3,
    (128, "constant"): 14, (128, "state_independent"): 14, (128, "state_dependent"): 124,
    (130, "constant"): 4, (130, "state_independent"): 4, (130, "state_dependent"): 103,
    (200, "constant"): 94, (200, "state_independent"): 94, (200, "state_dependent"): 2,
    (3, "state_dependent"): 4,                                     # WAVE_CAP_K: the case that crosses the head's wave cap
}


def head_inputs(k, kind, seed, rows=HEAD_ROWS):
    """(cur, batch, cfg) in float32 -- what the kernel reads -- from ppo_cases.make_case."""
    cur64, batch64, cfg = make_case(rows, k, seed, kind=kind, **{key: v for key, v in LOSS.items() if key != "clip_param"})
    return {key: v.float() for key, v in cur64.items()}, {key: v.float() for key, v in batch64.items()}, cfg


def head_covered(cov):
    return (cov["above"] >= 0.10 and cov["below"] >= 0.10 and cov["zero_grad_rows"] >= 0.10 and cov["vclip_active"] >= 0.10
            and cov["kink"] > KINK)


def head_restatement_errors(k, kind, inputs=None):
    """Per run of a head case the float32 restatement against the float64 one: [(rows, with_index, stats error per component
    by the measure of test_gpu_ppo.check_stats, largest scaled gradient error)]."""
    floors = torch.tensor([1.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    out = []
    for rows, with_index, idx in head_runs(k, kind):
        a, b = head_twin(k, kind, idx, torch.float32, inputs), head_twin(k, kind, idx, torch.float64, inputs)
        e_stats = (a[0].double() - b[0]).abs() / torch.maximum(b[0].abs(), floors)
        e_grad = max(float((x.double() - y).abs().max() / (y.abs().max() + 1e-30)) for x, y in zip(a[1:], b[1:]))
        out.append((rows, with_index, e_stats, e_grad))
    return out


def search_head_seed(k, kind, limit=2000, stats_room=0.25e-5, grad_room=0.25e-4):
    for seed in range(limit):
        inputs = head_inputs(k, kind, seed)
        if head_covered(coverage(*inputs)) and all(float(e.max()) < stats_room and g < grad_room
                                                   for _, _, e, g in head_restatement_errors(k, kind, inputs)):
            return seed
    raise AssertionError("no seed under %d for K = %d, %s" % (limit, k, kind))


@functools.lru_cache(maxsize=None)
def head_case(k, kind):
    return head_inputs(k, kind, HEAD_SEEDS[(k, kind)])


HEAD_RUN_ROWS = (1, 2, 33, 256)
# more rows than the head's 4096 waves take in one pass of two rows each: gathered, with repeats, from the 256 kink-free rows
# of one more head case (a fresh batch of 20 000 rows would not be kink-free)
WAVE_CAP_K, WAVE_CAP_KIND, WAVE_CAP_ROWS = 3, "state_dependent", (8200, 20000)


def wave_cap_index(rows):
    return torch.randint(HEAD_ROWS, (rows,), generator=torch.Generator().manual_seed(rows))


def head_runs(k, kind):
    """[(rows, with_index, idx)]: the rows of the 256-row batch that each run of a head case reads, in order."""
    g = torch.Generator().manual_seed(5 + k)
    return [(rows, with_index, torch.randperm(HEAD_ROWS, generator=g)[:rows] if with_index else torch.arange(rows))
            for rows in HEAD_RUN_ROWS for with_index in (False, True)]


def head_twin(k, kind, idx, dtype=torch.float64, inputs=None):
    """The loss of rows `idx` of a head case in plain torch (`dtype`) on the float32 inputs: (stats, d_mean, d_value, d_log_std
    -- per row for a state-dependent log-std, of the vector otherwise)."""
    cur, batch, cfg = inputs or head_case(k, kind)
    rows = idx.numel()
    mean = cur["mean"][idx].to(dtype).requires_grad_(True)
    value = cur["value"][idx].to(dtype).requires_grad_(True)
    if kind == "state_dependent":
        leaf = cur["log_std"][idx].to(dtype).requires_grad_(True)
        ls = leaf
    else:
        leaf = cur["log_std"][0].to(dtype).requires_grad_(True)
        ls = leaf.reshape(1, k).expand(rows, k)
    total, stats = P.ppo_loss_torch(mean, ls, value, cfg=cfg, **{key: v[idx].to(dtype) for key, v in batch.items()})
    total.backward()
    return stats.detach(), mean.grad, value.grad, leaf.grad


# ---------------------------------------------------------------------------------------
# segment tables of the GAE tests (the columns come from test_gpu_gae.dense_case)
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_segments():
    """4200 segments of 1..3 rows and two long ones (200 rows at index 1000, 131 rows at index 4150: below and above the
    4096 segments one pass of `gae_kernel`'s grid takes), 8736 rows in all; seg_done mixed: (lengths, done) as tuples."""
    g = torch.Generator().manual_seed(77)
    lengths = torch.randint(1, 4, (4200,), generator=g)
    lengths[1000], lengths[4150] = 200, 131
    short = [i for i in range(4200) if i not in (1000, 4150)]
    i = 0
    while int(lengths.sum()) != 8736:                       # nudge short segments, in order, to the row count wanted
        s = short[i % len(short)]
        step = 1 if int(lengths.sum()) < 8736 else -1
        if 1 <= int(lengths[s]) + step <= 3:
            lengths[s] += step
        i += 1
    done = torch.rand(4200, generator=g) < 0.4
    return tuple(int(v) for v in lengths), tuple(bool(v) for v in done)


@functools.lru_cache(maxsize=None)
def many_rows():
    """2100 segments of 1..300 rows: more rows than one pass of the standardisation's (1024 x 256) and the copy's grids."""
    g = torch.Generator().manual_seed(78)
    lengths = torch.randint(1, 301, (2100,), generator=g)
    done = torch.rand(2100, generator=g) < 0.4
    return tuple(int(v) for v in lengths), tuple(bool(v) for v in done)


def seg_start_of(lengths):
    return torch.tensor([0] + list(itertools.accumulate(lengths)), dtype=torch.int32)
