"""The PPO learner's host driver (physicsvae_amd/csrc/pvae_ppo_learner.h) and the model-level mixin
(`engine_ppo.PpoPolicy`), the parts that need no GPU.

1. ONE TABLE of malformed calls walked through every learner entry point of both models -- step, sgd, grad, apply, diag,
   peer_export, peer_open, evaluate, prepare, act -- on a null handle, an unbound one and one bound to fake pointers that
   the argument checks never dereference.  Every row pins the return code and a distinctive part of `pvae_last_error`,
   and that nothing was launched: the counters read 0.  The table records what the library did BEFORE the driver was
   written once: it passes unchanged against the parent commit's library (PVAE_LIB_PATH).  The one deliberate change --
   the stack set's evaluate, prepare and act now zero their counters on entry -- has no row that tells the two libraries
   apart here: the counters only ever leave 0 by launching, which takes a GPU (tests/test_gpu_gae.py reads them there).
2. The mixin on a stub engine that records its calls: the call sequence of `ppo_learn`, `ppo_prepare` and
   `compute_actions`, and the diagnostics binding restored when `ppo_sgd` raises."""
import ctypes as C
import types

import pytest
import torch

from physicsvae_amd import _lib
from physicsvae_amd import ppo as P
from physicsvae_amd.engine_ppo import PpoPolicy
from test_ppo_dp_cpu import fake, fc_config
from test_ppo_vae_cpu import DA, model, value_set

MODELS = ("fc", "vae")
K = {"fc": 54, "vae": DA}
NULL = {"fc": b"null stack set", "vae": b"null ctx"}
STEP = ("step", "sgd", "grad", "apply")
PEER = ("peer_export", "peer_open")
EVAL = ("evaluate", "prepare", "act")

# (entry points, handle state, what is wrong with the otherwise well-formed call, return code, part of the message --
#  one for both models, or one per model)
TABLE = [
    # -- the handle states
    (STEP + ("diag",) + EVAL, "null", {}, -1, NULL),
    (PEER, "null", {}, -1, {"fc": b"null argument", "vae": b"null ctx"}),
    (STEP + EVAL, "unbound", {}, -2, {"fc": b"pvae_fc_bind has not been called", "vae": b"workspace not bound"}),
    (PEER, "unbound", {}, -2, {"fc": b"pvae_fc_ppo_bind has not been called", "vae": b"pvae_ppo_bind has not been called"}),
    (("diag",), "unbound", {"capacity": 0}, -1, b"capacity_steps must be >= 1, got 0"),
    # -- what is refused before the handle is looked at, in each model's own order
    (("sgd",), "null", {"minibatch": 0}, -1, b"minibatch and num_sgd_iter must be positive"),
    (("prepare",), "null", {"gamma": 1.5}, -1, b"gamma and lambda must lie in [0, 1]"),
    (("act",), "null", {"act_in": None}, -1, {"fc": b"null stack set", "vae": b"null in, params or out"}),
    # -- the shared bad arguments, on a bound handle
    (("sgd",), "bound", {"minibatch": 0}, -1, b"minibatch and num_sgd_iter must be positive"),
    (("sgd",), "bound", {"num_sgd_iter": 0}, -1, b"minibatch and num_sgd_iter must be positive"),
    (("sgd",), "bound", {"minibatch": 9}, -1, b"minibatch 9 > max_batch 8"),
    (STEP, "bound", {"adam_t": 0}, -1, b"adam_t must be >= 1"),
    (STEP, "bound", {"train_mask": 8}, -1, {"fc": b"train_mask names a stack that does not exist",
                                            "vae": b"train_mask names a net that does not exist (bits: 1 TE, 2 MD, 4 value)"}),
    (STEP, "bound", {"train_mask": -1}, -1, b"train_mask names a"),
    (("grad", "apply"), "bound", {"kind": 1, "ls_grad": None}, -1, b"ls_grad is null (log_std_kind 1)"),
    (("step", "grad"), "bound", {"first": 6}, -1, b"rows [6, +4) outside the batch of 8"),
    (("step", "grad"), "bound", {"first": -1}, -1, b"rows [-1, +4) outside the batch of 8"),
    (("step", "grad"), "bound", {"rows": 9}, -1, b"rows 9 outside [1, 8]"),
    (("step", "grad"), "bound", {"rows": 0}, -1, b"rows must be positive"),
    (("step", "sgd", "grad"), "bound", {"stats": None}, -1, b"stats_out is null"),
    (("step", "sgd", "grad"), "bound", {"batch_k": 1}, -1, {"fc": b"batch k 55 != policy outputs 54", "vae": b"batch k 6 != dim_action 5"}),
    (STEP, "bound", {"kind": 3}, -1, b"log_std_kind 3"),
    (("apply",), "bound", {"params": None}, -1, b"null params"),
    (("sgd",), "bound", {"diag_capacity": 1}, -1, b"2 steps, the bound diagnostics buffer holds 1 rows"),
    # -- diag and the exchange set-up
    (("diag",), "bound", {"capacity": 0}, -1, b"capacity_steps must be >= 1, got 0"),
    (("diag",), "bound", {"diag_scratch": None}, -1, b"diagnostics scratch is null"),
    (("diag",), "bound", {"diag_scratch": 0x10008}, -1, b"diagnostics scratch must be 16-byte aligned"),
    (("diag",), "bound", {"diag_bytes": 8}, -1, b"diagnostics scratch too small: 8 <"),
    (("peer_export",), "bound", {"blob": None}, -1, {"fc": b"null argument", "vae": b"null blob"}),
    (("peer_open",), "bound", {"blob": None}, -1, {"fc": b"null argument", "vae": b"null blobs"}),
    (("peer_open",), "bound", {"world": 0}, -1, b"rank 0 / world 0 outside [0, "),
    (("peer_open",), "bound", {"rank": 2}, -1, b"rank 2 / world 2 outside [0, "),
    (("peer_open",), "bound", {}, -2, b"export first"),
    # -- evaluate, prepare, act
    (EVAL, "bound", {"n_rows": 0}, -1, b"n_rows 0 out of range"),
    (EVAL, "bound", {"rollout_k": 1}, -1, {"fc": b"k 55 != policy outputs 54", "vae": b"k 6 != dim_action 5"}),
    (EVAL, "bound", {"kind": 3}, -1, b"log_std_kind 3"),
    (EVAL, "bound", {"obs": None}, -1, b"rollout obs or actions is null"),
    (("evaluate", "prepare"), "bound", {"n_segs": 0}, -1, b"n_segs must be >= 1, got 0"),
    (("evaluate", "prepare"), "bound", {"boot_obs": None}, -1, b"rollout boot_obs or seg_done is null"),
    (("evaluate",), "bound", {"out_vf_preds": None, "last_value": None}, -1, b"neither vf_preds nor last_value: nothing to compute"),
    (("evaluate",), "bound", {"out_old_logp": None}, -1, b"an evaluate output (vf_preds, old_dist, old_logp) is null"),
    (("prepare",), "bound", {"gamma": 1.5}, -1, b"gamma and lambda must lie in [0, 1]"),
    (("prepare",), "bound", {"given_vf_preds": 0x700000}, -1, b"go together: all three or none"),
    (("prepare",), "bound", {"advantages": None}, -1, b"advantages or value_targets is null"),
    (("prepare",), "bound", {"seg_last": 7}, -1, b"seg_start must run from 0 to n_rows 8, got 0 .. 7"),
    (("prepare",), "bound", {"gae_scratch": None}, -1, b"scratch is null"),
    (("act",), "bound", {"act_in": None}, -1, b"null in, params or out"),
    (("act",), "bound", {"explore": 2}, -1, b"explore must be 0 or 1, got 2"),
    (("act",), "bound", {"n_dst_rows": 4}, -1, b"n_dst_rows 4 < n_rows 8 without out_row"),
]


@pytest.fixture(scope="module")
def handles():
    """{(model, state): handle} -- created once, bound to addresses that are never dereferenced."""
    lib = _lib.load()
    h, sets = {("fc", "null"): None, ("vae", "null"): None}, []
    for state in ("unbound", "bound"):
        ctx = C.c_void_p()
        assert lib.pvae_fc_create(C.byref(fc_config()), C.byref(ctx)) == 0
        if state == "bound":
            assert lib.pvae_fc_bind(ctx, fake(5), fake(6), 1 << 30) == 0
            assert lib.pvae_fc_ppo_bind(ctx, fake(1), fake(2), fake(3), fake(4), 1 << 20, fake(7), fake(8), fake(9)) == 0
        h["fc", state] = ctx
        ctx = C.c_void_p()
        assert lib.pvae_create(C.byref(model(8).engine.cfg), C.byref(ctx)) == 0
        if state == "bound":
            assert lib.pvae_bind_workspace(ctx, fake(5), 1 << 30) == 0
            assert lib.pvae_bind_arenas(ctx, fake(6), fake(17), fake(18), fake(19)) == 0
            sets.append(value_set(lib))
            assert lib.pvae_ppo_bind(ctx, fake(1), fake(2), fake(3), fake(4), 1 << 20, fake(7), fake(8), fake(9), sets[-1]) == 0
        h["vae", state] = ctx
    yield h
    for state in ("unbound", "bound"):
        lib.pvae_fc_destroy(h["fc", state])
        lib.pvae_destroy(h["vae", state])
    for s in sets:
        lib.pvae_fc_destroy(s)


def call(lib, m, entry, ctx, bad):
    """The entry point of model `m` on a call that is well formed but for what `bad` names."""
    k, pre = K[m], "pvae_fc_ppo_" if m == "fc" else "pvae_ppo_"
    fn = getattr(lib, pre + entry)
    draws = () if m == "fc" else (None, 1, 0, 0)                   # eps, noise, rng_seed, rng_offset
    kind = bad.get("kind", 0)
    if entry in STEP:
        b = _lib.FcPpoBatch()
        for i, (name, _) in enumerate(_lib.FcPpoBatch._fields_[:7]):
            setattr(b, name, 0x100000 * (i + 1))
        b.n_rows, b.k = 8, k + bad.get("batch_k", 0)
        p = P.PPOConfig().params(kind, adam_t=bad.get("adam_t", 1), train_mask=bad.get("train_mask", 0))
        first, rows, stats = bad.get("first", 0), bad.get("rows", 4), bad.get("stats", fake(20))
        ls_grad = bad.get("ls_grad", fake(21))
        if entry == "step":
            return fn(ctx, C.byref(b), None, first, rows, C.byref(p), *draws, stats, None)
        if entry == "grad":
            return fn(ctx, C.byref(b), None, first, rows, C.byref(p), *draws, stats, ls_grad, None)
        if entry == "sgd":
            return fn(ctx, C.byref(b), None, bad.get("minibatch", 4), bad.get("num_sgd_iter", 1), C.byref(p), *draws, stats, None)
        return fn(ctx, C.byref(p) if bad.get("params", p) is not None else None, 1.0, ls_grad, None)
    if entry == "diag":
        return fn(ctx, fake(22), bad.get("capacity", 4), bad.get("diag_scratch", fake(23)), bad.get("diag_bytes", 1 << 30))
    if entry == "peer_export":
        return fn(ctx, bad.get("blob", C.create_string_buffer(_lib.P2P_BLOB_BYTES)))
    if entry == "peer_open":
        return fn(ctx, bad.get("rank", 0), bad.get("world", 2), bad.get("blob", C.create_string_buffer(2 * _lib.P2P_BLOB_BYTES)))
    gp = P.make_gae_params(bad.get("gamma", 0.99), 0.95, True, kind)
    d = _lib.PpoDraws()
    d.noise, d.eps_out = 1, 0x900000
    dr = () if m == "fc" else (C.byref(d),)
    n_rows = bad.get("n_rows", 8)
    if entry == "act":
        i, o = _lib.PpoActIn(), _lib.PpoActOut()
        i.obs, i.n_rows, i.n_dst_rows, i.k = bad.get("obs", 0x100000), n_rows, bad.get("n_dst_rows", 8), k + bad.get("rollout_k", 0)
        i.explore = bad.get("explore", 1)
        o.actions, o.old_dist, o.old_logp, o.vf_preds, o.noise_out = 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
        return fn(ctx, C.byref(i) if bad.get("act_in", i) is not None else None, C.byref(gp), *dr, C.byref(o), None)
    ro, out = _lib.FcRollout(), _lib.FcPrepared()
    for i, name in enumerate(("obs", "actions", "rewards", "seg_start", "seg_done", "boot_obs")):
        setattr(ro, name, bad.get(name, 0x100000 * (i + 1)))
    ro.vf_preds = bad.get("given_vf_preds")
    ro.n_rows, ro.n_segs, ro.k, ro.seg_first, ro.seg_last = n_rows, bad.get("n_segs", 2), k + bad.get("rollout_k", 0), 0, bad.get("seg_last", n_rows)
    for i, name in enumerate(("vf_preds", "old_dist", "old_logp", "last_value", "advantages", "value_targets")):
        setattr(out, name, bad.get("out_" + name, bad.get(name, 0x1000000 * (i + 1))))
    if entry == "evaluate":
        return fn(ctx, C.byref(ro), C.byref(gp), *dr, C.byref(out), None)
    return fn(ctx, C.byref(ro), C.byref(gp), *dr, C.byref(out), bad.get("gae_scratch", fake(24)), 1 << 30, None)


def launched(lib, m, ctx):
    """(launches of the last step, of the last rows pass, of what followed it) as the library reports them."""
    s, e, r = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    pre = "pvae_fc_" if m == "fc" else "pvae_ppo_"
    assert getattr(lib, ("pvae_fc_ppo_" if m == "fc" else "pvae_ppo_") + "launches")(ctx, C.byref(s)) == 0
    assert getattr(lib, pre + "gae_launches")(ctx, C.byref(e), C.byref(r)) == 0
    return s.value, e.value, r.value


@pytest.mark.parametrize("m", MODELS)
@pytest.mark.parametrize("row", range(len(TABLE)), ids=lambda i: "%s-%s-%s" % (TABLE[i][0][0], TABLE[i][1], "-".join(TABLE[i][2]) or "ok"))
def test_malformed_call_is_refused_with_its_code_and_message_and_launches_nothing(handles, m, row):
    lib = _lib.load()
    entries, state, bad, code, msg = TABLE[row]
    ctx = handles[m, state]
    want = msg[m] if isinstance(msg, dict) else msg
    diag = getattr(lib, "pvae_fc_ppo_diag" if m == "fc" else "pvae_ppo_diag")
    if "diag_capacity" in bad:
        assert diag(ctx, fake(22), bad["diag_capacity"], fake(23), 1 << 30) == 0
    try:
        for entry in entries:
            rc = call(lib, m, entry, ctx, bad)
            assert rc == code and want in lib.pvae_last_error(), (entry, rc, lib.pvae_last_error())
            if ctx is not None:
                assert launched(lib, m, ctx) == (0, 0, 0), entry
    finally:
        if ctx is not None:
            assert diag(ctx, None, 0, None, 0) == 0                    # whatever a row bound is unbound again


def test_the_table_walks_every_entry_point_in_every_handle_state():
    seen = {(e, state) for entries, state, _, _, _ in TABLE for e in entries}
    assert seen == {(e, s) for e in STEP + ("diag",) + PEER + EVAL for s in ("null", "unbound", "bound")}


# 2. the mixin on a stub engine
class StubEngine:
    device, max_batch = torch.device("cpu"), 32

    def __init__(self, fail_sgd=False):
        self.calls, self.bound, self.fail_sgd = [], None, fail_sgd

    def _need_gpu(self):
        self.calls.append("_need_gpu")

    def ppo_bind(self, *a):
        self.calls.append("ppo_bind")

    def ppo_batch(self, columns):
        self.calls.append("ppo_batch")
        return (types.SimpleNamespace(n_rows=70), None)

    def ppo_diag_bound(self):
        self.calls.append("ppo_diag_bound")
        return self.bound

    def ppo_diag(self, buffer=None, row=0):
        self.calls.append(("ppo_diag", buffer, row))
        self.bound = None if buffer is None else (buffer, row)

    def ppo_sgd(self, cols, params, minibatch, num_sgd_iter, perm, **draws):
        self.calls.append(("ppo_sgd", params.adam_t, params.train_mask, params.log_std_kind, minibatch, num_sgd_iter, draws))
        if self.fail_sgd:
            raise RuntimeError("pvae_fc_ppo_sgd: refused")
        return torch.zeros(P.dp_steps(70, minibatch, num_sgd_iter), 5)

    def ppo_prepare(self, ro, params, **draws):
        self.calls.append(("ppo_prepare", sorted(ro), params.log_std_kind, draws))
        return {k: k for k in ("old_dist", "old_logp", "vf_preds", "advantages", "value_targets", "last_value")}

    def ppo_act(self, obs, params, **kw):
        self.calls.append(("ppo_act", params.log_std_kind, sorted(kw)))
        return {"actions": "a", "old_dist": "d", "old_logp": "l", "vf_preds": "v", "action_noise": "n"}


class Dummy(PpoPolicy):
    """A model with one frozen state_independent log-std vector and a latent: every hook records itself."""

    def __init__(self, engine):
        self.engine, self.after = engine, []

    def _ppo_learn_mask(self, config):
        self.engine.calls.append("learn_mask")
        return 3

    def _ppo_bind_engine(self):
        self.engine.ppo_bind()
        return "state_independent", 0.0, False

    def _ppo_draws(self, call, eps, dp_shape=None):
        return {"eps": eps, "offset": 11}

    def _ppo_after(self, call, n):
        self.after.append((call, n))


def test_mixin_call_sequences_and_the_diagnostics_binding_restored_when_sgd_raises():
    cfg = P.PPOConfig(sgd_minibatch_size=33, num_sgd_iter=2)
    batch = {k: None for k in P.SAMPLE_BATCH_KEYS}
    steps = P.dp_steps(70, 33, 2)
    diag_out = torch.zeros(steps, _lib.PPO_DIAG)
    # learn, without and with a diagnostics buffer; the caller's own binding comes back
    eng = StubEngine()
    d = Dummy(eng)
    stats = d._policy_learn(batch, cfg, None, "eps", None, None)
    sgd = ("ppo_sgd", 1, 3, 0, 33, 2, {"eps": "eps", "offset": 11})          # (a frozen vector is a constant one: kind 0)
    assert eng.calls == ["learn_mask", "ppo_bind", "ppo_batch", sgd] and tuple(stats.shape) == (steps, 5)
    assert d.after == [("learn", steps)] and d.__dict__["_ppo_t"] == steps
    eng.calls.clear()
    eng.bound = ("theirs", 2)
    d._policy_learn(batch, cfg, None, None, None, diag_out)
    assert eng.calls == ["learn_mask", "ppo_bind", "ppo_batch", "ppo_diag_bound", ("ppo_diag", diag_out, 0),
                         ("ppo_sgd", steps + 1, 3, 0, 33, 2, {"eps": None, "offset": 11}), ("ppo_diag", "theirs", 2)]
    assert eng.bound == ("theirs", 2) and d.__dict__["_ppo_t"] == 2 * steps
    with pytest.raises(ValueError, match="diag_out must be"):
        d._policy_learn(batch, cfg, None, None, None, torch.zeros(steps - 1, _lib.PPO_DIAG))
    # sgd raises: the binding is restored all the same, and nothing is counted
    eng = StubEngine(fail_sgd=True)
    d = Dummy(eng)
    with pytest.raises(RuntimeError, match="refused"):
        d._policy_learn(batch, cfg, None, None, None, diag_out)
    assert eng.calls[-2][0] == "ppo_sgd" and eng.calls[-1] == ("ppo_diag", None, 0) and eng.bound is None
    assert d.after == [] and "_ppo_t" not in d.__dict__
    # prepare: the sampler's columns go along only when all three are there
    eng = StubEngine()
    d = Dummy(eng)
    ro = {k: torch.zeros(70, 1) for k in P.ROLLOUT_KEYS}
    out = d._policy_prepare(dict(ro, vf_preds=1), cfg, "eps")
    keys = ["actions", "boot_obs", "obs", "rewards", "seg_done", "seg_start"]
    assert eng.calls == ["_need_gpu", "ppo_bind", ("ppo_prepare", keys, 1, {"eps": "eps", "offset": 11})]
    assert d.after == [("prepare", 3)] and "latent_eps" not in out and out["action_logp"] == "old_logp"
    with pytest.raises(KeyError, match="rollout lacks rewards"):
        d._policy_prepare({k: v for k, v in ro.items() if k != "rewards"}, cfg, None)
    eng.calls.clear()
    d._policy_prepare(dict(ro, vf_preds=1, action_dist_inputs=2, action_logp=3), cfg, None)
    assert eng.calls[-1][1] == sorted(keys + ["vf_preds", "old_dist", "old_logp"]) and d.after[-1] == ("prepare", 0)
    # act
    eng.calls.clear()
    res = d._policy_act(torch.zeros(40, 3), False, None, None, None, None, None)
    assert eng.calls == ["_need_gpu", "ppo_bind", ("ppo_act", 1, ["clip", "eps", "explore", "noise", "offset", "out", "out_row"])]
    assert d.after[-1] == ("act", 2) and "action_noise" not in res and res["action_dist_inputs"] == "d"
