"""FullyConnectedPolicy ("fcnn", rmt:323-457) and the stack set behind it (include/pvae.h pvae_fc_*), the parts that need
no GPU: the header and the binding name the same symbols, the layout queries are self-consistent, the module's state dict
has the keys and shapes of the reference's capture (tests/golden/fcnn_tiny.npz, tools/gen_golden_fcnn.py), and what the
HIP path does not offer is refused by name."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from physicsvae_amd import _lib
from physicsvae_amd.engine import Stack, StackSetEngine
from physicsvae_amd.spaces import Box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC_NAMES = {"pvae_fc_num_layers", "pvae_fc_layer", "pvae_fc_arena_floats", "pvae_fc_workspace_bytes", "pvae_fc_create",
            "pvae_fc_destroy", "pvae_fc_bind", "pvae_fc_forward", "pvae_fc_backward", "pvae_fc_launches"}
VARIANTS = ("constant", "state_independent", "state_dependent")


def policy(cmc, obs=22, num_outputs=10):
    from physicsvae_amd import FullyConnectedPolicy
    cmc = dict(cmc, device="cpu")
    return FullyConnectedPolicy(Box(np.zeros(obs), np.zeros(obs)), Box(np.zeros(num_outputs // 2), np.zeros(num_outputs // 2)),
                                num_outputs, {"custom_model_config": cmc}, "fcnn")


def spec_of(g, name):
    cmc = json.loads(str(g[name + "/spec"]))
    return cmc


def captured_state_dict(g, name):
    flat, sd, o = torch.from_numpy(g[name + "/sd"]), {}, 0
    for k, shape in json.loads(str(g[name + "/keys"])):
        n = int(np.prod(shape))
        sd[k] = flat[o: o + n].reshape(shape).clone()
        o += n
    assert o == flat.numel()
    return sd


def test_header_binding_and_library_name_the_same_symbols():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "pvae.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pvae_[a-z0-9_]+)\s*\(", header))
    assert FC_NAMES <= declared
    assert declared == set(_lib.EXPORTS)
    for name in FC_NAMES:
        assert hasattr(lib, name), name
    assert lib.pvae_abi_version() == _lib.ABI_VERSION == 12
    assert "#define PVAE_ABI_VERSION 12" in header and "#define PVAE_FC_MAX_STACKS 4" in header
    assert _lib.FC_MAX_STACKS == 4 and _lib.NUM_NETS == 5
    assert lib.pvae_set_option(None, b"fc_per_stack", 0) == 0


@pytest.mark.parametrize("stacks", [
    [((256, 256), 54), ((256, 256), 1)],
    [((256, 256), 54), ((256, 256), 1), ((64, 64), 54)],
    [((48, 40), 5), ((24,), 1), ((24, 16, 8), 5), ((7,), 3)],
])
def test_layout_queries_are_self_consistent(stacks):
    eng = StackSetEngine(722, [(Stack(w, "relu"), n) for w, n in stacks], 500, device="cpu")
    assert len(eng.layers) == sum(len(w) + 1 for w, _ in stacks)
    spans = []
    for s, (widths, n_out) in enumerate(stacks):
        prev = 722
        lays = eng.stack_layers(s)
        assert [l["index"] for l in lays] == list(range(len(widths) + 1))
        for l, want in zip(lays, list(widths) + [n_out]):
            assert (l["n_in"], l["n_out"]) == (prev, want)
            assert l["ld"] == (prev + 63) // 64 * 64 and l["n_out_pad"] == (want + 63) // 64 * 64       # the five-net arena's rules
            assert l["w_offset"] % 64 == 0 and l["b_offset"] % 64 == 0 and l["col0"] == 0
            spans.append((l["w_offset"], l["w_offset"] + l["n_out_pad"] * l["ld"]))
            spans.append((l["b_offset"], l["b_offset"] + l["n_out_pad"]))
            prev = want
        assert lays[-1]["act"] == _lib.ACT_LINEAR
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] == eng.arena_floats
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))          # disjoint, dense, inside the arena
    # the first layers of all stacks are ONE weight block with one bias vector, in stack order
    firsts = [eng.stack_layers(s)[0] for s in range(len(stacks))]
    for a, b in zip(firsts, firsts[1:]):
        assert b["w_offset"] == a["w_offset"] + a["n_out_pad"] * a["ld"] and b["b_offset"] == a["b_offset"] + a["n_out_pad"]
    assert firsts[0]["b_offset"] == firsts[-1]["w_offset"] + firsts[-1]["n_out_pad"] * firsts[-1]["ld"]
    assert eng.lib.pvae_fc_workspace_bytes(C.byref(eng.cfg)) > 0
    # views have the checkpoint shapes and alias the arena
    for s in range(len(stacks)):
        for (w, b), l in zip(eng.views(s), eng.stack_layers(s)):
            assert tuple(w.shape) == (l["n_out"], l["n_in"]) and tuple(b.shape) == (l["n_out"],)
            assert w.data_ptr() == eng.params.data_ptr() + 4 * l["w_offset"]


def test_bad_stack_sets_are_errors_not_crashes():
    lib = _lib.load()
    cfg = _lib.FcConfig()
    cfg.n_in, cfg.n_stacks, cfg.max_batch = 22, 5, 8
    assert lib.pvae_fc_arena_floats(C.byref(cfg)) < 0 and b"n_stacks" in lib.pvae_last_error()
    cfg.n_stacks = 1
    cfg.depth[0], cfg.n_out[0] = 1, 3
    assert lib.pvae_fc_num_layers(C.byref(cfg)) < 0 and b"width" in lib.pvae_last_error()
    cfg.width[0][0], cfg.act[0][0] = 8, 9
    assert lib.pvae_fc_num_layers(C.byref(cfg)) < 0 and b"activation" in lib.pvae_last_error()
    cfg.act[0][0] = _lib.LAYER_ACTS["tanh"]
    assert lib.pvae_fc_num_layers(C.byref(cfg)) == 2
    with pytest.raises(NotImplementedError, match="1..4 stacks"):
        StackSetEngine(22, [(Stack((8,)), 1)] * 5, 8, device="cpu")
    eng = StackSetEngine(22, [(Stack((8,)), 1)], 8, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.forward(torch.zeros(2, 22))


@pytest.mark.parametrize("name", VARIANTS)
def test_state_dict_has_the_captured_keys_and_shapes_and_loads_strictly(golden, name):
    g = golden("fcnn_tiny")
    m = policy(spec_of(g, name))
    want = json.loads(str(g[name + "/keys"]))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want
    assert len(want) == {"constant": 12, "state_independent": 13, "state_dependent": 18}[name]
    sd = captured_state_dict(g, name)
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # parameters are views into the one arena; pads stay zero
    eng = m.engine
    for k, p in m.named_parameters():
        if not k.endswith("log_std"):
            lo, hi = eng.params.data_ptr(), eng.params.data_ptr() + 4 * eng.arena_floats
            assert lo <= p.data_ptr() < hi, k
    live = torch.zeros_like(eng.params, dtype=torch.bool)
    for s in range(len(eng.stacks)):
        for w, b in eng.views(s, live):
            w.fill_(True)
            b.fill_(True)
    assert float(eng.params[~live].abs().max()) == 0.0
    # log_std as the reference builds it (rmt:266-270: log of sample_std, a scalar or one value per action)
    if name != "state_dependent":
        ls = m._policy_fn._model[-1].log_std.detach()
        assert torch.allclose(ls, torch.as_tensor(np.log(g[name + "/sample_std"]) * np.ones(5), dtype=torch.float32))
        assert isinstance(m._policy_fn._model[-1].log_std, torch.nn.Parameter) == (name == "state_independent")
    else:
        assert m._log_std_fn is not None and float(m._log_std_base) == pytest.approx(np.log(0.5))


def test_default_config_and_normc_initialisation():
    from physicsvae_amd import FullyConnectedPolicy
    d = FullyConnectedPolicy.DEFAULT_CONFIG
    assert d["log_std_type"] == "constant" and d["sample_std"] == 1.0 and d["policy_fn_type"] == "mlp"
    assert [l["hidden_size"] for l in d["policy_fn_layers"]] == [256, 256, "output"]
    assert [l["hidden_size"] for l in d["value_fn_layers"]] == [256, 256, "output"]
    assert [l["hidden_size"] for l in d["log_std_fn_layers"]] == [64, 64, "output"]
    torch.manual_seed(0)
    m = policy({"log_std_type": "state_dependent"}, obs=722, num_outputs=108)
    sd = m.state_dict()
    assert len(sd) == 18 and tuple(sd["_log_std_fn._model.2._model.0.weight"].shape) == (54, 64)
    for k, v in sd.items():
        if k.endswith("weight"):
            std = 0.01 if "._model.2." in k else 1.0
            assert torch.allclose(v.pow(2).sum(1).sqrt(), torch.full((v.shape[0],), std), rtol=1e-4), k     # normc rows
        elif k.endswith("bias"):
            assert float(v.abs().max()) == 0.0
    assert m.to("cpu") is m
    with pytest.raises(RuntimeError, match="chosen at construction"):
        m.double()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward({"obs_flat": torch.zeros(2, 722)}, [], None)
    with pytest.raises(AssertionError, match="forward"):
        m.value_function()


def test_refusals_raise_by_name():
    fc = lambda w, a="relu": {"type": "fc", "hidden_size": w, "activation": a, "init_weight": {"name": "normc", "std": 1.0}}   # noqa: E731
    out = {"type": "fc", "hidden_size": "output", "activation": "linear", "init_weight": {"name": "normc", "std": 0.01}}
    with pytest.raises(AssertionError, match="divisible by two"):
        policy({}, num_outputs=9)
    with pytest.raises(NotImplementedError, match="lstm"):
        policy({"policy_fn_type": "lstm"})
    with pytest.raises(AssertionError):
        policy({"log_std_type": "learned"})
    with pytest.raises(AssertionError, match="positive"):
        policy({"sample_std": 0.0})
    for bad in ("bn", "softmax", "hardmax"):
        with pytest.raises(NotImplementedError, match="policy_fn_layers: only 'fc' layers"):
            policy({"policy_fn_layers": [fc(16), {"type": bad}, out]})
    with pytest.raises(NotImplementedError, match="value_fn_layers: hidden activations"):
        policy({"value_fn_layers": [fc(16, "swish"), out]})
    with pytest.raises(NotImplementedError, match="log_std_fn_layers: hidden activations"):
        policy({"log_std_type": "state_dependent", "log_std_fn_layers": [fc(16), dict(out, activation="tanh")]})
    with pytest.raises(NotImplementedError, match="policy_fn_layers: last layer must have hidden_size 'output'"):
        policy({"policy_fn_layers": [fc(16), fc(8, "linear")]})
    m = policy({"log_std_type": "state_independent"})
    with pytest.raises(AssertionError, match="constant logstd"):
        m.set_exploration_std(0.5)
    m = policy({})
    m.set_exploration_std(0.5)
    assert torch.allclose(m._policy_fn._model[-1].log_std, torch.full((5,), float(np.log(0.5))))


def test_policy_weight_files_round_trip_with_the_capture(golden, tmp_path):
    """save_policy_weights writes what the reference's `torch.save(self._policy_fn.state_dict())` writes (rmt:452-457): the
    keys of `_policy_fn` alone, contiguous CPU tensors; a file holding the captured reference tensors strict-loads."""
    g = golden("fcnn_tiny")
    for name in VARIANTS:
        m = policy(spec_of(g, name))
        sd = captured_state_dict(g, name)
        pol = {k[len("_policy_fn."):]: v for k, v in sd.items() if k.startswith("_policy_fn.")}
        f = str(tmp_path / (name + "_ref.pt"))
        torch.save(pol, f)
        m.load_policy_weights(f)
        assert not m._policy_fn.training
        for k, v in m._policy_fn.state_dict().items():
            assert torch.equal(v, pol[k]), k
        f2 = str(tmp_path / (name + "_ours.pt"))
        m.save_policy_weights(f2)
        got = torch.load(f2)
        assert list(got) == list(pol)
        assert all(torch.equal(got[k], pol[k]) and got[k].is_contiguous() and got[k].device.type == "cpu" for k in pol)
        full = str(tmp_path / (name + "_full.pt"))
        torch.save(m.state_dict(), full)
        m2 = policy(spec_of(g, name))
        m2.load_state_dict(torch.load(full), strict=True)
