"""tools/gen_golden_fcnn.py -- record tests/golden/fcnn_tiny.npz from the REFERENCE's FullyConnectedPolicy (rmt:323-457).

Dev tool: it imports the reference's rllib_model_torch unmodified through the stand-in `ray` / `gym` packages of
oracle/stubs (location of the reference: $PVAE_REFERENCE, else the one oracle/gen_golden.py uses).  The test suite reads
the fixture only.  The file holds data and nothing else: per log_std_type a small seeded policy's state dict, a 7-row and a
40-row observation, the reference's logits and value on them, and torch autograd's gradients of
(logits * c1).sum() + (value * c2).sum() with respect to every parameter and the observation, plus the layer specs as JSON.
State dict and parameter gradients are stored as one flat vector each, in state-dict key order (`<variant>/keys` holds the
keys and shapes).

    python tools/gen_golden_fcnn.py            write the fixture
    python tools/gen_golden_fcnn.py --verify   regenerate in memory and compare with the committed file byte for byte
"""
import argparse
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "fcnn_tiny.npz")
OBS, NUM_OUTPUTS, ROWS = 22, 10, (7, 40)


def fc(width, act):
    return {"type": "fc", "hidden_size": width, "activation": act, "init_weight": {"name": "normc", "std": 1.0}}


def out_layer():
    return {"type": "fc", "hidden_size": "output", "activation": "linear", "init_weight": {"name": "normc", "std": 0.3}}


# (output layers at std 0.3 instead of the default 0.01: gradients of every layer at comparable magnitudes)
VARIANTS = {
    "constant": {"log_std_type": "constant", "sample_std": [0.5, 0.75, 1.0, 1.25, 1.5],
                 "policy_fn_layers": [fc(48, "relu"), fc(40, "tanh"), out_layer()],
                 "value_fn_layers": [fc(24, "elu"), fc(16, "relu"), out_layer()]},
    "state_independent": {"log_std_type": "state_independent", "sample_std": 0.7,
                          "policy_fn_layers": [fc(40, "tanh"), fc(24, "elu"), out_layer()],
                          "value_fn_layers": [fc(24, "relu"), fc(16, "tanh"), out_layer()]},
    "state_dependent": {"log_std_type": "state_dependent", "sample_std": 0.5,
                        "policy_fn_layers": [fc(40, "relu"), fc(32, "elu"), out_layer()],
                        "value_fn_layers": [fc(24, "tanh"), fc(24, "relu"), out_layer()],
                        "log_std_fn_layers": [fc(24, "relu"), fc(16, "tanh"), out_layer()]},
}


def reference_module():
    import oracle.gen_golden  # noqa: F401  (puts oracle/stubs and the reference on sys.path, as the other fixtures' generator)
    if not hasattr(np, "product"):
        np.product = np.prod                  # numpy 2 dropped it; rmt:384 uses it
    import rllib_model_torch as RMT
    return RMT


def flat(tensors):
    return np.concatenate([t.detach().numpy().astype(np.float32).reshape(-1) for t in tensors])


def capture():
    sys.path.insert(0, ROOT)
    RMT = reference_module()
    import torch
    from gym.spaces import Box
    torch.set_num_threads(1)
    fix = {}
    for v, (name, cmc) in enumerate(VARIANTS.items()):
        torch.manual_seed(100 + v)
        np.random.seed(100 + v)
        box = Box(-np.ones(OBS, dtype=np.float32), np.ones(OBS, dtype=np.float32))
        m = RMT.FullyConnectedPolicy(box, Box(-np.ones(NUM_OUTPUTS // 2, dtype=np.float32), np.ones(NUM_OUTPUTS // 2, dtype=np.float32)),
                                     NUM_OUTPUTS, {"custom_model_config": dict(cmc)}, "fcnn")
        g = torch.Generator().manual_seed(200 + v)
        with torch.no_grad():                 # biases away from zero (ray's SlimFC starts them at 0)
            for k, p in m.named_parameters():
                if k.endswith("bias"):
                    p.copy_(0.1 * torch.randn(p.shape, generator=g))
        fix[name + "/spec"] = np.array(json.dumps(cmc, sort_keys=True))
        fix[name + "/sample_std"] = np.asarray(cmc["sample_std"], dtype=np.float64)
        # the state dict as ONE flat vector in key order (+ keys and shapes): fewer members, a smaller file
        fix[name + "/keys"] = np.array(json.dumps([[k, list(t.shape)] for k, t in m.state_dict().items()]))
        fix[name + "/sd"] = flat(m.state_dict().values())
        for rows in ROWS:
            x = torch.randn(rows, OBS, generator=g).requires_grad_(True)
            c1 = torch.randn(rows, NUM_OUTPUTS, generator=g)
            c2 = torch.randn(rows, generator=g)
            for p in m.parameters():
                p.grad = None
            logits, _ = m.forward({"obs_flat": x}, [], None)
            value = m.value_function()
            ((logits * c1).sum() + (value * c2).sum()).backward()
            tag = "%s/r%d/" % (name, rows)
            fix[tag + "x"], fix[tag + "c1"], fix[tag + "c2"] = x.detach().numpy(), c1.numpy(), c2.numpy()
            fix[tag + "logits"], fix[tag + "value"] = logits.detach().numpy(), value.detach().numpy()
            fix[tag + "gx"] = x.grad.numpy()
            fix[tag + "g"] = flat(p.grad for _, p in m.named_parameters())      # (named_parameters order == state-dict order)
    return fix


def npz_bytes(fix):
    """A .npz np.load reads, with fixed member times: the same arrays give the same bytes (np.savez stamps the clock)."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(fix):
            a = io.BytesIO()
            np.lib.format.write_array(a, np.asarray(fix[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, a.getvalue())
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--verify", action="store_true", help="regenerate and compare with the committed fixture byte for byte")
    args = ap.parse_args()
    data = npz_bytes(capture())
    if args.verify:
        with open(OUT, "rb") as f:
            same = f.read() == data
        print("fcnn_tiny.npz: %s (%d bytes)" % ("byte-identical" if same else "DIFFERS from the reference's capture", len(data)))
        sys.exit(0 if same else 1)
    with open(OUT, "wb") as f:
        f.write(data)
    print("wrote %s: %d arrays, %d bytes" % (os.path.relpath(OUT, ROOT), len(np.load(io.BytesIO(data)).files), len(data)))


if __name__ == "__main__":
    main()
