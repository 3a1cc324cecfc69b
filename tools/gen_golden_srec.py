"""tools/gen_golden_srec.py -- record tests/golden/srec_tiny.npz: the REFERENCE trainer's joint phase with
`world_model_s_rec_coeff` > 0 (tpv:411-414, 421-434 while the world model is frozen, tpv:347-350).

Dev tool: it imports the reference's train_physics_vae unmodified through the stand-in `ray` / `gym` packages of
oracle/stubs (location of the reference: $PVAE_REFERENCE, else the one oracle/gen_golden.py uses) and drives its own
TrainModel.compute_loss + autograd.  The test suite reads the fixture only.  The file holds data and nothing else.
Inputs are regenerated from seeds on both sides (oracle/refpath.py: synth_demo(0, 2, 15, kind="dynamics"), the first
minibatch of 8 windows, eps_stream(2, Z)(t) per unrolled step, weights perturb_biases(init_state_dict(arch, 1), 3)),
so the fixture stores what the reference computed:

  L<k>/total, L<k>/total_without    joint loss with world_model_s_rec_coeff = 0.5 and = 0.0, the other coefficients at
                                    their defaults (so (total - total_without) / 0.5 is loss_s), lookahead k = 1, 2
  L<k>/grad                         every gradient of the 0.5 run as one flat vector in named_parameters order
                                    (`L<k>/keys`: names and shapes -- the world model has none: it is frozen)
  L1/grad_moved_by_term             max |grad(0.5) - grad(0.0)| at lookahead 1: 0.0, the term has no gradient there
  iso<k>/total, iso<k>/grad, /keys  the term ISOLATED (a_rec 0, kl 0, cyc 0, s_rec 1) at lookahead k = 2, 3, with the
                                    output-layer weights of the motor decoder and the world model multiplied by 30:
                                    every entry of that gradient arrived through the frozen world model's
                                    demonstrated-action pass

    python tools/gen_golden_srec.py            write the fixture
    python tools/gen_golden_srec.py --verify   regenerate in memory and compare with the committed file byte for byte
"""
import argparse
import io
import json
import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "srec_tiny.npz")
N_EP, N_STEPS, BATCH = 2, 15, 8
S_REC = 0.5
OUT_SCALE = 30.0


def tiny_arch(R):
    return R.make_arch(7, 3, latent=4, te=(16, 2), md=(24, 2), wm=(32, 2))


def isolation_state_dict(R, arch, scale=OUT_SCALE):
    """Seeded initial weights with the output layers of the motor decoder and the world model scaled up: at normc
    std 0.01 the gradient that reaches the decoder through two world-model passes is ~1e-7."""
    sd = R.perturb_biases(R.init_state_dict(arch, seed=1), seed=3)
    for net, key in (("_motor_decoder", "md"), ("_world_model", "wm")):
        k = "%s._model.%d._model.0.weight" % (net, arch[key][1])
        sd[k] = sd[k] * scale
    return sd


def flat(tensors):
    return np.concatenate([t.detach().numpy().astype(np.float32).reshape(-1) for t in tensors])


def joint_capture(G, tr, x, y, eps, coeffs):
    """The reference's own compute_loss + backward in the joint phase under the given config coefficients."""
    import torch
    m = tr.model
    m.set_learnable_task_encoder(True)
    m.set_learnable_motor_decoder(True)
    m.set_learnable_world_model(False)
    tr.config.update(coeffs)                   # the keys read_loss_fn_coeff reads (tpv:331-335): a user's dict edit
    tr.read_loss_fn_coeff(world=False)
    m.train()
    for p in m.parameters():
        p.grad = None
    with G.EpsPatch(lambda c, shape: eps[c]):
        loss = tr.compute_loss(y, x)
    loss.backward()
    grads = G.grads_of(m)
    assert not any(k.startswith("_world_model") for k in grads)
    return float(loss.detach()), grads


def capture():
    sys.path.insert(0, ROOT)
    import oracle.gen_golden as G              # puts oracle/stubs and the reference on sys.path; its trainer factory
    import torch
    from oracle import refpath as R
    torch.set_num_threads(1)
    torch.manual_seed(0)
    arch = tiny_arch(R)
    data = R.synth_demo(seed=0, n_episodes=N_EP, n_steps=N_STEPS, dim_body=arch["Db"], dim_action=arch["Da"], kind="dynamics")
    es = R.eps_stream(2, arch["Z"])
    default = {"vae_kl_coeff": 1.0, "motor_decoder_a_rec_coeff": 1.0, "vae_cycle_coeff": 1e-3}
    alone = {"vae_kl_coeff": 0.0, "motor_decoder_a_rec_coeff": 0.0, "vae_cycle_coeff": 0.0, "world_model_s_rec_coeff": 1.0}
    fix = {"meta": np.array([arch["Db"], arch["Da"], arch["Z"], *arch["te"], *arch["md"], *arch["wm"], N_EP, N_STEPS, BATCH]),
           "s_rec_coeff": np.array(S_REC), "out_scale": np.array(OUT_SCALE)}
    with tempfile.TemporaryDirectory() as td:
        pkl = os.path.join(td, "demo.pkl")
        R.write_demo(pkl, data)
        for L in (1, 2, 3):
            tr = G.make_reference_trainer(pkl, arch, BATCH, m_world=2, lookahead=L)
            x, y = next(iter(tr.train_loader))
            eps = torch.stack([es(t, (x.shape[0], arch["Z"])) for t in range(L)])
            if L <= 2:
                tr.model.load_state_dict(R.perturb_biases(R.init_state_dict(arch, seed=1), seed=3))
                t0, g0 = joint_capture(G, tr, x, y, eps, dict(default, world_model_s_rec_coeff=0.0))
                t1, g1 = joint_capture(G, tr, x, y, eps, dict(default, world_model_s_rec_coeff=S_REC))
                assert list(g0) == list(g1)
                pre = "L%d/" % L
                fix[pre + "total"], fix[pre + "total_without"] = np.array(t1, dtype=np.float64), np.array(t0, dtype=np.float64)
                fix[pre + "keys"] = np.array(json.dumps([[k, list(g.shape)] for k, g in g1.items()]))
                fix[pre + "grad"] = flat(g1.values())
                if L == 1:
                    fix[pre + "grad_moved_by_term"] = np.array(max(float((g1[k] - g0[k]).abs().max()) for k in g1))
            if L >= 2:
                tr.model.load_state_dict(isolation_state_dict(R, arch))
                t2, g2 = joint_capture(G, tr, x, y, eps, alone)
                pre = "iso%d/" % L
                fix[pre + "total"] = np.array(t2, dtype=np.float64)
                fix[pre + "keys"] = np.array(json.dumps([[k, list(g.shape)] for k, g in g2.items()]))
                fix[pre + "grad"] = flat(g2.values())
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
        print("srec_tiny.npz: %s (%d bytes)" % ("byte-identical" if same else "DIFFERS from the reference's capture", len(data)))
        sys.exit(0 if same else 1)
    with open(OUT, "wb") as f:
        f.write(data)
    print("wrote %s: %d arrays, %d bytes" % (os.path.relpath(OUT, ROOT), len(np.load(io.BytesIO(data)).files), len(data)))


if __name__ == "__main__":
    main()
