"""The oracle's joint-phase state-reconstruction term (refpath.compute_loss, `s_rec_coeff` > 0 while the world model is
frozen; tpv:411-414, 421-434) against the capture of the reference's own trainer (tests/golden/srec_tiny.npz,
tools/gen_golden_srec.py).  Both sides run the same float32 torch graph on the CPU, so they are held to the suite's
standing bounds and no looser: loss terms 1e-5 relative, gradients 1e-4 of the tensor's largest entry."""
import json

import pytest
import torch

from oracle import refpath as R
from util import arch_from_meta, max_err_scaled

ALONE = dict(vae_kl_coeff=0.0, a_rec_coeff=0.0, s_rec_coeff=1.0, vae_cycle_coeff=0.0)


def capture_inputs(g, L):
    """The minibatch, draws and weights the capture was taken on, regenerated from their seeds."""
    arch = arch_from_meta(g["meta"])
    n_ep, n_steps, batch = [int(v) for v in g["meta"][9:12]]
    data = R.synth_demo(0, n_ep, n_steps, arch["Db"], arch["Da"], kind="dynamics")
    X, Y = R.build_windows(data, lookahead=L)
    x, y = next(iter(R.make_loader(X, Y, batch)))
    es = R.eps_stream(2, arch["Z"])
    eps = torch.stack([es(t, (x.shape[0], arch["Z"])) for t in range(L)])
    sd = R.perturb_biases(R.init_state_dict(arch, seed=1), seed=3)
    return arch, x, y, eps, sd


def scaled_outputs(arch, sd, scale):
    """The isolation case's weights: output layers of the motor decoder and the world model multiplied by `scale`."""
    sd = dict(sd)
    for net, key in (("_motor_decoder", "md"), ("_world_model", "wm")):
        k = "%s._model.%d._model.0.weight" % (net, arch[key][1])
        sd[k] = sd[k] * scale
    return sd


def captured_grads(g, pre):
    out, flat, at = {}, torch.from_numpy(g[pre + "grad"]), 0
    for k, shape in json.loads(str(g[pre + "keys"])):
        n = 1
        for s in shape:
            n *= s
        out[k] = flat[at: at + n].reshape(shape)
        at += n
    assert at == flat.numel()
    return out


@pytest.mark.parametrize("L", [1, 2])
def test_oracle_joint_s_rec_matches_the_reference_capture(golden, L):
    g = golden("srec_tiny")
    arch, x, y, eps, sd = capture_inputs(g, L)
    c = float(g["s_rec_coeff"])
    want = R.loss_and_grads(arch, sd, x, y, eps, world=False, coeff_cfg={"s_rec_coeff": c})
    none = R.loss_and_grads(arch, sd, x, y, eps, world=False)
    pre = "L%d/" % L
    assert float(want["total"]) == pytest.approx(float(g[pre + "total"]), rel=1e-5)
    assert float(none["total"]) == pytest.approx(float(g[pre + "total_without"]), rel=1e-5)
    assert float(none["loss_s"]) == 0.0 and float(want["loss_s"]) > 0.1
    # the reference returns the total only: its loss_s is what the coefficient added to it
    assert float(want["loss_s"]) == pytest.approx((float(g[pre + "total"]) - float(g[pre + "total_without"])) / c, rel=1e-5)
    ref = captured_grads(g, pre)
    assert list(want["grads"]) == list(ref) and not any(k.startswith("_world_model") for k in ref)
    for k, gr in ref.items():
        assert max_err_scaled(want["grads"][k], gr) < 1e-4, k


def test_at_lookahead_one_the_term_moves_no_gradient(golden):
    """s1 and a_gt are data and the world model is frozen: the term is a number in the loss, nothing else."""
    g = golden("srec_tiny")
    assert float(g["L1/grad_moved_by_term"]) == 0.0                 # the reference's autograd says so itself
    arch, x, y, eps, sd = capture_inputs(g, 1)
    a = R.loss_and_grads(arch, sd, x, y, eps, world=False, coeff_cfg={"s_rec_coeff": 0.5})
    b = R.loss_and_grads(arch, sd, x, y, eps, world=False)
    assert list(a["grads"]) == list(b["grads"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    assert float(a["total"]) == pytest.approx(float(b["total"]) + 0.5 * float(a["loss_s"]), rel=1e-6)


@pytest.mark.parametrize("L", [2, 3])
def test_oracle_isolated_term_matches_the_reference_capture(golden, L):
    """a_rec 0, kl 0, cyc 0, s_rec 1: every gradient entry arrives through the frozen world model's demonstrated-action
    pass of a later step.  Non-zero in the reference, and the oracle agrees entry by entry."""
    g = golden("srec_tiny")
    arch, x, y, eps, sd = capture_inputs(g, L)
    sd = scaled_outputs(arch, sd, float(g["out_scale"]))
    want = R.loss_and_grads(arch, sd, x, y, eps, world=False, coeff_cfg=ALONE)
    pre = "iso%d/" % L
    assert float(want["total"]) == pytest.approx(float(g[pre + "total"]), rel=1e-5)
    ref = captured_grads(g, pre)
    assert list(want["grads"]) == list(ref)
    assert max(float(v.abs().max()) for v in ref.values()) > 1e-4
    for k, gr in ref.items():
        assert float(gr.abs().max()) > 0.0, k
        assert max_err_scaled(want["grads"][k], gr) < 1e-4, k
