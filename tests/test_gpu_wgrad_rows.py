"""The epilogue of the 64x64 weight-gradient body (pvae_gemm_wgrad.h, wgrad_reg_body): the finished tile goes through LDS
and leaves as whole 256-byte rows -- thread t stores columns 4 (t & 15) .. + 3 of rows (t >> 4) + 16 i -- and the
epilogue's operands (Adam's p, m, v) are fetched under the loop with the same mapping.

Through gemm_probe(kind=2) (gemm_wgrad with the gradient-store epilogue; a contraction length that is no multiple of 64,
or option wgrad32 = 0, selects this body): contraction lengths of 1, 3 and 5 k-tiles (BK = 32: the guarded tail, odd
group counts) times 1, 6 and 3 output tiles, and one case with wgrad32 = 0 at 64 rows.  The output sits in a NaN-filled
buffer one row longer and 64 columns wider than the gradient: afterwards every element of the gradient is finite and
everything around it is still NaN (no store outside a tile, no tile left unwritten).  Values are held against a float64
contraction at the tolerance of the neighbouring kernel tests, 2e-6 sqrt(M) of the tensor's max, and two runs must agree
to the bit (the LDS pass and its barrier are race-free).

Through the engine, one case with operands in the epilogue: two hidden layers of width 192 / 128 at 96 rows with
wgrad32 = 0, one optimizer step with Adam fused into the backward launches (deferred workgroups, and with
PVAE_DEFER_ADAM=0 in the weight-gradient epilogue itself) against the gradient-store schedule plus flat Adam:
parameters and both moments equal bit for bit."""
import os

import pytest
import torch

from oracle import refpath as R
from physicsvae_amd import _lib
from physicsvae_amd.engine import gemm_probe, make_step_params
from util import make_trainer, max_err_scaled

pytestmark = pytest.mark.gpu

# (M, N, Kin, wgrad32)
CASES = [(m, n, k, 1) for m in (32, 96, 160) for (n, k) in ((64, 64), (128, 192), (192, 64))] + [(64, 128, 128, 0)]


@pytest.fixture(scope="module")
def cases():
    """{case: (dz, x, float64 gradient)}, computed once."""
    out = {}
    for m, n, k, w32 in CASES:
        g = torch.Generator().manual_seed(31 * m + 7 * n + k)
        dz, x = torch.randn(m, n, generator=g), torch.randn(m, k, generator=g)
        out[(m, n, k, w32)] = (dz, x, dz.double().t() @ x.double())
    return out


def _run(dz, x, m, n, k, w32):
    lib = _lib.load()
    buf = torch.full((n + 1, k + 64), float("nan"), device="cuda")
    try:
        if not w32:
            assert lib.pvae_set_option(None, b"wgrad32", 0) >= 0
        gemm_probe(2, dz, x, buf, m=m, n=n, k=k)
        torch.cuda.synchronize()
    finally:
        if not w32:
            lib.pvae_set_option(None, b"wgrad32", 1)
    return buf.cpu()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "M%d-N%d-K%d-wgrad32=%d" % c)
def test_tile_rows_land_inside_the_gradient_and_nowhere_else(cases, case):
    m, n, k, w32 = case
    dz, x, want = cases[case]
    dzd, xd = dz.cuda(), x.cuda()
    a = _run(dzd, xd, m, n, k, w32)
    b = _run(dzd, xd, m, n, k, w32)
    inside = torch.zeros_like(a, dtype=torch.bool)
    inside[:n, :k] = True
    assert torch.isfinite(a[inside]).all()                   # no tile (or row of one) left unwritten
    assert torch.isnan(a[~inside]).all()                     # nothing stored outside [N][Kin]
    err, tol = max_err_scaled(a[:n, :k], want), 2e-6 * (m ** 0.5)
    print("M %d N %d Kin %d wgrad32 %d: %.3g (bound %.3g)" % (m, n, k, w32, err, tol))
    assert err < tol
    assert torch.equal(a[:n, :k], b[:n, :k])                 # two runs, the same bits


@pytest.mark.parametrize("defer", [None, "0"], ids=["deferred-adam", "adam-in-epilogue"])
def test_adam_through_the_epilogue_equals_gradient_store_plus_flat_adam(defer):
    lib = _lib.load()
    rows, Db, Da, Z = 96, 20, 6, 8
    arch = R.make_arch(Db, Da, latent=Z, te=(192, 2), md=(128, 2), wm=(192, 2))
    data = R.synth_demo(5, 2, rows + 4, Db, Da, kind="dynamics")
    X, Y = R.build_windows(data, lookahead=1)
    x, y = next(iter(R.make_loader(X, Y, rows)))
    assert x.shape[0] == rows
    sd = R.perturb_biases(R.init_state_dict(arch, seed=6), seed=8)
    eps = R.eps_stream(7, Z)(0, (rows, Z))
    saved = os.environ.get("PVAE_DEFER_ADAM")
    try:
        assert lib.pvae_set_option(None, b"wgrad32", 0) >= 0
        if defer is not None:
            os.environ["PVAE_DEFER_ADAM"] = defer                 # (read when the trainer creates its context)
        tr = make_trainer(arch, data, rows, device="cuda")
        eng = tr.engine
        for world in (False, True):
            phase = _lib.PHASE_WORLD if world else _lib.PHASE_JOINT
            nets = [_lib.NET_WM] if world else [_lib.NET_TE, _lib.NET_MD]
            co = R.phase_coeffs(world)
            sp = make_step_params(lr=5e-4, adam_t=(1, 1, 1), a_rec=co["a_rec_coeff"], kl=co["vae_kl_coeff"],
                                  s_rec=co["s_rec_coeff"], cyc=co["vae_cycle_coeff"], global_rows=rows)

            def run(fused):
                tr.model.load_state_dict(sd)
                eng.exp_avg.zero_()
                eng.exp_avg_sq.zero_()
                eng.set_batch(x, y)
                eng.forward_backward(phase, rows, sp, eps=None if world else eps, fused_adam=fused)
                if not fused:
                    eng.adam(nets, sp)
                return eng.params.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone()
            tr.model.load_state_dict(sd)
            before = eng.params.clone()
            fused, flat = run(True), run(False)
            for u, v in zip(fused, flat):
                assert torch.equal(u, v), world
            assert not torch.equal(fused[0], before)
    finally:
        lib.pvae_set_option(None, b"wgrad32", 1)
        if saved is None:
            os.environ.pop("PVAE_DEFER_ADAM", None)
        else:
            os.environ["PVAE_DEFER_ADAM"] = saved
