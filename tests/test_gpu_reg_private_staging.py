"""Wave-private staging of the register-staged split-K bodies (pvae_gemm_reg.h): every wave stages exactly the chunks of a
k-tile that it reads back, and the k-loops hold no workgroup barrier -- only the one in front of the split-K reduction
buffer, which overlays the staging ring.  A wrong lane -> chunk map gives wrong sums; a missing ordering point or barrier
gives results that change from run to run.

16x16 body (splitk_reg16_body) through gemm_probe, at the shapes the planner sends to 16x16 tiles (64 rows x 64 outputs:
16 workgroups): forward with bias + ReLU (P_ROW) and input gradient with mask (P_COL), contraction lengths of nk = 1, 2, 3,
4, 5, 8, 9 and 16 k-tiles of 64 -- the clamped prologue at nk <= D = 4, the guarded tail, odd and even counts of full groups.
The output sits in a NaN-filled buffer one row longer and 64 columns wider: afterwards everything inside is finite and
everything around it still NaN.  Each case is held against a float64 contraction at 2e-6 sqrt(K) of the tensor's max, the
bound of the neighbouring kernel tests (their measured errors are 1e-7 ... 4e-7), and ten runs must agree to the bit.

32x32 body (splitk_reg_body<false>: the input-gradient half of the fused pairs) through the engine: 128 rows x 1024 is the
smallest output that gives the pair 128 tiles of 32x32, below which the planner chooses 16x16 tiles (tests/tile_rules.py).
Two hidden layers, one optimizer step, both phases, with the context option "pair" = 1 and = 0: without pairs the same
input gradient comes from the LDS-DMA kernel and a stand-alone weight gradient, whose sums are the same by construction.
World phase: parameters, both moments and the loss terms must be equal bit for bit, ten pair runs from the same state
against the one unpaired run.  Joint phase: the loss terms must equal the unpaired run's bit for bit and the ten pair
runs must equal one another bit for bit in parameters, moments and loss terms -- but parameters and moments are NOT held
against the unpaired run there, because "pair" = 0 also takes the hand-overs between the stacks (action seed, sampler
seed: StepPlan::seed_sampler needs pair launches) off the tile epilogues and onto the stand-alone glue kernels, which round
differently.  Measured at 128 rows with the library as it was before the staging change and with this one, the same
figures from both: 6400 of 1181760 encoder and 33042 decoder parameters differ between "pair" = 0 and 1, by at most
3.0e-8 and 1.2e-7; stored gradients (no fused Adam) differ in 151851 / 659513 places by at most 3.7e-9 / 7.5e-9.  The
hidden pairs of the joint phase are the kernel instance the world phase runs (bwd_pair_kernel<EpiMask, .>).
(The 64x32 body of the pairs at 512 rows and more, splitk_reg64_body, keeps its barriers -- the same change measured
slower there, docs/experiments.md round 12 -- and has no case here.)"""
import pytest
import torch

import tile_rules as TR
from oracle import refpath as R
from physicsvae_amd import _lib
from physicsvae_amd.engine import gemm_probe, make_step_params
from util import make_trainer, max_err_scaled

pytestmark = pytest.mark.gpu

M = OUT = 64
NKS = (1, 2, 3, 4, 5, 8, 9, 16)
REPEATS = 10


def _inputs(nk):
    k = 64 * nk
    g = torch.Generator().manual_seed(1009 * nk + 7)
    x, w, b = torch.randn(M, k, generator=g), torch.randn(OUT, k, generator=g), torch.randn(OUT, generator=g)
    dz, wd, act = torch.randn(M, k, generator=g), torch.randn(k, OUT, generator=g), torch.randn(M, OUT, generator=g)
    return x, w, b, dz, wd, act


@pytest.fixture(scope="module")
def wanted():
    """{nk: float64 (forward, input gradient)}, computed once."""
    out = {}
    for nk in NKS:
        x, w, b, dz, wd, act = _inputs(nk)
        out[nk] = ((x.double() @ w.double().t() + b.double()).clamp_min(0), (dz.double() @ wd.double()) * (act > 0))
    return out


def _guarded(run):
    """`run(view)` writes the M x OUT result into a view of a NaN-filled buffer with a guard row and 64 guard columns."""
    buf = torch.full((M + 1, OUT + 64), float("nan"), device="cuda")
    run(buf[:M, :OUT])
    torch.cuda.synchronize()
    return buf.cpu()


@pytest.mark.parametrize("kind", [0, 1], ids=["forward-bias-relu", "input-gradient-mask"])
@pytest.mark.parametrize("nk", NKS)
def test_16x16_body_edges_guards_and_repeats(wanted, nk, kind):
    assert TR.plan_tiles("forward", M, OUT)[0] == "16x16" and TR.plan_tiles("dgrad", M, OUT)[0] == "16x16"
    k = 64 * nk
    x, w, b, dz, wd, act = (t.cuda() for t in _inputs(nk))
    if kind == 0:
        run = lambda o: gemm_probe(0, x, w, o, bias_or_mask=b, relu=True, m=M, n=OUT, k=k)            # noqa: E731
    else:
        run = lambda o: gemm_probe(1, dz, wd, o, bias_or_mask=act, m=M, n=k, k=OUT)                   # noqa: E731
    first = _guarded(run)
    inside = torch.zeros_like(first, dtype=torch.bool)
    inside[:M, :OUT] = True
    assert torch.isfinite(first[inside]).all()
    assert torch.isnan(first[~inside]).all()
    err, tol = max_err_scaled(first[:M, :OUT], wanted[nk][kind]), 2e-6 * (k ** 0.5)
    print("kind %d nk %d: %.3g (bound %.3g)" % (kind, nk, err, tol))
    assert err < tol
    for rep in range(1, REPEATS):
        again = _guarded(run)
        assert torch.equal(again[:M, :OUT], first[:M, :OUT]), rep
        assert torch.isnan(again[~inside]).all(), rep


def test_pair_input_gradient_equals_the_unpaired_schedule_bit_for_bit():
    rows = 128
    assert TR.plan_tiles("pair", rows, 1024)[0] == "32x32"
    assert TR.plan_tiles("pair", rows - 32, 1024)[0] == "16x16"                # one row block fewer: 16x16 tiles
    lib = _lib.load()
    Db, Da, Z = 23, 7, 8
    arch = R.make_arch(Db, Da, latent=Z, te=(1024, 2), md=(1024, 2), wm=(1024, 2))
    data = R.synth_demo(5, 2, rows + 4, Db, Da, kind="dynamics")
    X, Y = R.build_windows(data, lookahead=1)
    x, y = next(iter(R.make_loader(X, Y, rows)))
    assert x.shape[0] == rows
    sd = R.perturb_biases(R.init_state_dict(arch, seed=6), seed=8)
    eps = R.eps_stream(7, Z)(0, (rows, Z))
    tr = make_trainer(arch, data, rows, device="cuda")
    eng = tr.engine
    try:
        for world in (False, True):
            phase = _lib.PHASE_WORLD if world else _lib.PHASE_JOINT
            co = R.phase_coeffs(world)
            sp = make_step_params(lr=5e-4, adam_t=(1, 1, 1), a_rec=co["a_rec_coeff"], kl=co["vae_kl_coeff"],
                                  s_rec=co["s_rec_coeff"], cyc=co["vae_cycle_coeff"], global_rows=rows)

            def run(pair):
                assert lib.pvae_set_option(eng.ctx, b"pair", pair) >= 0
                tr.model.load_state_dict(sd)
                eng.exp_avg.zero_()
                eng.exp_avg_sq.zero_()
                eng.set_batch(x, y)
                loss = eng.forward_backward(phase, rows, sp, eps=None if world else eps, fused_adam=True)
                torch.cuda.synchronize()
                return eng.params.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone(), loss.clone()
            tr.model.load_state_dict(sd)
            before = eng.params.clone()
            alone = run(0)
            assert not torch.equal(alone[0], before)
            first = run(1)
            assert torch.equal(first[3], alone[3]), world              # loss terms: both phases
            want = alone if world else first                            # (joint: see the module docstring)
            for rep in range(REPEATS):
                for u, v in zip(first if rep == 0 else run(1), want):
                    assert torch.equal(u, v), (world, rep)
    finally:
        lib.pvae_set_option(eng.ctx, b"pair", 1)
