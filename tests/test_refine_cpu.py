"""CPU-side checks of backpropagation through imagined rollouts and of gradient refinement (include/pvae.h
pvae_imagine_grad*, pvae_plan_refine*; physicsvae_amd/refine.py, engine_refine.py): the symbols and struct sizes, the
refusals that need no device, the rule in torch against finite differences and against `plan` / `imagine`, and the cases of
tests/test_gpu_refine.py -- each float32 twin within a quarter of the fixed GPU bounds, the chain figure that
refine_cases.CHAIN_BOUND is formed from, the learning rate's descent, and the drop cap of the ReLU-kink rule."""
import ctypes as C
import functools
import math
import os
import re

import pytest
import torch

import imagine_cases as IC
import refine_cases as RC
from physicsvae_amd import _lib
from physicsvae_amd import plan as P
from physicsvae_amd import refine as RF
from physicsvae_amd.imagine import imagine_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"pvae_imagine_grad", "pvae_imagine_grad_sizeof", "pvae_imagine_grad_scratch_bytes", "pvae_imagine_grad_launches",
       "pvae_plan_refine", "pvae_plan_refine_sizeof", "pvae_plan_refine_scratch_bytes", "pvae_plan_refine_launches"}


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_symbols_are_declared_exported_and_bound_at_abi_12():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "pvae.h")).read()
    stripped = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pvae_[a-z0-9_]+)\s*\(", stripped))
    assert NEW <= declared and NEW <= set(_lib.EXPORTS) and declared == set(_lib.EXPORTS)
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.pvae_abi_version() == _lib.ABI_VERSION == 12 and "#define PVAE_ABI_VERSION 12" in header
    for struct, cls, sizeof in (("pvae_imagine_grad_args", _lib.ImagineGradArgs, lib.pvae_imagine_grad_sizeof),
                                ("pvae_plan_refine_args", _lib.PlanRefineArgs, lib.pvae_plan_refine_sizeof)):
        assert sizeof(0) == C.sizeof(cls)
        assert sizeof(1) < 0 and b"which" in lib.pvae_last_error()
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), stripped, flags=re.S).group(1)
        names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == [f for f, _ in cls._fields_], struct
    from physicsvae_amd import build
    assert "pvae_refine.hip" in build.UNITS and os.path.exists(os.path.join(build.CSRC, "pvae_refine.hip"))
    # the calls that need no device: a null context is refused by name
    assert lib.pvae_imagine_grad_scratch_bytes(None, 3, 5) == 0 and lib.pvae_plan_refine_scratch_bytes(None, 3, 5) == 0
    assert lib.pvae_imagine_grad(None, None, None) < 0 and b"null ctx" in lib.pvae_last_error()
    assert lib.pvae_plan_refine(None, None, None) < 0 and b"null ctx" in lib.pvae_last_error()
    assert lib.pvae_imagine_grad_launches(None, None, None, None) < 0 and lib.pvae_plan_refine_launches(None, None, None) < 0


def test_refusals_of_the_rule():
    ok = dict(envs=2, horizon=2, steps=1, lr=0.1)
    RF.check_refine(**ok, max_batch=2)
    RF.check_refine(**dict(ok, steps=0))
    for key, bad, word in (("envs", 0, "envs"), ("horizon", 0, "horizon"), ("steps", -1, "steps"), ("lr", 0.0, "lr"),
                           ("lr", -1.0, "lr"), ("lr", math.inf, "lr"), ("lr", math.nan, "lr"), ("group", 0, "group")):
        with pytest.raises(ValueError, match=word):
            RF.check_refine(**dict(ok, **{key: bad}))
    with pytest.raises(ValueError, match="max_batch"):
        RF.check_refine(**ok, max_batch=1)
    with pytest.raises(ValueError, match="max_batch"):
        RF.check_refine(**ok, max_batch=5, group=3)
    assert RF.refine_chunks(7, 11, 64) == [(0, 5), (5, 7)] and RF.refine_chunks(130, 1, 64) == [(0, 64), (64, 128), (128, 130)]
    with pytest.raises(ValueError, match="max_batch"):
        RF.refine_chunks(1, 65, 64)


@pytest.mark.parametrize("weights", (False, True))
def test_rollout_grad_against_finite_differences(weights):
    m = IC.case("db1")
    g = torch.Generator().manual_seed(3)
    E, G, H = 2, 3, 3
    s0, z = torch.randn(E, m.Db, generator=g).double(), torch.randn(H, E * G, m.Z, generator=g).double()
    targets = torch.randn(H, E, m.Db, generator=g).double()
    cw = torch.rand(m.Db, generator=g).double() + 0.5 if weights else None
    sw = torch.rand(H, generator=g).double() + 0.5 if weights else None
    assert float(RC.rollout_margin(m, s0.repeat_interleave(G, dim=0), z).min()) > 1e-4          # (off the kinks: differences are smooth)
    out = RF.rollout_grad_torch(m.A, m.sd, s0, z, targets, G, cw, sw)

    def J(s0_, z_):
        st = P.plan_unroll_torch(m.A, RC.sd64(m), s0_.repeat_interleave(G, dim=0), z_)
        return RF.rollout_cost_torch(st, targets, G, cw, sw)
    assert torch.allclose(out["cost"].double(), J(s0, z), rtol=1e-6, atol=0)
    h = 1e-6
    for t in range(H):
        for j in range(m.Z):
            dz = torch.zeros_like(z)
            dz[t, :, j] = h
            fd = (J(s0, z + dz) - J(s0, z - dz)) / (2 * h)
            assert torch.allclose(out["dz"][t, :, j], fd, rtol=1e-5, atol=1e-8), (t, j)
    for e in range(E):                                        # ds[0]: a start state moves every row of its group
        d0 = torch.zeros_like(s0)
        d0[e, 0] = h
        fd = (J(s0 + d0, z) - J(s0 - d0, z)) / (2 * h)
        assert torch.allclose(out["ds"][0, e * G:(e + 1) * G, 0], fd[e * G:(e + 1) * G], rtol=1e-5, atol=1e-8)
        assert not bool(fd[:e * G].any()) and not bool(fd[(e + 1) * G:].any())


def test_rule_is_plan_and_imagine_with_one_candidate():
    for name in ("helper", "task_body", "sphere"):
        m = IC.case(name)
        E, H = 5, 3
        s0, z, targets = m.s0[:E], m.z[:H, :E], m.targets[:H, :E]
        out = RF.rollout_grad_torch(m.A, m.sd, s0, z, targets)
        ref = imagine_torch(m.A, m.sd, "prior", s0, H, z=z)
        assert torch.equal(out["states"], ref["states"])
        assert torch.equal(out["cost"], P.plan_cost_torch(ref["states"], targets, 1).float().reshape(-1))
        assert out["cost"].dtype == torch.float32 and tuple(out["dz"].shape) == (H, E, m.Z) and tuple(out["ds"].shape) == (H, E, m.Db)
        if name == "task_body":
            assert not bool(out["dz"].view(torch.int32).any())            # +0.0 everywhere
        else:
            assert bool((out["dz"] != 0).any())


@pytest.mark.parametrize("cid", ("sphere-E5-s3-H3-w", "zero_mean-E5-s3-H3", "task_body-E5-s3-H3", "helper-E1-s0-H1"))
def test_refine_rule_keeps_the_best_iterate(cid):
    c = RC.refine_case(cid)
    r = RC.refine64(c, dtype=torch.float32)
    ic = r["iter_cost"]
    assert tuple(ic.shape) == (c.steps + 1, c.E) and ic.dtype == torch.float32 and r["best_iter"].dtype == torch.int32
    want = torch.tensor([min(range(c.steps + 1), key=lambda i: (float(ic[i, e]), i)) for e in range(c.E)], dtype=torch.int32)
    assert torch.equal(r["best_iter"], want)
    pick = torch.arange(c.E)
    assert same_bits(r["plan_z"], r["z_iters"][r["best_iter"].long(), :, pick].permute(1, 0, 2))
    assert same_bits(r["cost"], ic[r["best_iter"].long(), pick]) and bool((r["cost"] <= ic[0]).all())
    if c.steps == 0:
        assert same_bits(r["plan_z"], RF.project_torch(c.m.A.prior, c.nominal)) and not bool(r["grad"].any())
    if c.model == "task_body":                                # nothing to descend along: the nominal stays, ties to iterate 0
        assert r["best_iter"].tolist() == [0] * c.E and same_bits(r["plan_z"], c.nominal)
    if c.m.A.prior == RF.SPHERE:
        assert float((r["z_iters"].norm(dim=-1) - 1).abs().max()) < 1e-6
    assert torch.equal(RF.best_iter_torch(torch.tensor([[3.0, 0.5], [1.0, 0.5], [1.0, 0.7]])), torch.tensor([1, 0], dtype=torch.int32))


def test_cases_are_what_the_gpu_file_claims():
    gc, rc = [RC.BY_ID[i] for i in RC.GRAD_IDS], [RC.BY_ID[i] for i in RC.REFINE_IDS]
    assert len(gc) == 32 and len(rc) == 72 and RC.MODELS == IC.CASE_IDS and len(RC.MODELS) == 8
    for name in RC.MODELS:
        assert IC.case(name).max_batch == 64
        mine = [c for c in gc if c.model == name]
        assert {(c.E, c.G) for c in mine} == {(1, 1), (5, 1), (3, 11), (64, 1)}
        assert {c.H for c in mine} == {1, 3} and {c.weights for c in mine} == {True, False}
        mine = [c for c in rc if c.model == name]
        assert {(c.E, c.steps) for c in mine} == {(E, s) for E in (1, 5, 33) for s in (0, 1, 3)}
        assert {c.H for c in mine} == {1, 3} and {c.weights for c in mine} == {True, False}
    c = RC.grad_case("zero_mean-3x11-H1-w")
    assert int((c.cw == 0).sum()) == 1 and tuple(c.z.shape) == (1, 33, 8) and tuple(c.s0.shape) == (3, 31)
    assert not RC.reads_code(IC.case("task_body")) and sum(RC.reads_code(IC.case(n)) for n in RC.MODELS) == 7


@functools.lru_cache(maxsize=None)
def twin(cid):
    return RC.grad_twin32_errors(cid) if cid in RC.GRAD_IDS else RC.refine_twin32_errors(cid)


@pytest.mark.parametrize("cid", RC.GRAD_IDS + RC.REFINE_IDS)
def test_twin32_within_a_quarter(cid):
    e = twin(cid)
    print(cid, e)
    for k in RC.FIXED:
        if k in e:
            assert e[k] <= RC.BOUNDS[k] / 4, (k, e[k])
    assert len(RC.RESEED) <= len(RC.GRAD_IDS + RC.REFINE_IDS) // 8


def test_chain_twin_observed():
    """The float32 twin's whole-chain figure over all configurations: what refine_cases.CHAIN_TWIN_OBSERVED states (never
    exceeded, and not overstated by more than the factor the float32 summation order of the host's BLAS may move it by)."""
    worst = max(max(twin(cid).get("chain", 0.0), twin(cid).get("grad", 0.0)) for cid in RC.GRAD_IDS + RC.REFINE_IDS)
    print("chain twin: observed %.3e, stated %.3e, bound %.3e" % (worst, RC.CHAIN_TWIN_OBSERVED, RC.CHAIN_BOUND))
    assert RC.CHAIN_TWIN_OBSERVED / 4 <= worst <= RC.CHAIN_TWIN_OBSERVED
    assert RC.CHAIN_BOUND == min(4 * RC.CHAIN_TWIN_OBSERVED, 1e-3)


def test_reference_keeps_every_case_within_the_drop_cap():
    """infer_cases' drop rule: the float64 reference alone leaves at most DROP_CAP of the candidates it looked at out."""
    over = []
    for cid in RC.GRAD_IDS:
        c = RC.grad_case(cid)
        if c.dropped > RC.drop_cap(c.rows):
            over.append((cid, round(c.dropped, 3)))
    for cid in RC.REFINE_IDS:
        c = RC.refine_case(cid)
        if c.dropped > RC.drop_cap(c.E):
            over.append((cid, round(c.dropped, 3)))
    print(over)
    assert not over, over


@pytest.mark.parametrize("cid", [i for i in RC.REFINE_IDS if RC.BY_ID[i].steps == 3])
def test_learning_rate_descends_in_float64(cid):
    c = RC.refine_case(cid)
    ic = RC.refine64(c)["iter_cost"].double().sum(dim=1)
    if RC.reads_code(c.m):
        assert float(ic[3]) < float(ic[0]), ic
    else:
        assert same_bits(ic[3:], ic[:1])
