"""CPU-side checks of the planner (include/pvae.h pvae_plan*, physicsvae_amd/plan.py, engine_plan.py): the symbols, the struct
size, the refusals that need no device, the chunking arithmetic, the rule in torch against a brute-force restatement, and
the cases of tests/test_gpu_plan.py (each float32 twin within a quarter of the GPU bounds; each positive lam leaves two
candidates per environment a say)."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import imagine_cases as IC
import plan_cases as PC
from physicsvae_amd import _lib
from physicsvae_amd import plan as P
from physicsvae_amd.imagine import imagine_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"pvae_plan", "pvae_plan_sizeof", "pvae_plan_scratch_bytes", "pvae_plan_launches"}


def test_symbols_are_declared_exported_and_bound_at_abi_12():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "pvae.h")).read()
    stripped = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pvae_[a-z0-9_]+)\s*\(", stripped))
    assert NEW <= declared and NEW <= set(_lib.EXPORTS) and declared == set(_lib.EXPORTS)
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.pvae_abi_version() == _lib.ABI_VERSION == 12 and "#define PVAE_ABI_VERSION 12" in header
    assert lib.pvae_plan_sizeof(0) == C.sizeof(_lib.PlanArgs)
    assert lib.pvae_plan_sizeof(1) < 0 and b"which" in lib.pvae_last_error()
    body = re.search(r"typedef struct pvae_plan_args \{(.*?)\} pvae_plan_args;", stripped, flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f for f, _ in _lib.PlanArgs._fields_]
    assert "#define PVAE_PLAN_MAX_CANDIDATES %d" % _lib.PLAN_MAX_CANDIDATES in header
    # the unit is built with the others
    from physicsvae_amd import build
    assert "pvae_plan.hip" in build.UNITS and os.path.exists(os.path.join(build.CSRC, "pvae_plan.hip"))
    # the calls that need no device: a null context is refused by name
    assert lib.pvae_plan_scratch_bytes(None, 3, 5) == 0
    assert lib.pvae_plan(None, None, None) < 0 and b"null ctx" in lib.pvae_last_error()
    assert lib.pvae_plan_launches(None, None, None, None) < 0


def test_refusals_of_the_rule():
    ok = dict(envs=2, candidates=3, horizon=2, iters=1, sigma=1.0, lam=0.0)
    P.check_plan(**ok, max_batch=6)
    for key, bad, word in (("envs", 0, "envs"), ("candidates", 0, "candidates"), ("horizon", 0, "horizon"), ("iters", 0, "iters"),
                           ("sigma", -1.0, "sigma"), ("sigma", math.inf, "sigma"), ("sigma", math.nan, "sigma"),
                           ("lam", -1e-3, "lam"), ("lam", math.nan, "lam")):
        with pytest.raises(ValueError, match=word):
            P.check_plan(**dict(ok, **{key: bad}))
    with pytest.raises(ValueError, match="max_batch"):
        P.check_plan(**ok, max_batch=5)
    c = PC.case(PC.CONFIG_IDS[1])
    with pytest.raises(ValueError, match="cannot draw"):
        P.plan_torch(c.m.A, c.m.sd, c.s0, c.targets, c.H, c.K)


def test_chunking_arithmetic():
    assert P.plan_chunks(3, 11, 64) == [(0, 3, 0)]
    assert P.plan_chunks(7, 11, 64) == [(0, 5, 0), (5, 7, 55)]
    assert P.plan_chunks(130, 1, 64) == [(0, 64, 0), (64, 128, 64), (128, 130, 128)]
    assert P.plan_chunks(3, 64, 64) == [(0, 1, 0), (1, 2, 64), (2, 3, 128)]
    assert P.plan_chunks(2, 33, 64) == [(0, 1, 0), (1, 2, 33)]
    with pytest.raises(ValueError, match="max_batch"):
        P.plan_chunks(1, 65, 64)
    for E, K in ((9, 5), (64, 1), (1, 64), (13, 7)):                 # the chunks tile the environments, rows numbered globally
        ch = P.plan_chunks(E, K, 64)
        assert ch[0][0] == 0 and ch[-1][1] == E and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all((hi - lo) * K <= 64 and row0 == lo * K for lo, hi, row0 in ch)


def _brute(c):
    """The rule once more, with loops over environments and candidates and `imagine_torch` as the unroll."""
    m, H, K = c.m, c.H, c.K
    u = c.nominal.double().clone()
    cw = torch.ones(m.Db, dtype=torch.float64) if c.cw is None else c.cw.double()
    sw = torch.ones(H, dtype=torch.float64) if c.sw is None else c.sw.double()
    for i in range(c.iters):
        new = torch.empty_like(u)
        for e in range(c.E):
            zs = [u[:, e] + (0 if k == 0 else c.sigma * c.noise[i, :, e * K + k].double()) for k in range(K)]
            if m.A.prior == P.SPHERE:
                zs = [z / z.norm(dim=1, keepdim=True).clamp_min(1e-12) for z in zs]
            st = [imagine_torch(m.A, m.sd, "prior", c.s0[e: e + 1].double(), H, z=z[:, None])["states"][:, 0] for z in zs]
            cost = torch.stack([(sw[:, None] * cw * (s - c.targets[:, e].double()) ** 2).sum() / m.Db for s in st]).float()
            best = min(range(K), key=lambda k: (float(cost[k]), k))
            if c.lam == 0:
                new[:, e] = zs[best]
            else:
                w = torch.exp(-(cost.double() - cost[best].double()) / c.lam)
                new[:, e] = sum(w[k] * zs[k] for k in range(K)) / w.sum()
                if m.A.prior == P.SPHERE:
                    new[:, e] = new[:, e] / new[:, e].norm(dim=1, keepdim=True).clamp_min(1e-12)
        u = new
    return u, cost, best


@pytest.mark.parametrize("cid", [i for i in PC.CONFIG_IDS if "-3x11-" in i and "philox" not in i or i.startswith("sphere-1x5")])
def test_plan_torch_against_a_brute_force_restatement(cid):
    c = PC.case(cid)
    got = PC.plan64(c)
    u, cost, best = _brute(c)
    assert got["plan_z"].dtype == torch.float64 and got["cost"].dtype == torch.float32 and got["best"].dtype == torch.int32
    assert float((got["plan_z"] - u).abs().max()) <= 1e-12
    assert torch.allclose(got["cost"][-1], cost, rtol=2e-7, atol=0) and int(got["best"][-1]) == best
    assert tuple(got["iter_cost"].shape) == (c.iters, c.E) and tuple(got["z_cand"].shape) == (c.H, c.rows, c.m.Z)
    assert not bool(got["noise_out"].reshape(c.H, c.E, c.K, c.m.Z)[:, :, 0].any())


def test_ties_go_to_the_lowest_candidate_and_k1_is_imagine():
    c = PC.case("zero_mean-3x11-H1-i1-w")
    got = P.plan_torch(c.m.A, c.m.sd, c.s0, c.targets, c.H, c.K, sigma=0.0, nominal=c.nominal, noise=torch.zeros_like(c.noise))
    assert bool((got["cost"] == got["cost"][:, :1]).all()) and got["best"].tolist() == [0] * c.E
    assert torch.equal(P.plan_best_torch(torch.tensor([[3.0, 1.0, 1.0, 2.0], [0.5, 0.5, 0.5, 0.5]])), torch.tensor([1, 0], dtype=torch.int32))
    c = PC.case("helper-64x1-H3-i1-w")
    got = PC.plan64(c, dtype=torch.float32)
    ref = imagine_torch(c.m.A, c.m.sd, "prior", c.s0, c.H, z=c.nominal)
    assert torch.equal(got["states"], ref["states"]) and torch.equal(got["plan_z"], c.nominal)
    assert torch.equal(got["a0"], ref["actions"][0]) and torch.equal(got["s1"], ref["states"][0])


def test_cases_are_what_the_gpu_file_claims():
    cs = [PC.case(i) for i in PC.CONFIG_IDS]
    assert len(cs) == 42 and all(c.m.max_batch == 64 and c.rows <= 64 for c in cs)
    for name in PC.MODELS:
        mine = [c for c in cs if c.model == name]
        assert {(c.E, c.K) for c in mine} == set(PC.SHAPES)
        assert {c.H for c in mine} == {1, 3} and {c.iters for c in mine} == {1, 2}
        assert {c.weights for c in mine} == {True, False} and {c.lam > 0 for c in mine} == {True, False}
        assert sum(c.philox for c in mine) == 1
        assert any(c.cw is not None and int((c.cw == 0).sum()) == 1 for c in mine) or name == "db1"
    assert {c.m.prior for c in cs} == set(IC.I.PRIOR_KINDS) and any(c.m.mh is not None for c in cs)


@pytest.mark.parametrize("cid", PC.CONFIG_IDS)
def test_twin32_within_a_quarter(cid):
    e = PC.twin32_errors(cid)
    print(cid, e)
    for k, v in e.items():
        assert v <= PC.BOUNDS[k] / 4, (k, v)
    assert len(PC.RESEED) <= len(PC.CONFIG_IDS) // 8


@pytest.mark.parametrize("cid", [i for i in PC.CONFIG_IDS if "mppi" in i])
def test_positive_lam_keeps_two_candidates_in_play(cid):
    c = PC.case(cid)
    assert c.lam > 0 and c.lam == float(torch.tensor(c.lam, dtype=torch.float32)) and PC.weights_ok(c)
