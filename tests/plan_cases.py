"""Cases of the planner's tests (tests/test_gpu_plan.py, checked without a GPU by tests/test_plan_cpu.py): seven models of
tests/imagine_cases.py (max_batch 64; `task_body` is left out -- its decoder does not read the code) under six
configurations each:

  (E, K) in {(1, 1), (1, 5), (3, 11), (2, 32), (64, 1)} -- 1, 5, 33 and 64 rows: partial hand-over workgroups, environment
  boundaries inside a wave group, K = 1, one full batch -- with H in {1, 3}, iters in {1, 2}, weights absent or given (one
  entry of cw zero), lam zero or positive, rotating over the models so that every value meets every model; noise supplied;
  and one configuration per model, (3, 11) at H = 3 and two iterations, that draws from Philox (on the CPU a stand-in draw
  of the same distribution takes the place of `noise_out`).

A positive lam is chosen on the CPU from the case's float64 costs of iteration 0: the largest, over the environments, gap
between the best and the second-best cost -- the second-best candidate then keeps exp(-1) of the best's weight or more;
rounded to float32 so that host and device divide by the same number.  tests/test_plan_cpu.py asserts for every iteration
that at least two candidates of every environment keep a normalised weight above 1e-3.

Bounds (infer_cases.py), stage by stage on the stage's own inputs, because selection is discontinuous: z_cand, one step's
states, a0 / s1 within ROLLOUT_BOUND (2e-5, max_err_scaled) of float64; cost within FORWARD_BOUND (1e-5) relative of the
float64 cost of the same states; plan_z within FORWARD_BOUND (max_err_scaled) of `plan_select_torch` in float64 on the same
costs and candidates.  A case whose float32 twin does not stay within a quarter of these is reseeded (RESEED), never
loosened."""
import functools
import types

import torch

import imagine_cases as IC
import infer_cases as I
from physicsvae_amd import plan as P
from physicsvae_amd.imagine import step_torch
from vae_ppo_cases import scaled

ROLLOUT_BOUND, FORWARD_BOUND = I.ROLLOUT_BOUND, I.FORWARD_BOUND
MODELS = ("zero_mean", "state_mean", "sphere", "none", "body_task", "helper", "db1")
SHAPES = ((1, 1), (1, 5), (3, 11), (2, 32), (64, 1))
HORIZONS, ITERS = (1, 3), (1, 2)
SIGMA = 0.7
MIN_WEIGHT = 1e-3
RESEED = {}                     # configuration id -> seeds further (none needed: tests/test_plan_cpu.py::test_twin32_within_a_quarter)


def _configs():
    out = []
    for m, name in enumerate(MODELS):
        for j, (E, K) in enumerate(SHAPES):
            out.append(types.SimpleNamespace(
                model=name, E=E, K=K, H=HORIZONS[(j + m) % 2], iters=ITERS[(j + m // 2) % 2], weights=(j + m // 2) % 2 == 0,
                mppi=K > 1 and (j + m) % 2 == 1, philox=False))
        out.append(types.SimpleNamespace(model=name, E=3, K=11, H=3, iters=2, weights=m % 2 == 1, mppi=m % 2 == 1, philox=True))
    for c in out:
        c.id = "%s-%dx%d-H%d-i%d%s%s%s" % (c.model, c.E, c.K, c.H, c.iters, "-w" if c.weights else "", "-mppi" if c.mppi else "",
                                           "-philox" if c.philox else "")
    return out


CONFIGS = _configs()
CONFIG_IDS = tuple(c.id for c in CONFIGS)
BY_ID = {c.id: c for c in CONFIGS}


@functools.lru_cache(maxsize=None)
def case(cid):
    """The configuration with its data: the model (imagine_cases.case), s0 [E, Db], targets [H, E, Db], nominal [H, E, Z],
    noise [iters, H, rows, Z], cw / sw (None without weights), sigma, lam.  Built once, left unchanged."""
    cfg = BY_ID[cid]
    m = IC.case(cfg.model)
    c = types.SimpleNamespace(**vars(cfg))
    c.m, c.rows = m, cfg.E * cfg.K
    g = torch.Generator().manual_seed(7700 + 10 * CONFIG_IDS.index(cid) + RESEED.get(cid, 0))
    rn = lambda *shape: torch.randn(*shape, generator=g)                              # noqa: E731
    c.s0, c.targets, c.nominal = rn(c.E, m.Db), rn(c.H, c.E, m.Db), 0.5 * rn(c.H, c.E, m.Z)
    c.noise = rn(c.iters, c.H, c.rows, m.Z)
    c.cw = c.sw = None
    if c.weights:
        c.cw, c.sw = torch.rand(m.Db, generator=g) + 0.25, torch.rand(c.H, generator=g) + 0.25
        if m.Db > 1:                # (db1 has one column: its weight stays positive)
            c.cw[m.Db // 2] = 0.0
    c.sigma, c.lam = SIGMA, 0.0
    if c.mppi:
        r = plan64(c, lam=0.0, iters=1)
        two = torch.sort(r["cost"].double(), dim=1).values[:, :2]
        c.lam = float((two[:, 1] - two[:, 0]).max().float())
        assert c.lam > 0
    return c


def plan64(c, lam=None, iters=None, dtype=torch.float64, noise=None):
    t = lambda x: None if x is None else x.to(dtype)                                  # noqa: E731
    iters = c.iters if iters is None else iters
    noise = c.noise if noise is None else noise
    return P.plan_torch(c.m.A, c.m.sd, t(c.s0), t(c.targets), c.H, c.K, iters=iters, sigma=c.sigma, lam=c.lam if lam is None else lam,
                        nominal=t(c.nominal), noise=t(noise[:iters]), col_weight=t(c.cw), step_weight=t(c.sw))


def stage_errors(c, got, u_in, noise):
    """The checks of the module docstring on one call's results `got` (float32: the float32 twin's, or the device's), stage by
    stage in float64 on the stage's own inputs.  u_in [H, E, Z]: the nominal that entered the LAST iteration; noise [H, rows,
    Z]: what that iteration added (`noise_out`).  {stage: error by that stage's measure}."""
    m, d = c.m, lambda x: x.double()                                                  # noqa: E731
    sd = {k: v.double() for k, v in m.sd.items()}
    e = {}
    z64, n64 = P.plan_candidates_torch(m.A.prior, d(u_in), d(noise), c.sigma, c.K)
    e["z_cand"] = scaled(got["z_cand"], z64)
    s0_rows = d(c.s0).repeat_interleave(c.K, dim=0)
    e["states"] = scaled(got["states"], P.plan_unroll_torch(m.A, sd, s0_rows, d(got["z_cand"]), teacher=d(got["states"])))
    j64 = P.plan_cost_torch(got["states"], c.targets, c.K, c.cw, c.sw)
    e["cost"] = float(((d(got["cost"]) - j64).abs() / j64).max())
    u64, best = P.plan_select_torch(got["cost"], d(got["z_cand"]), c.lam, m.A.prior)
    e["best"] = 0.0 if torch.equal(best, got["best"]) else 1.0
    e["plan_z"] = scaled(got["plan_z"], u64)
    a64, _, s64 = step_torch(m.A, sd, "prior", d(c.s0), z=d(got["plan_z"][0]))
    e["a0"], e["s1"] = scaled(got["a0"], a64), scaled(got["s1"], s64)
    return e


BOUNDS = {"z_cand": ROLLOUT_BOUND, "states": ROLLOUT_BOUND, "cost": FORWARD_BOUND, "best": 0.0, "plan_z": FORWARD_BOUND,
          "a0": ROLLOUT_BOUND, "s1": ROLLOUT_BOUND}


def nominal_before_last(c, plan):
    """The nominal that enters the last iteration: the case's own for one iteration, else plan_z of a call with one iteration
    fewer (`plan`: callable(iters) -> results)."""
    return c.nominal if c.iters == 1 else plan(c.iters - 1)["plan_z"]


def twin32_errors(cid):
    c = case(cid)
    got = plan64(c, dtype=torch.float32)
    u_in = nominal_before_last(c, lambda iters: plan64(c, iters=iters, dtype=torch.float32))
    return stage_errors(c, got, u_in, got["noise_out"])


def weights_ok(c):
    """Every iteration of the float64 plan leaves at least two candidates per environment a normalised weight > MIN_WEIGHT."""
    for iters in range(1, c.iters + 1):
        w = P.plan_weights_torch(plan64(c, iters=iters)["cost"], c.lam)
        w = w / w.sum(dim=1, keepdim=True)
        if int((w > MIN_WEIGHT).sum(dim=1).min()) < 2:
            return False
    return True
