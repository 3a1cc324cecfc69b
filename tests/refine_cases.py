"""Cases of the tests of backpropagation through imagined rollouts and of gradient refinement (tests/test_gpu_refine.py,
checked without a GPU by tests/test_refine_cpu.py): the eight models of tests/imagine_cases.py (max_batch 64; `task_body`'s
decoder does not read the code: dz is a structural zero).

Gradient configurations, four per model: (E, G) in {(1, 1), (5, 1), (3, 11), (64, 1)} -- 1, 5, 33 and 64 rows: partial
hand-over workgroups, group boundaries inside a wave group, one full batch -- with H in {1, 3} (H = 1 has no recompute and no
carry) and the weights absent or given (one entry of cw zero), rotating over the models so that every value meets every
model.  Refinement configurations, nine per model: E in {1, 5, 33} x steps in {0, 1, 3}, H and the weights rotating.

ReLU kinks (infer_cases.py's drop rule).  A configuration draws three times the candidates it needs (+ 16) -- environments,
and for G > 1 codes per environment -- runs the float64 rule on them, and keeps the first ones whose smallest
|pre-activation| over every ReLU layer of the decoder, the helper and the world model, over every step (for a refinement: of
the unroll at iterate steps - 1, the one whose gradient is compared with float64), is at least ppo_cases.KINK.  `dropped`
records the share of the candidates it looked at that it left out, and the CPU file holds that share to
infer_cases.DROP_CAP (environments are independent of one another in both rules, so the selection changes nothing for the
ones kept); a configuration over the cap is reseeded, as there.  The device's states are within rounding of the float64
ones, a thousandth of KINK, so the rows kept are off the kinks there too.

The data's scale (SCALES).  With start states and codes of size one the imagined states shrink to a std of about 0.05 by
step 2 (the world model's output layer is 30 x normc(0.01)), the pre-activations behind them are then of the size of the
perturbed biases, 0.05, and 19 to 46 % of the rows come within KINK of a kink over three steps -- no seed keeps 64 rows under
a cap of 0.10.  So the start states are drawn at 30 x N(0, 1) and the codes at 64 x 0.7 N(0, 1) (nominals: 64 x 0.5 N(0, 1)):
a first layer that reads the code, or an unbounded hidden layer behind it, then keeps pre-activations of size one and more
at every step, and the share falls to 0.2 - 5 % (measured on 4000 rows per model).  Under the sphere the code is a unit vector
whatever its scale, so only the start states are scaled.  Scaled errors do not depend on the data's scale; Adam's step is lr
per element, so a configuration's learning rate follows its codes' scale (lr_of).

Bounds (infer_cases.py; `scaled` = max_err_scaled):
  cost    FORWARD_BOUND, relative, against the float64 cost of the SAME states
  stage   GRAD_BOUND: dz_t and ds_t of every step against `rollout_step_vjp_torch` in float64 at the same s_t, with the
          cotangent built from the same s_{t+1} and the same ds_{t+1} (teacher-forced: one step's error, not the chain's)
  chain   dz and ds against float64 backpropagation through time from s0.  Not fixed in advance: tests/test_refine_cpu.py
          measures the float32 twin of the rule (never the device code) over all configurations, the largest figure stands in
          CHAIN_TWIN_OBSERVED, and CHAIN_BOUND is four times that, capped at 1e-3 (as imagine_cases.GOLDEN_BOUND is formed).
          The gradient `refine` exposes is held to the same bound
  update  FORWARD_BOUND: z_iters[i + 1] against one float64 Adam step (+ projection) from z_iters[i] and the gradients the
          same calls returned
  a0, s1  ROLLOUT_BOUND against one float64 step on plan_z[0]
A configuration whose float32 twin does not stay within a quarter of the fixed bounds is reseeded (RESEED), never loosened.

LR (times the codes' scale): chosen on the CPU so that the float64 rule descends -- iter_cost[3].sum() < iter_cost[0].sum() -- in every refinement
configuration of three steps whose decoder reads the code; tests/test_refine_cpu.py asserts it."""
import functools
import types

import torch

import imagine_cases as IC
import infer_cases as I
from physicsvae_amd import refine as RF
from physicsvae_amd.imagine import _ACTS, NET_KEYS, _window, step_torch
from ppo_cases import KINK
from vae_ppo_cases import scaled

ROLLOUT_BOUND, FORWARD_BOUND, GRAD_BOUND = I.ROLLOUT_BOUND, I.FORWARD_BOUND, I.GRAD_BOUND
MODELS = IC.CASE_IDS
SHAPES = ((1, 1), (5, 1), (3, 11), (64, 1))
HORIZONS = (1, 3)
REFINE_ENVS, REFINE_STEPS = (1, 5, 33), (0, 1, 3)
LR = 0.05                       # at codes of size one; a configuration's own: lr_of (Adam's step is lr per element, so lr follows the codes' scale)
# (start-state scale, code scale) of a model's data: see the module docstring, "ReLU kinks"
SCALES = {name: (30.0, 64.0) for name in IC.CASE_IDS}
SCALES["sphere"] = (30.0, 1.0)
CHAIN_TWIN_OBSERVED = 1.5e-5    # the float32 twin's largest chain / grad figure (tests/test_refine_cpu.py::test_chain_twin_observed)
CHAIN_BOUND = min(4 * CHAIN_TWIN_OBSERVED, 1e-3)
# configuration id -> seeds further: the first seed's pool was over its drop cap (0.154, 0.111, 0.167, 0.286; found with
# tests/test_refine_cpu.py's measures; that file holds len(RESEED) to one configuration in eight)
RESEED = {"zero_mean-3x11-H1-w": 1, "zero_mean-64x1-H3": 1, "state_mean-E5-s1-H3-w": 1, "body_task-E5-s1-H3-w": 1}
BOUNDS = {"cost": FORWARD_BOUND, "stage": GRAD_BOUND, "chain": CHAIN_BOUND, "update": FORWARD_BOUND, "grad": CHAIN_BOUND,
          "a0": ROLLOUT_BOUND, "s1": ROLLOUT_BOUND}
FIXED = ("cost", "stage", "update", "a0", "s1")


def _grad_configs():
    out = []
    for m, name in enumerate(MODELS):
        for j, (E, G) in enumerate(SHAPES):
            c = types.SimpleNamespace(model=name, E=E, G=G, H=HORIZONS[(j + m) % 2], weights=(j + m // 2) % 2 == 0)
            c.id = "%s-%dx%d-H%d%s" % (name, E, G, c.H, "-w" if c.weights else "")
            out.append(c)
    return out


def _refine_configs():
    out = []
    for m, name in enumerate(MODELS):
        for j, E in enumerate(REFINE_ENVS):
            for k, steps in enumerate(REFINE_STEPS):
                c = types.SimpleNamespace(model=name, E=E, steps=steps, H=HORIZONS[(j + k + m) % 2], weights=(j + k + m // 2) % 2 == 0)
                c.id = "%s-E%d-s%d-H%d%s" % (name, E, steps, c.H, "-w" if c.weights else "")
                out.append(c)
    return out


GRAD_CONFIGS, REFINE_CONFIGS = _grad_configs(), _refine_configs()
GRAD_IDS, REFINE_IDS = tuple(c.id for c in GRAD_CONFIGS), tuple(c.id for c in REFINE_CONFIGS)
BY_ID = {c.id: c for c in GRAD_CONFIGS + REFINE_CONFIGS}


def lr_of(model):
    return LR * SCALES[model][1]


def reads_code(m):
    return tuple(m.md_inputs) != tuple(I.BODY)


def sd64(m):
    return {k: v.double() for k, v in m.sd.items()}


def _stack_margin(sd, net, acts, x):
    """Smallest |pre-activation| per row over the ReLU layers of one stack on its windowed input x (inf: no ReLU layer)."""
    margin = torch.full((x.shape[0],), float("inf"), dtype=x.dtype)
    for i, a in enumerate(acts):
        x = x @ sd["%s._model.%d._model.0.weight" % (net, i)].t() + sd["%s._model.%d._model.0.bias" % (net, i)]
        if a == "relu":
            margin = torch.minimum(margin, x.abs().min(dim=1).values)
        x = _ACTS[a](x)
    return margin


def step_margin(m, sd, s, z):
    """Per row: the ReLU margin of one step of the rule from (s, z) over the decoder, the helper and the world model."""
    A = m.A
    x = torch.cat([s, z], 1)
    lo, hi = _window(A.md_inputs, A.Db, A.Db + A.Z)
    margin = _stack_margin(sd, NET_KEYS["md"], A.md.acts, x[:, lo:hi])
    if A.mh is not None:
        margin = torch.minimum(margin, _stack_margin(sd, NET_KEYS["mh"], A.mh.acts, x[:, lo:hi]))
    a, _, _ = step_torch(A, sd, "prior", s, z=z)
    return torch.minimum(margin, _stack_margin(sd, NET_KEYS["wm"], A.wm.acts, torch.cat([s, a], 1)))


def rollout_margin(m, s0_rows, z):
    """Per row: the ReLU margin over every step of the float64 unroll of the codes z [H, rows, Z] from s0_rows."""
    sd = sd64(m)
    s, margin = s0_rows.double(), None
    with torch.no_grad():
        for t in range(z.shape[0]):
            mt = step_margin(m, sd, s, z[t].double())
            margin = mt if margin is None else torch.minimum(margin, mt)
            _, _, s = step_torch(m.A, sd, "prior", s, z=z[t].double())
    return margin


def _weights(c, m, g):
    c.cw = c.sw = None
    if c.weights:
        c.cw, c.sw = torch.rand(m.Db, generator=g) + 0.25, torch.rand(c.H, generator=g) + 0.25
        if m.Db > 1:                # (db1 has one column: its weight stays positive)
            c.cw[m.Db // 2] = 0.0


def _first(keep, need, what):
    sel = torch.nonzero(keep)[:need, 0]
    assert sel.numel() == need, (what, "too few candidates off the ReLU kinks", int(keep.sum()), need)
    drawn = int(sel[-1]) + 1                                  # candidates looked at until `need` were found
    return sel, 1.0 - need / drawn


@functools.lru_cache(maxsize=None)
def grad_case(cid):
    """The configuration with its data: the model, s0 [E, Db], targets [H, E, Db], z [H, E * G, Z], cw / sw (None without
    weights), `dropped`.  Built once, left unchanged."""
    cfg = BY_ID[cid]
    m = IC.case(cfg.model)
    c = types.SimpleNamespace(**vars(cfg))
    c.m, c.rows = m, cfg.E * cfg.G
    g = torch.Generator().manual_seed(8800 + 10 * GRAD_IDS.index(cid) + RESEED.get(cid, 0))
    rn = lambda *shape: torch.randn(*shape, generator=g)                              # noqa: E731
    nE, nG = 3 * c.E + 16, (3 * c.G + 16 if c.G > 1 else 1)
    ss, zs = SCALES[cfg.model]
    s0, targets, z = ss * rn(nE, m.Db), rn(c.H, nE, m.Db), zs * 0.7 * rn(c.H, nE, nG, m.Z)
    _weights(c, m, g)
    margin = rollout_margin(m, s0.repeat_interleave(nG, dim=0), z.reshape(c.H, nE * nG, m.Z)).reshape(nE, nG)
    if c.G == 1:
        env, c.dropped = _first(margin[:, 0] >= KINK, c.E, cid)
        z = z[:, env, 0]
    else:                                                     # per environment the first G codes off the kinks
        ok = (margin >= KINK).sum(dim=1) >= c.G
        env, _ = _first(ok, c.E, cid)
        picks, shares = zip(*[_first(margin[e] >= KINK, c.G, cid) for e in env.tolist()])
        z = torch.stack([z[:, e, p] for e, p in zip(env.tolist(), picks)], dim=1).reshape(c.H, c.rows, m.Z)
        c.dropped = max(shares)
    c.s0, c.targets, c.z = s0[env].contiguous(), targets[:, env].contiguous(), z.contiguous()
    return c


def refine64(c, steps=None, dtype=torch.float64, s0=None, targets=None, nominal=None):
    t = lambda x: None if x is None else x.to(dtype)                                  # noqa: E731
    return RF.refine_torch(c.m.A, c.m.sd, t(c.s0 if s0 is None else s0), t(c.targets if targets is None else targets), c.H,
                           c.steps if steps is None else steps, c.lr, nominal=t(c.nominal if nominal is None else nominal),
                           col_weight=t(c.cw), step_weight=t(c.sw))


@functools.lru_cache(maxsize=None)
def refine_case(cid):
    """The configuration with its data: the model, s0 [E, Db], targets [H, E, Db], nominal [H, E, Z], cw / sw, `dropped`."""
    cfg = BY_ID[cid]
    m = IC.case(cfg.model)
    c = types.SimpleNamespace(**vars(cfg))
    c.m = m
    g = torch.Generator().manual_seed(9900 + 10 * REFINE_IDS.index(cid) + RESEED.get(cid, 0))
    rn = lambda *shape: torch.randn(*shape, generator=g)                              # noqa: E731
    nE = 3 * c.E + 16
    ss, zs = SCALES[cfg.model]
    c.lr = lr_of(cfg.model)
    s0, targets, nominal = ss * rn(nE, m.Db), rn(c.H, nE, m.Db), zs * 0.5 * rn(c.H, nE, m.Z)
    _weights(c, m, g)
    margin = torch.full((nE,), float("inf"), dtype=torch.float64)
    if c.steps > 0:                 # the one unroll whose gradient is compared with float64: the last backward's
        margin = rollout_margin(m, s0, refine64(c, s0=s0, targets=targets, nominal=nominal)["z_iters"][c.steps - 1])
    env, c.dropped = _first(margin >= KINK, c.E, cid)
    c.s0, c.targets, c.nominal = s0[env].contiguous(), targets[:, env].contiguous(), nominal[:, env].contiguous()
    return c


def drop_cap(rows):
    return I.DROP_CAP if rows >= 5 else I.DROP_CAP_FEW_ROWS


# ---------------------------------------------------------------------------------------
# the measures of the module docstring, on one call's results (float32: the float32 twin's, or the device's)
# ---------------------------------------------------------------------------------------
def grad_errors(c, got, ref=None):
    """`got`: {"cost", "dz", "ds", "states"} of one gradient call on the configuration.  {measure: error}."""
    m, d = c.m, lambda x: x.double()                                                  # noqa: E731
    sd = sd64(m)
    e = {}
    j64 = RF.rollout_cost_torch(d(got["states"]), d(c.targets), c.G, c.cw, c.sw)
    e["cost"] = float(((d(got["cost"]) - j64).abs() / j64).max())
    coef = RF.cost_coef(m.Db, c.H, torch.float64, c.cw, c.sw)
    tg = d(c.targets).repeat_interleave(c.G, dim=1)
    s0_rows = d(c.s0).repeat_interleave(c.G, dim=0)
    e["stage"] = 0.0
    for t in range(c.H):
        cot = coef[t] * (d(got["states"][t]) - tg[t]) + (d(got["ds"][t + 1]) if t + 1 < c.H else 0.0)
        dz, ds, _ = RF.rollout_step_vjp_torch(m.A, sd, d(got["states"][t - 1]) if t > 0 else s0_rows, d(c.z[t]), cot)
        e["stage"] = max(e["stage"], scaled(got["dz"][t], dz), scaled(got["ds"][t], ds))
    ref = grad64(c) if ref is None else ref
    e["chain"] = max(scaled(got["dz"], ref["dz"]), scaled(got["ds"], ref["ds"]))
    return e


def grad64(c, dtype=torch.float64):
    t = lambda x: None if x is None else x.to(dtype)                                  # noqa: E731
    return RF.rollout_grad_torch(c.m.A, c.m.sd, t(c.s0), t(c.z), t(c.targets), c.G, t(c.cw), t(c.sw))


def grad_twin32_errors(cid):
    c = grad_case(cid)
    return grad_errors(c, grad64(c, torch.float32))


def adam64(v, m, w, g, k, lr):
    """One Adam step of the rule in float64 with exact scalars."""
    m = RF.BETA1 * m + (1.0 - RF.BETA1) * g
    w = RF.BETA2 * w + (1.0 - RF.BETA2) * g * g
    v = v - lr / (1.0 - RF.BETA1 ** k) * (m / (w.sqrt() / (1.0 - RF.BETA2 ** k) ** 0.5 + RF.ADAM_EPS))
    return v, m, w


def refine_errors(c, run):
    """`run(steps)`: the results of one refinement call of that many steps on the configuration, with "z_iters" and "grad"
    (a call of fewer steps exposes an earlier iteration's gradient).  {measure: error}."""
    m, d = c.m, lambda x: x.double()                                                  # noqa: E731
    sd = sd64(m)
    got = run(c.steps)
    e = {"update": 0.0, "grad": 0.0}
    sphere = m.A.prior == RF.SPHERE
    v, mo, w = d(c.nominal), torch.zeros_like(d(c.nominal)), torch.zeros_like(d(c.nominal))
    e["update"] = scaled(got["z_iters"][0], RF.project_torch(m.A.prior, v))
    for i in range(c.steps):
        g = got["grad"] if i + 1 == c.steps else run(i + 1)["grad"]
        if not sphere:
            v = d(got["z_iters"][i])                          # (the iterate is the code: the device's own)
        if i + 1 == c.steps:                                  # the exposed gradient against float64 from the same iterate
            r = RF.rollout_grad_torch(m.A, sd, d(c.s0), d(got["z_iters"][i]), d(c.targets), 1, c.cw, c.sw)
            e["grad"] = scaled(g, RF.pullback_torch(m.A.prior, v, r["dz"]))
        v, mo, w = adam64(v, mo, w, d(g), i + 1, c.lr)
        e["update"] = max(e["update"], scaled(got["z_iters"][i + 1], RF.project_torch(m.A.prior, v)))
    a64, _, s64 = step_torch(m.A, sd, "prior", d(c.s0), z=d(got["plan_z"][0]))
    e["a0"], e["s1"] = scaled(got["a0"], a64), scaled(got["s1"], s64)
    return e


def refine_twin32_errors(cid):
    c = refine_case(cid)
    return refine_errors(c, lambda steps: refine64(c, steps=steps, dtype=torch.float32))
