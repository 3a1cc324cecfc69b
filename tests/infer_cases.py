"""Cases of the sweep of the rollout and autograd entry points of physicsvae_amd/csrc/pvae_infer.hip
(tests/test_gpu_infer_shapes.py, checked without a GPU by tests/test_infer_cases_cpu.py): 32 random and 10 directed models --
stacks given layer by layer, the four latent priors, the nine input-subset pairs, the helper, widths past 1024 -- each with
its float64 twin, a pool of observation rows and draws, and one output cotangent per stack.  Everything is built on the CPU
from a seed, once (lru_cache), and left unchanged.

The twin is plain torch on the case's own float32 weights: nothing in it calls the library.  A case's SHAPE comes from its
seed and index or from its DIRECTED entry; its DATA (weights from oracle.refpath's normc initialiser with perturbed biases,
observations, draws, cotangents) from a seed of its own.

ReLU kinks.  Gradients are compared on rows whose smallest |pre-activation| over every ReLU layer of the encoder, the
decoder, the helper, the world model and the learned prior (at the inputs the tests hand those stacks) is at least
ppo_cases.KINK.  A pool draws a quarter more candidate rows than it needs and records the share it dropped; the caps are
those of vae_ppo_cases.py.  With normc weights (rows of norm 1) a ReLU pre-activation of a first layer on N(0, 1) inputs is
about N(0, 1): one unit drops a row with probability 2 KINK / sqrt(2 pi) = 8e-4, and the cap of 0.10 would leave room for
about 130 ReLU units on the gradient paths of one model.  Behind a bounded activation, or on a unit-norm code, the inputs are
two to three times smaller and the density at zero as much higher (a budget of 64 units put nine of the 42 cases over a
limit), so RELU_BUDGET holds a random case to 32 units: a drawn "relu" past the budget becomes the next non-ReLU
activation drawn, and every second layer that fits the budget is a ReLU layer whatever was drawn (the directed cases spend
64 units on a first layer, whose inputs are N(0, 1)).  KINK is a thousand
times the margin at which float32 and float64 can disagree about a ReLU; it is the margin the sweep was asked to keep, and
its price is that wide ReLU layers stay with the default-model tests.  The value branch carries no gradient and is exempt.

A case whose float32 twin does not stay within a quarter of every bound the GPU file asserts, one of whose compared gradient
tensors is all-zero in the float64 twin without the case making it so, or whose pool is over its drop cap, is replaced by
the next seed that passes: RESEED names it and `reseed_for` finds the seed.  A random case draws its dims and stacks again
(what cycles with the index stays); a directed case keeps its shape and draws new data.  The bounds never move, and the CPU
file holds the number of replaced cases to one in eight."""
import functools
import math
import types

import numpy as np
import torch

import fc_cases as F
from oracle import refpath as R
from ppo_cases import KINK
from vae_ppo_cases import BODY, BOTH, PAIRS, TASK, md_window, scaled, te_window           # noqa: F401

DBS = (1, 2, 13, 31, 32, 33, 70)
DAS = (1, 2, 5, 45, 64, 65)
ZS = (1, 2, 3, 8, 32, 33, 65)
WIDTHS = (5, 17, 31, 64, 100, 129, 200, 257, 320)
ACT_NAMES = ("relu", "tanh", "sigmoid", "elu", "linear")
ZERO_MEAN, STATE_MEAN, SPHERE = R.PRIORS
PRIOR_KINDS = (ZERO_MEAN, STATE_MEAN, SPHERE, False)
NOISE_MODES = ("eps", "philox", "off")
LOG_STD_TYPES = ("constant", "state_independent")
MAX_BATCHES = (32, 64, 128)
ROLLOUT_ROWS = (1, 2, 3, 4, 5, 31, 33)
AUTOGRAD_ROWS = (1, 3, 4, 5, 33, 64, 97)
N_RANDOM = 32
RELU_BUDGET = 32
DROP_CAP, DROP_CAP_FEW_ROWS = 0.10, 0.15                         # from 5 rows up / below
SAMPLE_STD = 0.1                                                 # the module's default: a constant log-std of log(0.1)
HELPER_GAIN = 60.0                                               # a helper term as large as the decoder's (tests/test_gpu_autograd.py)
# what the GPU file asserts: the project's standing bounds for these quantities (max_err_scaled)
ROLLOUT_BOUND = 2e-5          # a_hat, s2_hat, z of the rollout launches; eng.mlp_forward (test_gpu_rollout_module / _server)
VALUE_BOUND = 1e-4            # m.value_function() (test_rollout_and_value_branch_with_per_layer_stacks)
FORWARD_BOUND = 1e-5          # forward values of the autograd entry points (test_gpu_autograd.py); the policy's loss, relative
GRAD_BOUND = 1e-4             # dx, every parameter gradient, d_mu_logvar
NET_KEYS = {"te": "_task_encoder", "md": "_motor_decoder", "mh": "_motor_decoder_helper", "wm": "_world_model",
            "pr": "_latent_prior", "vb": "_value_branch"}
GRAD_NETS = ("te", "md", "mh", "wm", "pr")                       # the arena stacks: what carries a gradient here


# ---------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------
def chain(stack, layers, x):
    """One stack (widths, acts) holding `layers` [(W, b)] on x: (output of its linear last layer, smallest |pre-activation|
    over its ReLU layers per row)."""
    outs, margin = F.forward_graph([(stack[0], stack[1], layers[-1][0].shape[0])], [layers], x)
    return outs[0], margin


def te_out(c):
    return 2 * c.Z if c.prior in (ZERO_MEAN, STATE_MEAN) else c.Z


def nets_of(c):
    """The arena stacks the case has, in the order the tests visit them."""
    return tuple(k for k in GRAD_NETS if getattr(c, k) is not None)


def in_width(c, key):
    """Columns of the dense input the library reads for stack `key`: its full input width."""
    return {"te": 2 * c.Db, "md": c.Db + c.Z, "mh": c.Db + c.Z, "wm": c.Db + c.Da, "pr": c.Db, "vb": 2 * c.Db}[key]


def window(c, key):
    """Columns of that input the first layer of stack `key` reads."""
    if key == "te":
        return te_window(c)
    if key in ("md", "mh"):
        return md_window(c)
    return 0, in_width(c, key)


def out_width(c, key):
    return {"te": te_out(c), "md": c.Da, "mh": c.Da, "wm": c.Db, "pr": c.Z, "vb": 1}[key]


def run_stack(c, key, layers, x):
    """Stack `key` on its full-width input x: (output -- after the helper's tanh --, ReLU margin per row)."""
    lo, hi = window(c, key)
    out, margin = chain(getattr(c, key), layers, x[:, lo:hi])
    return (torch.tanh(out) if key == "mh" else out), margin


def sampler(c, h, eps, noise):
    """z of the encoder's output h (rmt:734-740, 795-816): N(mu, s^2) kinds z = mu + eps exp(logvar / 2), noise off z = mu;
    hypersphere z = e / max(|e|, 1e-12); no prior z = e."""
    if c.prior is False:
        return h
    if c.prior == SPHERE:
        return h / h.norm(dim=1, keepdim=True).clamp_min(1e-12)
    mu, lv = h[:, :c.Z], h[:, c.Z:]
    return mu + eps * torch.exp(lv / 2) if noise else mu


def sampler_backward(c, h, eps, noise, dz):
    """d h of `sampler` from dz, by hand (tests/test_infer_cases_cpu.py holds it against autograd)."""
    if c.prior is False:
        return dz.clone()
    if c.prior == SPHERE:
        n = h.norm(dim=1, keepdim=True).clamp_min(1e-12)
        z = h / n
        return (dz - z * (z * dz).sum(1, keepdim=True)) / n
    lv = h[:, c.Z:]
    return torch.cat([dz, dz * eps * 0.5 * torch.exp(lv / 2) if noise else torch.zeros_like(dz)], 1)


def forward(c, params, obs, eps, noise):
    """The model of case `c` on `params` {key: [(W, b)]} in their dtype: .h (the encoder's output), .z, .a (the action, helper
    term included), .s2 (the world model on [s_body | a]), .prior_mu (state-mean prior), .value, .margin (ReLU margin per row
    over the arena stacks)."""
    s_body = obs[:, :c.Db]
    h, margin = run_stack(c, "te", params["te"], obs)
    z = sampler(c, h, eps, noise)
    md_in = torch.cat([s_body, z], 1)
    a, m = run_stack(c, "md", params["md"], md_in)
    margin = torch.minimum(margin, m)
    if c.mh is not None:
        add, m = run_stack(c, "mh", params["mh"], md_in)
        a, margin = a + c.mh_range * add, torch.minimum(margin, m)
    s2, m = run_stack(c, "wm", params["wm"], torch.cat([s_body, a], 1))
    margin = torch.minimum(margin, m)
    prior_mu = None
    if c.pr is not None:
        prior_mu, m = run_stack(c, "pr", params["pr"], s_body)
        margin = torch.minimum(margin, m)
    value, _ = run_stack(c, "vb", params["vb"], obs)
    return types.SimpleNamespace(h=h, z=z, a=a, s2=s2, prior_mu=prior_mu, value=value.squeeze(1), margin=margin)


def leaves(c, dtype, grad=False):
    """The case's weights in `dtype` (as autograd leaves with `grad`)."""
    return {key: [(w.to(dtype).clone().requires_grad_(grad), b.to(dtype).clone().requires_grad_(grad)) for w, b in layers]
            for key, layers in c.params.items()}


def stack_twin(c, key, x, dy, dtype=torch.float64):
    """What `HipNet` computes for stack `key` on x [rows, full input width] and the cotangent dy: .out, .dx (inside the
    stack's window; the library's is exactly zero outside it), .grads [(dW, db)]."""
    layers = leaves(c, dtype, True)[key]
    lo, hi = window(c, key)
    xw = x[:, lo:hi].to(dtype).clone().requires_grad_(True)
    out, _ = chain(getattr(c, key), layers, xw)
    if key == "mh":
        out = torch.tanh(out)
    (out * dy.to(dtype)).sum().backward()
    return types.SimpleNamespace(out=out.detach(), dx=xw.grad, grads=[(w.grad, b.grad) for w, b in layers])


def policy_twin(c, obs, eps, noise, dtype=torch.float64, prior_term=True, weight=None):
    """The loss of the GPU file's policy test, (a^2).sum() + (s2^2).sum() [+ (prior_mu^2).sum()], rows weighted by `weight`
    (0 / 1: a row at a ReLU kink under draws only the GPU knows leaves the sum), and its gradients {key: [(dW, db)]} -- None
    where the loss does not reach a parameter."""
    params = leaves(c, dtype, True)
    out = forward(c, params, obs.to(dtype), None if eps is None else eps.to(dtype), noise)
    w = torch.ones(obs.shape[0], 1, dtype=dtype) if weight is None else weight.to(dtype).reshape(-1, 1)
    loss = (w * out.a ** 2).sum() + (w * out.s2 ** 2).sum()
    if prior_term and out.prior_mu is not None:
        loss = loss + (w * out.prior_mu ** 2).sum()
    flat = [t for key in nets_of(c) for pair in params[key] for t in pair]
    got = iter(torch.autograd.grad(loss, flat, allow_unused=True))
    grads = {key: [(next(got), next(got)) for _ in params[key]] for key in nets_of(c)}
    return types.SimpleNamespace(loss=loss.detach(), grads=grads, out=out)


# ---------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------
def spec(Db, Da, Z, te, md, wm, vb=((17,), ("relu",)), pr=None, mh=None, mh_range=0.5, prior=ZERO_MEAN, te_inputs=BOTH,
         md_inputs=BOTH, noise="eps", log_std_type="constant", max_batch=64, extra_rows=()):
    if prior == STATE_MEAN and pr is None:
        pr = te
    return types.SimpleNamespace(Db=Db, Da=Da, Z=Z, te=te, md=md, wm=wm, vb=vb, pr=pr if prior == STATE_MEAN else None, mh=mh,
                                 mh_range=mh_range, prior=prior, te_inputs=te_inputs, md_inputs=md_inputs, noise=noise,
                                 log_std_type=log_std_type, max_batch=max_batch, extra_rows=tuple(extra_rows))


@functools.lru_cache(maxsize=None)
def pair_order():
    """Subset pairs of the random cases: drawn without replacement in rounds of nine, so every pair comes up."""
    g = torch.Generator().manual_seed(5999)
    return tuple(int(v) for _ in range((N_RANDOM + 8) // 9) for v in torch.randperm(9, generator=g))


def draw_stack(g, budget):
    """1-4 hidden layers (widths, acts) and what is left of the case's ReLU budget."""
    ri = lambda n: int(torch.randint(n, (1,), generator=g))                          # noqa: E731
    widths, acts = [], []
    for _ in range(1 + ri(4)):
        w, a = WIDTHS[ri(len(WIDTHS))], ACT_NAMES[ri(len(ACT_NAMES))]
        if a == "relu" and w > budget:
            a = ACT_NAMES[1 + ri(len(ACT_NAMES) - 1)]
        elif w <= budget and ri(2) == 0:                         # (ReLU is what production runs: every second layer that fits)
            a = "relu"
        if a == "relu":
            budget -= w
        widths.append(w)
        acts.append(a)
    return (tuple(widths), tuple(acts)), budget


def random_spec(i, bump=0):
    """Shape of random case i (`bump`: of its replacement, see RESEED).  What must all come up cycles with the index (prior
    i % 4, noise mode i % 3, max_batch (i // 3) % 3, the log-std kind in the pattern c s s c, the subset pairs in shuffled
    rounds of nine); dims and stacks are drawn from the seed, the stack that spends the ReLU budget first rotating."""
    g = torch.Generator().manual_seed(6000 + i + 1000 * bump)
    ri = lambda n: int(torch.randint(n, (1,), generator=g))                          # noqa: E731
    Db, Da, Z = DBS[ri(len(DBS))], DAS[ri(len(DAS))], ZS[ri(len(ZS))]
    prior = PRIOR_KINDS[i % 4]
    keys = ["te", "md", "wm"] + (["pr"] if prior == STATE_MEAN else [])
    keys = keys[i % len(keys):] + keys[:i % len(keys)]
    stacks, budget = {}, RELU_BUDGET
    for key in keys:
        stacks[key], budget = draw_stack(g, budget)
    vb, _ = draw_stack(g, 10 ** 6)
    te_inputs, md_inputs = PAIRS[pair_order()[i]]
    return spec(Db, Da, Z, stacks["te"], stacks["md"], stacks["wm"], vb=vb, pr=stacks.get("pr"), prior=prior, te_inputs=te_inputs,
                md_inputs=md_inputs, noise=NOISE_MODES[i % 3], log_std_type=LOG_STD_TYPES[(i + i // 2) % 2],
                max_batch=MAX_BATCHES[(i // 3) % 3])


def helper_spec():
    """`helper`: R.with_helper's stack on a random-sized model -- the dims and stacks of the first random shape whose prior is
    the zero-mean one (the rollout server serves it) -- with the helper's 17 ReLU units inside the budget."""
    s = random_spec(0)
    assert s.prior == ZERO_MEAN and sum(w for st in (s.te, s.md, s.wm) for w, a in zip(*st) if a == "relu") + 17 <= 130
    return spec(s.Db, s.Da, s.Z, s.te, s.md, s.wm, vb=s.vb, mh=((17, "relu"), (33, "tanh")), noise="eps", max_batch=64)


T64, S64, E64 = ((64,), ("tanh",)), ((64,), ("sigmoid",)), ((64,), ("elu",))
R64 = ((64,), ("relu",))
DIRECTED = {
    # gemv_rollout_kernel `for (k = lane * 4 + 1024; k < K; ...)`: the second layer of every stack reads ld = 1088
    "wide_k": spec(13, 5, 8, ((1088, 64), ("tanh", "elu")), ((1088, 64), ("elu", "tanh")), ((1088, 64), ("sigmoid", "linear")),
                   max_batch=32),
    # the encoder's first layer reads ld = pad64(2 x 520) = 1088; Ka = 520 for input kinds 2 / 3
    "wide_obs": spec(520, 5, 8, R64, T64, E64, max_batch=32),
    "ones": spec(1, 1, 1, ((5,), ("relu",)), ((5,), ("tanh",)), ((5,), ("relu",)), max_batch=32),
    # sampler_bwd_kernel's `c += 64` lane loops: two passes and a bit; the norm loops of input kind 5
    "z130_zero_mean": spec(13, 5, 130, R64, T64, S64, prior=ZERO_MEAN, max_batch=64),
    "z130_hypersphere": spec(13, 5, 130, R64, T64, E64, prior=SPHERE, noise="philox", max_batch=64),
    "z130_none": spec(13, 5, 130, S64, T64, R64, prior=False, noise="off", max_batch=64),
    # the staged path of infer_impl at <= 4 rows; net_seed_kernel's act_grad on the helper's tanh at widths other than 16
    "helper": None,
    # 128 rows x 1024: the backward pairs on 32x32 tiles
    "pair32": spec(23, 7, 8, ((1024, 1024), ("tanh", "elu")), ((1024, 1024), ("elu", "sigmoid")), ((1024, 1024), ("sigmoid", "tanh")),
                   max_batch=128, noise="philox"),
    # EpiGradAccum on 32x32 weight-gradient tiles (64-row chunks), then a 3-row GEMV tail chunk
    "chunk64": spec(13, 5, 8, ((128, 192), ("tanh", "elu")), ((128, 192), ("elu", "sigmoid")), ((128, 192), ("sigmoid", "tanh")),
                    max_batch=64, extra_rows=(128, 131)),
    # EpiGradAccum on 64x64 tiles (32-row chunks); a 1-row last chunk
    "chunk32": spec(13, 5, 8, ((128, 192), ("elu", "tanh")), ((128, 192), ("tanh", "linear")), ((128, 192), ("linear", "sigmoid")),
                    max_batch=32, extra_rows=(33, 65, 97)),
}
DIRECTED["helper"] = helper_spec()
CASE_IDS = ["random%d" % i for i in range(N_RANDOM)] + list(DIRECTED)
# the rollout server's cases: directed shapes and three random ones whose priors it accepts (it refuses the hypersphere
# by design, see tests/test_gpu_infer_shapes.py)
SERVER_CASES = ("ones", "z130_zero_mean", "helper", "random4", "random1", "random3")
# cases that run on another seed than their first, because the first one did not pass `case_passes`: name -> how many seeds
# further (found with `reseed_for`; tests/test_infer_cases_cpu.py holds len(RESEED) to one case in eight)
# random19, 23: the pool over its drop cap (0.225, 0.32: a ReLU layer on a code of size 0.01 has pre-activations the size
# of its biases, 0.05); random6, 26: a hypersphere with Z = 1, whose code is +-1 and whose gradient through the sampler is
# exactly zero in float64 and rounding noise in float32
RESEED = {"random6": 1, "random19": 1, "random23": 1, "random26": 1}


def shape_of(name):
    return DIRECTED[name] if name in DIRECTED else random_spec(int(name[len("random"):]), RESEED.get(name, 0))


def rollout_rows(c):
    return tuple(sorted({min(r, c.max_batch) for r in ROLLOUT_ROWS}))


def autograd_rows(c):
    return tuple(sorted(set(AUTOGRAD_ROWS) | set(c.extra_rows)))


def relu_units(s):
    return sum(w for key in GRAD_NETS if getattr(s, key) is not None
               for w, a in (zip(*getattr(s, key)) if key != "mh" else s.mh) if a == "relu")


# ---------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------
def arch_of(s):
    """The case as oracle.refpath describes an architecture (what RefModel and the weight initialiser read)."""
    pairs = lambda st: [(w, a) for w, a in zip(*st)]                                 # noqa: E731
    arch = R.make_arch(s.Db, s.Da, latent=s.Z, te=pairs(s.te), md=pairs(s.md), wm=pairs(s.wm), vb=pairs(s.vb), prior=s.prior,
                       pr=pairs(s.pr) if s.pr is not None else None)
    arch = R.with_inputs(arch, s.te_inputs, s.md_inputs)
    return R.with_helper(arch, hidden=s.mh, rng=s.mh_range) if s.mh is not None else arch


def state_dict_of(s, seed):
    sd = R.perturb_biases(R.init_state_dict(arch_of(s), seed=seed), seed=seed + 2)
    if s.mh is not None:
        key = "_motor_decoder_helper._model.%d._model.0.weight" % len(s.mh)
        sd[key] = sd[key] * HELPER_GAIN
    return sd


def stack_inputs(c, obs, out):
    """The dense float32 input the tests hand each stack: the observation, [s_body | z] and [s_body | a] of the float64 twin
    rounded to float32, s_body."""
    s_body = obs[:, :c.Db]
    md_in = torch.cat([s_body, out.z.float()], 1)
    return {"te": obs, "md": md_in, "mh": md_in, "wm": torch.cat([s_body, out.a.float()], 1), "pr": s_body}


def build_case(name, s, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=g)                              # noqa: E731
    c = types.SimpleNamespace(**vars(s))
    c.name, c.seed = name, seed
    if isinstance(c.mh, tuple):                                   # the helper as a stack (widths, acts)
        c.mh_layers, c.mh = c.mh, (tuple(w for w, _ in s.mh), tuple(a for _, a in s.mh))
    c.arch = arch_of(s)
    c.sd = state_dict_of(s, seed)
    c.params = {key: [(c.sd["%s._model.%d._model.0.weight" % (net, i)], c.sd["%s._model.%d._model.0.bias" % (net, i)])
                      for i in range(len(getattr(c, key)[0]) + 1)] for key, net in NET_KEYS.items() if getattr(c, key) is not None}
    c.ls_vec = (torch.full((s.Da,), float(math.log(SAMPLE_STD)), dtype=torch.float32) if s.log_std_type == "constant"
                else -1.0 + 0.2 * rn(s.Da))
    need = max(autograd_rows(c))
    n = need + need // 4 + 8
    obs, eps = rn(n, 2 * s.Db), rn(n, s.Z)
    p64 = leaves(c, torch.float64)
    with torch.no_grad():
        out = forward(c, p64, obs.double(), eps.double(), s.noise != "off")
        margin = out.margin
        for key, x in stack_inputs(c, obs, out).items():          # the margins at the rounded inputs the stack tests use
            if key in c.params:
                margin = torch.minimum(margin, run_stack(c, key, p64[key], x.double())[1])
    keep = margin >= KINK
    c.dropped = 1.0 - float(keep.double().mean())
    sel = torch.nonzero(keep)[:need, 0]
    assert sel.numel() == need, (name, "too few rows off the ReLU kinks", int(keep.sum()), need)
    c.obs, c.eps = obs[sel].contiguous(), eps[sel].contiguous()
    c.dy = {key: rn(need, out_width(c, key)) for key in nets_of(c)}
    c.dz = rn(need, s.Z)
    return c


def first_seed(name):
    return 7000 + 100 * CASE_IDS.index(name)


@functools.lru_cache(maxsize=None)
def case(name):
    return build_case(name, shape_of(name), first_seed(name) + RESEED.get(name, 0))


def all_cases():
    return [case(name) for name in CASE_IDS]


@functools.lru_cache(maxsize=None)
def twin(name, rows, dtype=torch.float64):
    """The twin's forward of the first `rows` rows of the pool under the case's own draws (noise mode "off": z = mu), and the
    stack inputs derived from the FLOAT64 twin (the same tensors whatever `dtype`)."""
    c = case(name)
    with torch.no_grad():
        out64 = forward(c, leaves(c, torch.float64), c.obs[:rows].double(), c.eps[:rows].double(), c.noise != "off")
        out = out64 if dtype == torch.float64 else forward(c, leaves(c, dtype), c.obs[:rows].to(dtype), c.eps[:rows].to(dtype),
                                                            c.noise != "off")
    out.x = stack_inputs(c, c.obs[:rows], out64)
    return out


# ---------------------------------------------------------------------------------------
# what a case must pass (the float32 twin within a quarter of every bound; no accidental all-zero gradient; the drop cap)
# ---------------------------------------------------------------------------------------
QUARTER = {"rollout": ROLLOUT_BOUND / 4, "value": VALUE_BOUND / 4, "forward": FORWARD_BOUND / 4, "gradients": GRAD_BOUND / 4}


def structurally_zero(c, key):
    """The policy loss does not reach stack `key`: the encoder under a decoder that reads the body alone."""
    return key == "te" and c.md_inputs == BODY


def twin32_errors(name):
    """The float32 twin against the float64 twin by the GPU file's measures, over every row count the GPU file runs:
    ({quantity: largest error}, [compared gradient tensors that are all-zero in the float64 twin by accident])."""
    c = case(name)
    e = dict.fromkeys(QUARTER, 0.0)
    zeros = []
    up = lambda key, v: e.__setitem__(key, max(e[key], v))                          # noqa: E731
    noise = c.noise != "off"
    for rows in rollout_rows(c):
        a, b = twin(name, rows, torch.float32), twin(name, rows)
        for q in ("a", "s2", "z"):
            up("rollout", scaled(getattr(a, q), getattr(b, q)))
        up("value", scaled(a.value, b.value))
    for rows in autograd_rows(c):
        x = twin(name, rows).x
        for key in nets_of(c):
            a, b = stack_twin(c, key, x[key], c.dy[key][:rows], torch.float32), stack_twin(c, key, x[key], c.dy[key][:rows])
            up("forward", scaled(a.out, b.out))
            up("gradients", scaled(a.dx, b.dx))
            for i, (pa, pb) in enumerate(zip(a.grads, b.grads)):
                for j, (ga, gb) in enumerate(zip(pa, pb)):
                    up("gradients", scaled(ga, gb))
                    if float(gb.abs().max()) == 0.0:
                        zeros.append((rows, key, i, j))
        if rows <= c.max_batch:
            h = twin(name, rows).h
            for on in (True, False):
                z32, z64 = sampler(c, h.float(), c.eps[:rows], on), sampler(c, h, c.eps[:rows].double(), on)
                up("forward", scaled(z32, z64))
                up("gradients", scaled(sampler_backward(c, h.float(), c.eps[:rows], on, c.dz[:rows]),
                                       sampler_backward(c, h, c.eps[:rows].double(), on, c.dz[:rows].double())))
        a, b = policy_twin(c, c.obs[:rows], c.eps[:rows], noise, torch.float32), policy_twin(c, c.obs[:rows], c.eps[:rows], noise)
        up("forward", abs(float(a.loss) - float(b.loss)) / abs(float(b.loss)))
        for key in nets_of(c):
            for i, (pa, pb) in enumerate(zip(a.grads[key], b.grads[key])):
                for j, (ga, gb) in enumerate(zip(pa, pb)):
                    if gb is None:
                        assert ga is None and structurally_zero(c, key), (name, key, i, j)
                        continue
                    up("gradients", scaled(ga, gb))
                    if float(gb.abs().max()) == 0.0 and not structurally_zero(c, key):
                        zeros.append((rows, "policy " + key, i, j))
    return e, zeros


def drop_cap(c):
    return DROP_CAP if max(autograd_rows(c)) >= 5 else DROP_CAP_FEW_ROWS


def case_passes(name):
    e, zeros = twin32_errors(name)
    return all(e[key] <= QUARTER[key] for key in QUARTER) and not zeros and case(name).dropped <= drop_cap(case(name))


def reseed_for(name, limit=20):
    """The entry RESEED needs for `name` (0: none): the first seed at which `case_passes`."""
    for bump in range(limit):
        saved = RESEED.get(name)
        RESEED[name] = bump
        case.cache_clear()
        twin.cache_clear()
        try:
            ok = case_passes(name)
        except AssertionError:
            ok = False
        finally:
            if saved is None:
                RESEED.pop(name, None)
            else:
                RESEED[name] = saved
            case.cache_clear()
            twin.cache_clear()
        if ok:
            return bump
    raise AssertionError("no seed under %d for %s" % (limit, name))


# ---------------------------------------------------------------------------------------
# the module of a case
# ---------------------------------------------------------------------------------------
def module_for(c, device, max_batch=None):
    """`PhysicsVAE` as the case configures it, holding the case's weights and log-std vector."""
    from physicsvae_amd.model import PhysicsVAE
    from physicsvae_amd.spaces import Box
    box = lambda n: Box(np.zeros(n), np.zeros(n))                                   # noqa: E731
    arch = c.arch
    cmc = dict(observation_space=box(2 * c.Db), observation_space_body=box(c.Db), observation_space_task=box(c.Db),
               action_space=box(c.Da), task_encoder_layers=R.fc_layer_list(arch["te"]), motor_decoder_layers=R.fc_layer_list(arch["md"]),
               world_model_layers=R.fc_layer_list(arch["wm"]), value_fn_layers=R.fc_layer_list(arch["vb"]),
               task_encoder_output_dim=c.Z, latent_prior_type=c.prior, device=device, max_batch=max_batch or c.max_batch,
               log_std_type=c.log_std_type, sample_std=SAMPLE_STD, task_encoder_inputs=list(c.te_inputs),
               motor_decoder_inputs=list(c.md_inputs))
    if c.prior == STATE_MEAN:
        cmc["latent_prior_layers"] = R.fc_layer_list(arch["pr"])
    if c.mh is not None:
        layers = R.fc_layer_list(arch["mh"])
        layers[-1]["activation"] = "tanh"
        cmc.update(motor_decoder_helper_enable=True, motor_decoder_helper_layers=layers, motor_decoder_helper_range=c.mh_range)
    m = PhysicsVAE(cmc["observation_space"], cmc["action_space"], 2 * c.Da, {"custom_model_config": cmc}, "physics_vae")
    sd = {k: v.clone() for k, v in c.sd.items()}
    if c.log_std_type == "state_independent":
        sd["_motor_decoder._model.%d.log_std" % (len(c.md[0]) + 1)] = c.ls_vec.clone()
    m.load_state_dict(sd)
    m.latent_prior_noise = c.noise != "off"
    return m
