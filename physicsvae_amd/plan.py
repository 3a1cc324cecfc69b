"""Planning in the latent space: sampled candidate codes over imagined rollouts -- the rule, in torch.

`plan_torch` is the specification of `pvae_plan` (include/pvae.h; `HipEngine.plan`, `PhysicsVAE.plan`,
`TrainModel.evaluate_plan`) and the oracle of its tests.  It computes in the dtype of its inputs and calls nothing of the
library.  The rule is this project's own: the reference has no planner.  It is random shooting (lam == 0) or MPPI (lam > 0)
over the codes the motor decoder reads, with the world model as the simulator.

A call takes E environments, K >= 1 candidates per environment (rows = E * K, row r = e * K + k, environment-major), a
horizon H >= 1, `iters` >= 1, a nominal code sequence u [H, E, Z] (zeros when absent), targets [H, E, Db] and start states
s0 [E, Db]; row r reads the targets and the start state of environment r // K.

For iteration i = 0 .. iters - 1:

1. Candidates.  v(t, r) = u(t, e) + sigma * n_i(t, r), one float product and one float sum.  Candidate k = 0 is the nominal
   itself: its noise is 0, is not drawn, and the written noise is 0.0.  n is supplied (`noise` [iters, H, rows, Z]) or, on
   the device, drawn from Philox at (seed, offset + i * H + t), Philox row row0 + r, in the latent groups below Z / 4 -- the
   domain the sampler and `imagine`'s prior mode use; `row0` lets a chunked caller number its rows globally, so that two
   chunks never draw the same noise.  z = v, except under `hypersphere_uniform`, where z = v / max(|v|, 1e-12) in the
   sampler's arithmetic (the decoder was trained on unit codes).  All four `latent_prior_type`s are accepted.  The learned
   prior's mean does NOT enter: candidates are centred on the nominal, whatever the prior kind.
2. Unroll.  `imagine`'s prior mode with z supplied on E * K rows for H steps: the decoder, the helper where the model has
   one, the world model; input subsets hold.
3. Cost.  J(r) = sum_t sw[t] * sum_c cw[c] * double(d)^2 / Db with d = s_{t+1}(r, c) - targets(t, e, c) formed in float32
   (in the inputs' dtype here: the `horizon_error` convention), squares and sums in double; cw [Db] and sw [H] are optional
   non-negative weights, ones when absent.  After step H - 1, J is rounded ONCE to float32 and stored in cost [E, K];
   selection reads those float32 values, so that a host that holds `cost` can reproduce every decision exactly.
4. Selection, per environment.  best(e) = the k of the smallest cost(e, k), ties to the lowest k.  With lam == 0:
   u'(t, e) = z(t, e * K + best) -- a copy (under the sphere already a unit code, not projected again).  With lam > 0:
   w_k = exp(-(cost_k - cost_best) / lam) in double, u'(t, e, j) = float32(sum_k w_k * double(z(t, r_k, j)) / sum_k w_k),
   summed over k in ascending order, and under the sphere projected again, u' / max(|u'|, 1e-12).  u <- u';
   iter_cost[i, e] = cost(e, best).

After the last iteration the plan's first step runs once more on E rows with z = u(0) -- an `imagine` prior-mode step of
horizon 1: a0 [E, Da], the decoder's mean (plus the helper) with no exploration noise and no clipping, and s1 [E, Db], the
world model's prediction for it.

Results: plan_z [H, E, Z] (the final u), best [E] int32, cost [E, K] float32, iter_cost [iters, E], a0, s1 and, from the
last iteration, z_cand [H, rows, Z], noise_out [H, rows, Z] (what was added, row k = 0 zero) and states [H, rows, Db].

With K == 1 nothing is drawn: the call is `imagine("prior", z = u)` followed by the one-step pass.  Shifting the returned
plan by one step for receding-horizon use is a slice on the host and not part of the rule.

Draws.  `plan_torch` cannot draw from Philox: the caller passes `noise` -- for a comparison with the device, `noise_out`.
"""
import torch

from .imagine import NET_KEYS, step_torch

SPHERE = "hypersphere_uniform"


def check_plan(envs, candidates, horizon, iters, sigma, lam, max_batch=None):
    """The refusals of the rule, by name: what `pvae_plan` answers with -1."""
    import math
    if envs < 1:
        raise ValueError("envs %d < 1" % envs)
    if candidates < 1:
        raise ValueError("candidates %d < 1" % candidates)
    if max_batch is not None and envs * candidates > max_batch:
        raise ValueError("rows %d = envs * candidates above max_batch %d" % (envs * candidates, max_batch))
    if horizon < 1:
        raise ValueError("horizon %d < 1" % horizon)
    if iters < 1:
        raise ValueError("iters %d < 1" % iters)
    if not (math.isfinite(sigma) and sigma >= 0):
        raise ValueError("sigma %r is negative or not finite" % (sigma,))
    if not (math.isfinite(lam) and lam >= 0):
        raise ValueError("lam %r is negative or not finite" % (lam,))


def plan_chunks(envs, candidates, max_batch):
    """[(first environment, one past the last, row0)] of a call over `envs` environments in chunks of floor(max_batch / K)
    environments; row0 = first environment * K numbers the rows globally."""
    if candidates > max_batch:
        raise ValueError("candidates %d above max_batch %d" % (candidates, max_batch))
    per = max_batch // candidates
    return [(lo, min(lo + per, envs), lo * candidates) for lo in range(0, envs, per)]


def _unit(v):
    return v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def plan_candidates_torch(prior, u, noise, sigma, candidates):
    """Step 1 for one iteration: u [H, E, Z], noise [H, E * K, Z] (None with K == 1) -> (z [H, E * K, Z], the noise as
    written: candidate 0's rows zero)."""
    H, E, Z = u.shape
    K = int(candidates)
    n = torch.zeros(H, E, K, Z, dtype=u.dtype) if noise is None else noise.to(u.dtype).reshape(H, E, K, Z).clone()
    n[:, :, 0] = 0
    v = u[:, :, None, :] + sigma * n
    v[:, :, 0] = u
    v = v.reshape(H, E * K, Z)
    return (_unit(v) if prior == SPHERE else v), n.reshape(H, E * K, Z)


def plan_cost_torch(states, targets, candidates, col_weight=None, step_weight=None):
    """Step 3: states [H, E * K, Db] against targets [H, E, Db] -> J [E, K] in double (the stored cost is J.float())."""
    H, rows, Db = states.shape
    d = (states - targets.to(states.dtype).repeat_interleave(int(candidates), dim=1)).double()
    q = d * d
    if col_weight is not None:
        q = q * col_weight.double()
    per_step = q.sum(dim=2) / Db
    if step_weight is not None:
        per_step = per_step * step_weight.double()[:, None]
    return per_step.sum(dim=0).reshape(rows // int(candidates), int(candidates))


def plan_best_torch(cost):
    """best [E] int32: the k of the smallest cost, ties to the lowest k."""
    K = cost.shape[1]
    k = torch.arange(K).expand_as(cost)
    return torch.where(cost == cost.min(dim=1, keepdim=True).values, k, torch.full_like(k, K)).min(dim=1).values.to(torch.int32)


def plan_weights_torch(cost, lam):
    """w [E, K] in double: exp(-(cost_k - cost_best) / lam)."""
    c = cost.double()
    return torch.exp(-(c - c.min(dim=1, keepdim=True).values) / float(lam))


def plan_select_torch(cost, z, lam, prior=None):
    """Step 4: cost [E, K] float32, z [H, E * K, Z] -> (u' [H, E, Z] in z's dtype, best [E] int32)."""
    E, K = cost.shape
    H, _, Z = z.shape
    best = plan_best_torch(cost)
    zz = z.reshape(H, E, K, Z)
    if lam == 0:
        return zz[:, torch.arange(E), best.long()], best
    w = plan_weights_torch(cost, lam)
    num, den = torch.zeros(H, E, Z, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)
    for k in range(K):                                       # (ascending k, as the device sums)
        num = num + w[None, :, k, None] * zz[:, :, k].double()
        den = den + w[:, k]
    u = (num / den[None, :, None]).to(z.dtype)
    return (_unit(u) if prior == SPHERE else u), best


def _weights_of(sd, device):
    return {k: v.detach().to(device) for k, v in sd.items() if k.split(".")[0] in NET_KEYS.values() and k.endswith(("weight", "bias"))}


def plan_unroll_torch(arch, sd, s0_rows, z, teacher=None):
    """Step 2: states [H, rows, Db] of `imagine`'s prior mode on the codes z [H, rows, Z] from s0_rows [rows, Db].  `teacher`
    (tests): step t starts from teacher[t - 1], the device's own states."""
    s, out = s0_rows, []
    for t in range(z.shape[0]):
        if teacher is not None and t > 0:
            s = teacher[t - 1].to(s0_rows.dtype)
        _, _, s = step_torch(arch, sd, "prior", s, z=z[t])
        out.append(s)
    return torch.stack(out)


def plan_torch(arch, sd, s0, targets, horizon, candidates, iters=1, sigma=1.0, lam=0.0, nominal=None, noise=None,
               col_weight=None, step_weight=None):
    """The rule on an `Arch` and a module's state dict.  s0 [E, Db], targets [H, E, Db], nominal [H, E, Z], noise [iters, H,
    E * K, Z] (needed when K > 1), col_weight [Db], step_weight [H], all in the dtype of s0.  Returns the dict of results
    named in the module docstring."""
    E, H, K = s0.shape[0], int(horizon), int(candidates)
    check_plan(E, K, H, int(iters), float(sigma), float(lam))
    if K > 1 and noise is None:
        raise ValueError("plan_torch cannot draw: pass noise")
    sd = _weights_of(sd, s0.device)
    u = torch.zeros(H, E, arch.Z, dtype=s0.dtype) if nominal is None else nominal.to(s0.dtype)
    s0_rows = s0.repeat_interleave(K, dim=0)
    iter_cost = []
    with torch.no_grad():
        for i in range(int(iters)):
            z, n = plan_candidates_torch(arch.prior, u, None if noise is None else noise[i], float(sigma), K)
            states = plan_unroll_torch(arch, sd, s0_rows, z)
            cost = plan_cost_torch(states, targets, K, col_weight, step_weight).float()
            u, best = plan_select_torch(cost, z, float(lam), arch.prior)
            iter_cost.append(cost[torch.arange(E), best.long()])
        a0, _, s1 = step_torch(arch, sd, "prior", s0, z=u[0])
    return {"plan_z": u, "best": best, "cost": cost, "iter_cost": torch.stack(iter_cost), "a0": a0, "s1": s1, "z_cand": z,
            "noise_out": n, "states": states}
