"""Gradient-refined latent plans: backpropagation through imagined rollouts -- the rule, in torch.

`rollout_grad_torch` is the specification of `pvae_imagine_grad` and `refine_torch` that of `pvae_plan_refine`
(include/pvae.h; `HipEngine.imagine_grad` / `.refine`, `PhysicsVAE.imagine_grad` / `.refine` / `.imagine_cost`,
`TrainModel.evaluate_plan(refine_steps=...)`), and both are the oracles of their tests.  They compute in the dtype of their
inputs and call nothing of the library.  The rule is this project's own: the reference has no planner.

Rollout cost and its gradient.  `imagine`'s prior mode with z supplied, the planner's setting, on rows = E * G rows
(`group` G >= 1, row r = e * G + g reads the start state and the targets of environment e = r // G, as `plan` does with K).
z [H, rows, Z] is the code as the decoder reads it; nothing is projected here.  The cost is `plan`'s step 3 exactly:
J(r) = sum_t sw[t] * sum_c cw[c] * double(d)^2 / Db with d = s_{t+1}(r, c) - targets(t, e, c) formed in float32 (here: the
inputs' dtype), squares and sums in double, J rounded ONCE to float32 into cost [rows].  dz [H, rows, Z] = dJ(r) / dz_t(r) and
ds [H, rows, Db] = dJ(r) / ds_t(r) (ds[0]: the gradient at the start state) come from full backpropagation through time
through the decoder (+ mh_range * tanh(helper)) and the world model, step by step from t = H - 1 down to 0:

    cot_{t+1}(r, c) = coef(t, c) * d(t, r, c) + ds_{t+1}(r, c)        one product and one sum in the inputs' dtype, ds_H = 0
    coef(t, c)      = float32(2 * sw[t] * cw[c] / Db)                  formed in double, rounded once
    (dz_t, ds_t)    = the vector-Jacobian product of one step (s_t, z_t) -> s_{t+1} with cot_{t+1}

ds_t sums, in this order, the world model's body columns, then the decoder's, then the helper's (the last two only where the
decoder reads the body).  A decoder that does not read the code (`md_inputs == ("body",)`) gets dz = +0.0 everywhere.  The
model's parameters get no gradient: every stack is frozen.

Refinement.  E environments, G = 1.  The iterate is v_i [H, E, Z], v_0 = nominal (zeros when absent).  The code fed to the
unroll is z_i = v_i, under `hypersphere_uniform` z_i = v_i / max(|v_i|, 1e-12).  For i = 0 .. steps - 1: forward and backward
at z_i give iter_cost[i] (float32) and g_i = dJ / dv -- dz itself, or under the sphere dz pulled back through the projection
(the sampler's backward): ie = 1 / max(|v|, 1e-12), g = (dz - v * ie * <v, dz> * ie) * ie -- then one Adam step on v, with
k = i + 1, beta1 = 0.9, beta2 = 0.999, eps = 1e-8, first and second moments zero at the start of EVERY call, in the inputs'
dtype, every operation rounded on its own (no fused multiply-add), in this order:

    m  = beta1 * m + float(1 - beta1) * g
    w  = beta2 * w + float(1 - beta2) * (g * g)
    v  = v - float(lr / (1 - beta1^k)) * (m / (sqrt(w) * float(1 / sqrt(1 - beta2^k)) + eps))

(the four scalars are formed in double and rounded once).  After the last update one forward-only unroll gives
iter_cost[steps].  best_iter [E] int32 = argmin over i of the STORED float32 costs, ties to the lowest i, so a host that holds
iter_cost reproduces it exactly; plan_z [H, E, Z] = z_{best_iter(e)}, a copy; cost [E] = iter_cost[best_iter], so a refined
plan is never worse than the plan it started from.  a0 [E, Da] and s1 [E, Db] come from the closing one-step pass on
z = plan_z[0], exactly as `plan`'s closing.  Optional: z_iters [steps + 1, H, E, Z] and grad [H, E, Z] (g of the last
backward; zeros with steps == 0).  steps == 0 is allowed: the call is then the cost of the nominal and the closing pass.
"""
import math

import torch

from .imagine import NET_KEYS, step_torch

SPHERE = "hypersphere_uniform"
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8


def check_refine(envs, horizon, steps, lr, max_batch=None, group=1):
    """The refusals of the rule, by name: what `pvae_plan_refine` (and, but for steps and lr, `pvae_imagine_grad`) answers
    with -1."""
    if envs < 1:
        raise ValueError("envs %d < 1" % envs)
    if group < 1:
        raise ValueError("group %d < 1" % group)
    if max_batch is not None and envs * group > max_batch:
        raise ValueError("rows %d = envs * group above max_batch %d" % (envs * group, max_batch))
    if horizon < 1:
        raise ValueError("horizon %d < 1" % horizon)
    if steps < 0:
        raise ValueError("steps %d < 0" % steps)
    if not (math.isfinite(lr) and lr > 0):
        raise ValueError("lr %r is not finite or not positive" % (lr,))


def refine_chunks(envs, group, max_batch):
    """[(first environment, one past the last)] of a call over `envs` environments in chunks of floor(max_batch / G)."""
    if group > max_batch:
        raise ValueError("group %d above max_batch %d" % (group, max_batch))
    per = max_batch // group
    return [(lo, min(lo + per, envs)) for lo in range(0, envs, per)]


def _weights_of(sd, device):
    return {k: v.detach().to(device) for k, v in sd.items() if k.split(".")[0] in NET_KEYS.values() and k.endswith(("weight", "bias"))}


def _unit(v):
    return v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def cost_coef(Db, horizon, dtype, col_weight=None, step_weight=None):
    """coef [H, Db] in `dtype`: 2 * sw[t] * cw[c] / Db formed in double, rounded once."""
    cw = torch.ones(Db, dtype=torch.float64) if col_weight is None else col_weight.double().cpu()
    sw = torch.ones(horizon, dtype=torch.float64) if step_weight is None else step_weight.double().cpu()
    return (2.0 * sw[:, None] * cw[None, :] / Db).to(dtype)


def rollout_step_vjp_torch(arch, sd, s, z, cot):
    """One step's vector-Jacobian product: from s_t [rows, Db], z_t [rows, Z] and the cotangent at s_{t+1} to (dz_t, ds_t, the
    s_{t+1} it recomputed).  dz_t is +0.0 where the decoder does not read the code."""
    s = s.detach().clone().requires_grad_(True)
    z = z.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        _, _, s1 = step_torch(arch, sd, "prior", s, z=z)
        dz, ds = torch.autograd.grad(s1, [z, s], cot.to(s1.dtype), allow_unused=True)
    dz = torch.zeros_like(z) if dz is None or tuple(arch.md_inputs) == ("body",) else dz
    return dz.detach(), (torch.zeros_like(s) if ds is None else ds).detach(), s1.detach()


def rollout_cost_torch(states, targets, group=1, col_weight=None, step_weight=None):
    """J [rows] in double of states [H, rows, Db] against targets [H, E, Db] (the stored cost is J.float())."""
    from .plan import plan_cost_torch
    return plan_cost_torch(states, targets, group, col_weight, step_weight).reshape(-1)


def rollout_grad_torch(arch, sd, s0, z, targets, group=1, col_weight=None, step_weight=None):
    """The rule on an `Arch` and a module's state dict: s0 [E, Db], z [H, E * G, Z], targets [H, E, Db], col_weight [Db],
    step_weight [H] in the dtype of s0.  Returns {"cost" [rows] float32, "dz" [H, rows, Z], "ds" [H, rows, Db], "states"
    [H, rows, Db]}."""
    H, rows, G = int(z.shape[0]), int(z.shape[1]), int(group)
    check_refine(s0.shape[0], H, 0, 1.0, group=G)
    if rows != s0.shape[0] * G:
        raise ValueError("z: %d rows, expected envs * group = %d" % (rows, s0.shape[0] * G))
    sd = _weights_of(sd, s0.device)
    dtype = s0.dtype
    tg = targets.to(dtype).repeat_interleave(G, dim=1)
    coef = cost_coef(arch.Db, H, dtype, col_weight, step_weight).to(s0.device)
    s, states = s0.repeat_interleave(G, dim=0), []
    with torch.no_grad():
        for t in range(H):
            _, _, s1 = step_torch(arch, sd, "prior", s, z=z[t])
            states.append(s1)
            s = s1
    states = torch.stack(states)
    cost = rollout_cost_torch(states, targets.to(dtype), G, col_weight, step_weight).float()
    dz, ds = [None] * H, [None] * H
    carry = torch.zeros(rows, arch.Db, dtype=dtype, device=s0.device)
    for t in range(H - 1, -1, -1):
        cot = coef[t] * (states[t] - tg[t]) + carry
        s_t = states[t - 1] if t > 0 else s0.repeat_interleave(G, dim=0)
        dz[t], ds[t], _ = rollout_step_vjp_torch(arch, sd, s_t, z[t], cot)
        carry = ds[t]
    return {"cost": cost, "dz": torch.stack(dz), "ds": torch.stack(ds), "states": states}


def project_torch(prior, v):
    """z of the iterate v: v itself, or the unit code under the sphere."""
    return _unit(v) if prior == SPHERE else v


def pullback_torch(prior, v, dz):
    """g = dJ / dv from dz = dJ / dz: dz itself, or the sampler's backward of the sphere projection."""
    if prior != SPHERE:
        return dz
    ie = 1.0 / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    zg = (v * dz).sum(dim=-1, keepdim=True) * ie
    return (dz - v * ie * zg) * ie


def adam_scalars(lr, k, dtype):
    """(float(1 - beta1), float(1 - beta2), float(lr / (1 - beta1^k)), float(1 / sqrt(1 - beta2^k))) rounded once to `dtype`."""
    r = lambda x: float(torch.tensor(x, dtype=torch.float64).to(dtype))                  # noqa: E731
    return r(1.0 - BETA1), r(1.0 - BETA2), r(lr / (1.0 - BETA1 ** k)), r(1.0 / math.sqrt(1.0 - BETA2 ** k))


def adam_step_torch(v, m, w, g, lr, k):
    """One Adam step of the rule on the iterate v with moments (m, w) and gradient g, step count k >= 1: (v', m', w')."""
    dtype = v.dtype
    r = lambda x: float(torch.tensor(x, dtype=torch.float64).to(dtype))                  # noqa: E731
    omb1, omb2, step, ibc2 = adam_scalars(lr, k, dtype)
    m = r(BETA1) * m + omb1 * g
    w = r(BETA2) * w + omb2 * (g * g)
    v = v - step * (m / (w.sqrt() * ibc2 + r(ADAM_EPS)))
    return v, m, w


def best_iter_torch(iter_cost):
    """best_iter [E] int32 of iter_cost [n, E]: the i of the smallest stored cost, ties to the lowest i."""
    n = iter_cost.shape[0]
    i = torch.arange(n, device=iter_cost.device)[:, None].expand_as(iter_cost)
    return torch.where(iter_cost == iter_cost.min(dim=0, keepdim=True).values, i, torch.full_like(i, n)).min(dim=0).values.to(torch.int32)


def refine_torch(arch, sd, s0, targets, horizon, steps, lr, nominal=None, col_weight=None, step_weight=None):
    """The refinement rule.  s0 [E, Db], targets [H, E, Db], nominal [H, E, Z].  Returns {"plan_z", "cost", "best_iter",
    "iter_cost", "a0", "s1", "z_iters", "grad"} as the module docstring names them."""
    E, H, steps = int(s0.shape[0]), int(horizon), int(steps)
    check_refine(E, H, steps, float(lr))
    sdw = _weights_of(sd, s0.device)
    dtype = s0.dtype
    v = torch.zeros(H, E, arch.Z, dtype=dtype, device=s0.device) if nominal is None else nominal.to(dtype).clone()
    m, w = torch.zeros_like(v), torch.zeros_like(v)
    g = torch.zeros_like(v)
    z_iters, iter_cost = [project_torch(arch.prior, v)], []
    for i in range(steps):
        out = rollout_grad_torch(arch, sdw, s0, z_iters[-1], targets, 1, col_weight, step_weight)
        iter_cost.append(out["cost"])
        g = pullback_torch(arch.prior, v, out["dz"])
        v, m, w = adam_step_torch(v, m, w, g, float(lr), i + 1)
        z_iters.append(project_torch(arch.prior, v))
    with torch.no_grad():
        s, states = s0, []
        for t in range(H):
            _, _, s = step_torch(arch, sdw, "prior", s, z=z_iters[-1][t])
            states.append(s)
        iter_cost.append(rollout_cost_torch(torch.stack(states), targets.to(dtype), 1, col_weight, step_weight).float())
        iter_cost = torch.stack(iter_cost)
        best = best_iter_torch(iter_cost)
        z_iters = torch.stack(z_iters)
        pick = torch.arange(E, device=s0.device)
        plan_z = z_iters[best.long(), :, pick].permute(1, 0, 2).contiguous()
        a0, _, s1 = step_torch(arch, sdw, "prior", s0, z=plan_z[0])
    return {"plan_z": plan_z, "cost": iter_cost[best.long(), pick], "best_iter": best, "iter_cost": iter_cost, "a0": a0, "s1": s1,
            "z_iters": z_iters, "grad": g}
