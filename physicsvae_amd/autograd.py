"""Torch autograd through the arena stacks: what PPO's `loss.backward()` does to `PhysicsVAE.forward` (rmt:743-771) and the
stage functions (rmt:773-853) when the task encoder / motor decoder are learnable (rmt:473, 488), on the HIP kernels.

The arena stacks (TE, MD, WM, PR, MH) are views into the engine's flat parameter arena and their forward is a library call,
so torch cannot differentiate it by itself.  The Functions below give those calls a backward built from
`pvae_net_backward` (recompute the stack's forward, then the trainer's per-layer backward plan) and `pvae_reparam_backward`.
Their forwards are the very calls the module makes without autograd, so values are the same bits either way.

  HipNet      one stack: (x, *parameter views of the stack) -> output
  HipReparam  the sampler: mu_logvar -> z, with the draws the forward used kept for the backward
  HipPolicy   `forward()` as ONE `pvae_infer_logits` call: (obs, *TE, *MD, *MH, *WM) -> (a_hat, z, mu_logvar, s2)
  HipStackSet a stack set (`pvae_fc_*`, FullyConnectedPolicy): (x, *params of all stacks) -> (out_0, ..., out_{S-1})
  HipImagineCost  the cost of an imagined rollout (`pvae_imagine_grad`): (s0, z) -> cost, the stacks frozen

Every backward runs in chunks of at most `max_batch` rows, the parameter gradient summed over the chunks into one flat
buffer per stack (accumulate = 1 after the first chunk) and handed back as views shaped like the parameters.  The
parameter views, the inputs and the outputs a backward reads are saved with `save_for_backward`, never kept as ctx
attributes: an output held by its own ctx is a reference cycle through the graph that the garbage collector cannot
break.  An in-place write between forward and backward -- an optimizer step, `load_state_dict`, a caller recycling its
observation buffer -- then raises torch's usual error instead of returning gradients taken at other values.  Double
backward is not offered (`once_differentiable`).
"""
import sys

import torch
from torch.autograd.function import once_differentiable

from ._lib import NET_MD, NET_MH, NET_TE, NET_WM


def chunks(rows, max_batch):
    """[(lo, hi)] spans of at most `max_batch` rows covering [0, rows)."""
    return [(lo, min(lo + max_batch, rows)) for lo in range(0, rows, max_batch)]


def stack_params(fc):
    """The weight / bias views of one FC stack in layer order (AppendLogStd is not part of the arena)."""
    out = []
    for m in fc._model:
        lin = getattr(m, "_model", None)
        if isinstance(lin, torch.nn.Sequential) and isinstance(lin[0], torch.nn.Linear):
            out += [lin[0].weight, lin[0].bias]
    return out


def grad_views(eng, net, gbuf):
    """`gbuf` (a flat gradient of stack `net`'s arena segment) as views shaped like the stack's parameters, in the order
    of `stack_params`: W[:n_out, col0:col0 + n_in] of every padded block, then its bias."""
    off0 = eng.segments[net][0]
    out = []
    for info in eng.layers:
        if info["net"] != net:
            continue
        w0, b0 = info["w_offset"] - off0, info["b_offset"] - off0
        blk = gbuf[w0: w0 + info["n_out_pad"] * info["ld"]].view(info["n_out_pad"], info["ld"])
        out.append(blk[: info["n_out"], info["col0"]: info["col0"] + info["n_in"]])
        out.append(gbuf[b0: b0 + info["n_out"]])
    return out


def net_forward(eng, net, x):
    """`engine.net_forward` over any number of rows (chunks of at most `max_batch`)."""
    x = x.reshape(x.shape[0], -1)
    if x.shape[0] <= eng.max_batch:
        return eng.net_forward(net, x)
    return torch.cat([eng.net_forward(net, x[lo:hi]) for lo, hi in chunks(x.shape[0], eng.max_batch)])


def net_backward(eng, net, x, dy, want_dx, want_grad):
    """(dx | None, flat parameter gradient of the stack | None) over any number of rows."""
    gbuf = torch.empty(eng.segments[net][1], dtype=torch.float32, device=eng.device) if want_grad else None
    if not (want_dx or want_grad):
        return None, None
    dxs = [eng.net_backward(net, x[lo:hi], dy[lo:hi], want_dx, gbuf, accumulate=i > 0)
           for i, (lo, hi) in enumerate(chunks(x.shape[0], eng.max_batch))]
    dx = (dxs[0] if len(dxs) == 1 else torch.cat(dxs)) if want_dx else None
    return dx, gbuf


def _param_grads(eng, net, gbuf, needs):
    if gbuf is None:
        return [None] * len(needs)
    return [g if n else None for g, n in zip(grad_views(eng, net, gbuf), needs)]


class HipNet(torch.autograd.Function):
    """One arena stack: `HipNet.apply(engine, net, x, *stack_params(fc))` -> output [rows, n_out] (after the output
    activation: the helper's tanh).  Forward = `engine.net_forward` (chunked); backward = `engine.net_backward` with
    grad = None when no parameter of the stack wants a gradient (frozen stack: input gradient only) and dx = None when
    `x` does not."""

    @staticmethod
    def forward(ctx, eng, net, x, *params):
        ctx.eng, ctx.net, ctx.x_shape, ctx.x_dtype = eng, net, x.shape, x.dtype
        ctx.save_for_backward(x, *params)
        return net_forward(eng, net, _dense(eng, x))

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x = ctx.saved_tensors[0]                 # (raises if x or a parameter was written in place since the forward)
        needs = ctx.needs_input_grad[3:]
        dx, gbuf = net_backward(ctx.eng, ctx.net, _dense(ctx.eng, x), gy.float().contiguous(), ctx.needs_input_grad[2],
                                any(needs))
        if dx is not None:
            dx = dx.view(ctx.x_shape).to(ctx.x_dtype)
        return (None, None, dx) + tuple(_param_grads(ctx.eng, ctx.net, gbuf, needs))


def _dense(eng, x):
    """x as the library reads it: [rows, features] fp32, dense, on the engine's device (x itself when it already is)."""
    return x.reshape(x.shape[0], -1).to(eng.device, torch.float32).contiguous()


def used_draws(eng, rows, eps, noise):
    """The standard-normal draws a sampler call of `rows` rows just used (N(mu, s^2) kinds with noise on): the caller's
    `eps`, or the Philox draws the library left in its eps panel -- a copy, taken in stream order behind that call."""
    if not noise or eng.arch.prior in ("hypersphere_uniform", False):
        return None
    if eps is not None:
        return eps.to(eng.device, torch.float32).reshape(rows, -1).clone()
    return eng.panel("eps")[:rows].clone()


class HipReparam(torch.autograd.Function):
    """The sampler (rmt:734-740; per prior kind rmt:795-816): `HipReparam.apply(engine, noise, seed, offset, eps,
    mu_logvar)` -> z [rows, Z], rows <= max_batch.  Forward = `engine.reparam`; backward = `engine.reparam_backward` on
    the draws this forward used."""

    @staticmethod
    def forward(ctx, eng, noise, seed, offset, eps, mu_logvar):
        z = eng.reparam(_dense(eng, mu_logvar), eps=eps, noise=noise, seed=seed, offset=offset)
        ctx.eng, ctx.noise, ctx.dtype = eng, noise, mu_logvar.dtype
        ctx.used = used_draws(eng, mu_logvar.shape[0], eps, noise)     # (a private copy: no cycle, nobody else writes it)
        ctx.save_for_backward(mu_logvar)
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, dz):
        ml = _dense(ctx.eng, ctx.saved_tensors[0])
        d = ctx.eng.reparam_backward(ml, ctx.used, dz.float().contiguous(), noise=ctx.noise)
        return None, None, None, None, None, d.to(ctx.dtype)


_served_warned = [False]


def warn_served_once():
    """The rollout server answers a graph-building call: say once that the served path is inference-only."""
    if not _served_warned[0]:
        _served_warned[0] = True
        print("physicsvae_amd: forward() served by the rollout server returns no autograd graph (inference only); "
              "pass the observation on the GPU, or stop the server, to train through forward()", file=sys.stderr)


class HipPolicy(torch.autograd.Function):
    """`PhysicsVAE.forward` (rmt:742-771) under autograd, keeping its one library call (`pvae_infer_logits`, so the action
    is the same bits as without a graph): `HipPolicy.apply(model, obs, eps, noise, offset, want_s2, counts, *params)` with
    params = TE | MD | MH | WM views (`counts` = how many of each) -> (a_hat [rows, Da], z [rows, Z], mu_logvar
    [rows, n_out of TE], s2 [rows, Db] or None without `want_s2`), rows <= max_batch.
    Backward, from the saved observation, [s_body | z], [s_body | a_hat], mu_logvar and the draws: WM (when s2 has a
    gradient; its input gradient joins the action's), the helper (tanh seed, dy = range * d a_hat) and MD on [s_body | z],
    then the sampler, then TE."""

    @staticmethod
    def forward(ctx, model, obs, eps, noise, offset, want_s2, counts, *params):
        eng = model.engine
        Da, Z = eng.arch.Da, eng.arch.Z
        x = _dense(eng, obs)
        rows = x.shape[0]
        logits, s2, z = eng.infer_logits(x, model.__dict__["_als"].on_device(eng.device), eps=eps if noise else None,
                                         noise=noise, seed=model._rng_seed, offset=offset, want_s2=want_s2)
        if eng.arch.te_out == 2 * Z:
            ml = torch.cat([eng.read("mu", rows), eng.read("logvar", rows)], dim=1)
        else:                                    # (unit-sphere / no-prior encoders: the raw encoder output e)
            ml = eng.read("mu", rows)
        a = logits[:, :Da].contiguous()
        # (nothing on ctx refers to the model or to an output: the module keeps this forward's outputs in its `_cur_*` state)
        ctx.eng, ctx.mh_range = eng, float(model._motor_decoder_helper_range or 0.0)
        ctx.noise, ctx.counts, ctx.obs_dtype = noise, counts, obs.dtype
        ctx.used = used_draws(eng, rows, eps, noise)                   # (a private copy: no cycle, nobody else writes it)
        ctx.save_for_backward(obs, a, z, ml, *params)
        return a, z, ml, s2

    @staticmethod
    @once_differentiable
    def backward(ctx, g_a, g_z, g_ml, g_s2):
        obs_in, a, z, ml = ctx.saved_tensors[:4]     # (raises if any of them or a parameter was written in place since)
        eng = ctx.eng
        Db, Da, Z = eng.arch.Db, eng.arch.Da, eng.arch.Z
        n_te, n_md, n_mh, n_wm = ctx.counts
        needs = ctx.needs_input_grad[7:]
        need_te, need_md = needs[:n_te], needs[n_te: n_te + n_md]
        need_mh, need_wm = needs[n_te + n_md: n_te + n_md + n_mh], needs[n_te + n_md + n_mh:]
        want_obs = ctx.needs_input_grad[1]
        obs = _dense(eng, obs_in)
        s_body = obs[:, :Db]
        d_obs = torch.zeros_like(obs) if want_obs else None
        g_wm = g_mh = g_md = g_te = None
        if g_s2 is not None and (any(need_wm) or any(need_md) or any(need_mh) or any(need_te) or want_obs):
            x_wm = torch.cat([s_body, a], dim=1)
            dx, g_wm = net_backward(eng, NET_WM, x_wm, g_s2.float().contiguous(), True, any(need_wm))
            g_a = dx[:, Db: Db + Da] if g_a is None else g_a + dx[:, Db: Db + Da]
            if want_obs:
                d_obs[:, :Db] += dx[:, :Db]
        want_z = any(need_te) or want_obs               # (z feeds nothing but the encoder's gradient and the observation's)
        dz = g_z.float() if g_z is not None else None
        if g_a is not None:
            g_a = g_a.float().contiguous()
            md_in = torch.cat([s_body, z], dim=1)
            stacks = [(NET_MD, g_a, need_md)]
            if n_mh:
                stacks.append((NET_MH, g_a * ctx.mh_range, need_mh))
            grads = {}
            for net, dy, need in stacks:
                dx, grads[net] = net_backward(eng, net, md_in, dy, want_z, any(need))
                if dx is not None:
                    dz = dx[:, Db: Db + Z] if dz is None else dz + dx[:, Db: Db + Z]
                    if want_obs:
                        d_obs[:, :Db] += dx[:, :Db]
            g_md, g_mh = grads.get(NET_MD), grads.get(NET_MH)
        d_ml = g_ml.float() if g_ml is not None else None
        if dz is not None and want_z:
            d = torch.cat([eng.reparam_backward(ml[lo:hi], ctx.used[lo:hi] if ctx.used is not None else None,
                                                dz[lo:hi].contiguous(), noise=ctx.noise)
                           for lo, hi in chunks(dz.shape[0], eng.max_batch)])
            d_ml = d if d_ml is None else d_ml + d
        if d_ml is not None and want_z:
            dx, g_te = net_backward(eng, NET_TE, obs, d_ml.contiguous(), want_obs, any(need_te))
            if want_obs:
                d_obs += dx
        out = (_param_grads(eng, NET_TE, g_te, need_te) + _param_grads(eng, NET_MD, g_md, need_md)
               + _param_grads(eng, NET_MH, g_mh, need_mh) + _param_grads(eng, NET_WM, g_wm, need_wm))
        d_obs = d_obs.view(obs_in.shape).to(ctx.obs_dtype) if d_obs is not None else None
        return (None, d_obs, None, None, None, None, None) + tuple(out)


def stack_set_forward(eng, x, want=None):
    """`StackSetEngine.forward` over any number of rows (chunks of at most `max_batch`)."""
    if x.shape[0] <= eng.max_batch:
        return eng.forward(x, want)
    parts = [eng.forward(x[lo:hi], want) for lo, hi in chunks(x.shape[0], eng.max_batch)]
    return [None if p[0] is None else torch.cat(p) for p in zip(*parts)]


def stack_set_grad_views(eng, gbuf):
    """`gbuf` (a flat gradient with the stack set's arena layout) as views shaped like the parameters, stack by stack in
    layer order: weight, bias, weight, bias, ..."""
    return [t for s in range(len(eng.stacks)) for wb in eng.views(s, gbuf) for t in wb]


class HipStackSet(torch.autograd.Function):
    """A stack set under autograd (FullyConnectedPolicy.forward, rmt:430-441: the policy, the value and the log-std
    stacks on one observation): `HipStackSet.apply(engine, x, *params)` with params = the weight / bias views of all stacks,
    stack by stack in layer order -> (out_0, ..., out_{S-1}).  Forward = `engine.forward` (chunked), the very call made
    without a graph.  Backward = `engine.backward` per chunk: an output nobody differentiates costs nothing, a stack none
    of whose parameters wants a gradient (frozen) passes the input gradient only, and the parameter gradient is summed over
    the chunks inside the library (accumulate = 1 after the first).  x and the parameters are kept with
    `save_for_backward` only; no double backward."""

    @staticmethod
    def forward(ctx, eng, x, *params):
        ctx.eng, ctx.x_shape, ctx.x_dtype = eng, x.shape, x.dtype
        ctx.set_materialize_grads(False)         # an output nobody differentiates arrives as None, not as a tensor of zeros
        ctx.save_for_backward(x, *params)
        return tuple(stack_set_forward(eng, x.reshape(x.shape[0], -1).to(eng.device, torch.float32).contiguous()))

    @staticmethod
    @once_differentiable
    def backward(ctx, *gys):
        eng = ctx.eng
        x = ctx.saved_tensors[0]                 # (raises if x or a parameter was written in place since the forward)
        x = x.reshape(x.shape[0], -1).to(eng.device, torch.float32).contiguous()
        needs = ctx.needs_input_grad[2:]
        want_dx = ctx.needs_input_grad[1]
        mask, k = 0, 0
        for s in range(len(eng.stacks)):
            n = 2 * len(eng.stack_layers(s))
            if any(needs[k: k + n]) and gys[s] is not None:
                mask |= 1 << s
            k += n
        dys = [None if g is None else g.float().contiguous() for g in gys]
        gbuf = torch.empty(eng.arena_floats, dtype=torch.float32, device=eng.device) if mask else None
        if not (want_dx or mask) or all(d is None for d in dys):
            return (None, None) + (None,) * len(needs)
        dxs = [eng.backward(x[lo:hi], [None if d is None else d[lo:hi] for d in dys], want_dx, gbuf, mask, accumulate=i > 0)
               for i, (lo, hi) in enumerate(chunks(x.shape[0], eng.max_batch))]
        dx = None
        if want_dx:
            dx = (dxs[0] if len(dxs) == 1 else torch.cat(dxs)).view(ctx.x_shape).to(ctx.x_dtype)
        grads = [None] * len(needs)
        if mask:
            views, k = stack_set_grad_views(eng, gbuf), 0
            for s in range(len(eng.stacks)):
                n = 2 * len(eng.stack_layers(s))
                if (mask >> s) & 1:
                    grads[k: k + n] = [v if nd else None for v, nd in zip(views[k: k + n], needs[k: k + n])]
                k += n
        return (None, dx) + tuple(grads)


class HipImagineCost(torch.autograd.Function):
    """The planner's rollout cost, differentiable in the codes and the start states: `HipImagineCost.apply(module, s0, z,
    targets, group, col_weight, step_weight)` -> cost [rows] (`PhysicsVAE.imagine_grad`, chunked by environments; the rule:
    refine.py).  The forward runs the backward through the unroll as well and keeps dz (and, group == 1, ds[0]); the
    backward scales them by the incoming per-row gradient.  The model's parameters get NO gradient: every stack is frozen
    in this call.  No double backward."""

    @staticmethod
    def forward(ctx, module, s0, z, targets, group, col_weight, step_weight):
        want_s0 = ctx.needs_input_grad[1]
        if want_s0 and int(group) != 1:
            raise ValueError("s0.grad needs group == 1 (a start state is shared by the rows of its group)")
        out = module.imagine_grad(s0.detach(), z.detach(), targets, group=group, col_weight=col_weight, step_weight=step_weight,
                                  want=("cost", "dz") + (("ds",) if want_s0 else ()))
        ctx.want_s0, ctx.dtypes = want_s0, (s0.dtype, z.dtype)
        ctx.save_for_backward(out["dz"], *((out["ds"][0],) if want_s0 else ()))
        return out["cost"]

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        dz = ctx.saved_tensors[0]
        gy = gy.to(dz.device, torch.float32)
        gz = (gy[None, :, None] * dz).to(ctx.dtypes[1]) if ctx.needs_input_grad[2] else None
        gs = (gy[:, None] * ctx.saved_tensors[1]).to(ctx.dtypes[0]) if ctx.want_s0 else None
        return None, gs, gz, None, None, None, None
