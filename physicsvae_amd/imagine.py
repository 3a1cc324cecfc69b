"""Imagined rollouts: the H-step closed-loop unroll of the policy and the world model -- the rule, in torch.

`imagine_torch` is the specification of `pvae_imagine` (include/pvae.h; `HipEngine.imagine`, `PhysicsVAE.imagine`,
`TrainModel.evaluate_rollout`) and the oracle of its tests.  It computes in the dtype of its inputs and calls nothing of the
library.

The rule.  A call takes `rows` start states s_0 [rows, Db] and a horizon H >= 1, and runs step t = 0 .. H-1 in one of three
modes:

"replay" (the world model alone, open loop)
    a_t = actions[t], given;  s_{t+1} = WM([s_t | a_t]).

"track" (the whole model follows a goal sequence)
    obs_t = [s_t | goals[t]];  h_t = TE(obs_t);  z_t = the sampler by prior kind, exactly as pvae_infer forms it:
        N(mu, s^2) kinds   z = mu + eps_t exp(logvar / 2), eps[t] supplied or drawn from Philox at (seed, offset + t), row r
                           drawing Philox row r; with noise off z = mu
        hypersphere        z = e / max(|e|, 1e-12)
        False              z = e
    a_t = MD([s_t | z_t]) + motor_decoder_helper_range * helper([s_t | z_t]) when the model has the helper (rmt:833-835);
    s_{t+1} = WM([s_t | a_t]).

"prior" (the reference's pass_through in imagination, envs/rllib_env_imitation.py:234-258)
    z_t = z[t] when supplied.  Otherwise it is drawn: normal_zero_mean_one_std z_t = n_t; normal_state_mean_one_std z_t =
    prior(s_t) + n_t, one float32 add; the other two prior kinds need z supplied, as upstream raises there.  n_t is the draw
    the sampler would use as eps at (seed, offset + t): the same counter and the same groups below Z / 4.  The encoder's
    sampler does not run in this mode, so no stream is shared.  Then the decoder, the helper and the world model as in
    "track".

In every mode: input subsets hold as everywhere -- a stack whose first layer does not read the body columns never sees s_t;
the actions are the decoder's means, with no exploration noise and no clipping; the value branch does not run.

Per-horizon error.  With targets[t] [rows, Db]: err[t] = float32(sum_{r,c} double(d_rc) * double(d_rc) / (rows * Db)), d =
s_{t+1} - targets[t] in float32 (in the inputs' dtype here).  On the device squares and sums are in double, in a fixed order,
without atomics: the same bits on every call -- the convention of the diagnostics and clip launches.

Results, all optional, dense and row-major: states [H, rows, Db] = s_1 .. s_H, actions [H, rows, Da], z [H, rows, Z] (none
in replay mode), err [H].

Draws.  `imagine_torch` cannot draw from Philox: where the rule draws, the caller passes the draws (`eps` in track mode,
`n` in prior mode) -- for a comparison with the device, the ones the device used.
"""
import torch

MODES = ("replay", "track", "prior")
NET_KEYS = {"te": "_task_encoder", "md": "_motor_decoder", "mh": "_motor_decoder_helper", "wm": "_world_model",
            "pr": "_latent_prior"}
DRAWN_PRIORS = ("normal_zero_mean_one_std", "normal_state_mean_one_std")

_ACTS = {"relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "elu": torch.nn.functional.elu,
         "linear": lambda x: x, None: lambda x: x}


def check_mode(mode, prior, goals=None, actions=None, z=None):
    """The refusals of the rule, by name: what `pvae_imagine` answers with -1."""
    if mode not in MODES:
        raise ValueError("mode %r: one of %s" % (mode, MODES))
    if mode == "replay" and actions is None:
        raise ValueError("replay mode needs actions")
    if mode == "track" and goals is None:
        raise ValueError("track mode needs goals")
    if mode == "prior" and z is None and prior not in DRAWN_PRIORS:
        raise ValueError("prior mode needs z under latent_prior_type %r" % (prior,))


def _stack(sd, net, acts, x, dtype):
    """One FC stack of the state dict on its (windowed) input: hidden activations `acts`, linear last layer."""
    for i in range(len(acts) + 1):
        w = sd["%s._model.%d._model.0.weight" % (net, i)].to(dtype)
        b = sd["%s._model.%d._model.0.bias" % (net, i)].to(dtype)
        x = x @ w.t() + b
        if i < len(acts):
            x = _ACTS[acts[i]](x)
    return x


def _window(inputs, Db, width):
    """Columns of a [body | task] input that a first layer with the subset `inputs` reads."""
    inputs = tuple(inputs)
    return (0, width) if inputs == ("body", "task") else ((0, Db) if inputs == ("body",) else (Db, width))


def sampler_torch(prior, h, Z, eps, noise):
    if prior is False:
        return h
    if prior == "hypersphere_uniform":
        return h / h.norm(dim=1, keepdim=True).clamp_min(1e-12)
    mu, lv = h[:, :Z], h[:, Z:]
    return mu + eps * torch.exp(lv / 2) if noise else mu


def step_torch(arch, sd, mode, s, goal=None, action=None, z=None, eps=None, n=None, noise=True):
    """One step of the rule from the states `s`: (a_t, z_t or None, s_{t+1})."""
    dtype, Db, Z = s.dtype, arch.Db, arch.Z
    if mode == "replay":
        a, zt = action, None
    else:
        if mode == "track":
            obs = torch.cat([s, goal], 1)
            lo, hi = _window(arch.te_inputs, Db, 2 * Db)
            zt = sampler_torch(arch.prior, _stack(sd, NET_KEYS["te"], arch.te.acts, obs[:, lo:hi], dtype), Z, eps, noise)
        elif z is not None:
            zt = z
        elif arch.prior == "normal_zero_mean_one_std":
            zt = n
        else:
            zt = _stack(sd, NET_KEYS["pr"], arch.pr.acts, s, dtype) + n
        x = torch.cat([s, zt], 1)
        lo, hi = _window(arch.md_inputs, Db, Db + Z)
        a = _stack(sd, NET_KEYS["md"], arch.md.acts, x[:, lo:hi], dtype)
        if arch.mh is not None:
            a = a + arch.mh_range * torch.tanh(_stack(sd, NET_KEYS["mh"], arch.mh.acts, x[:, lo:hi], dtype))
    return a, zt, _stack(sd, NET_KEYS["wm"], arch.wm.acts, torch.cat([s, a], 1), dtype)


def horizon_error(states, targets):
    """err [H] of states [H, rows, Db] against targets of the same shape: the difference in the inputs' dtype, squares and
    sums in double, the mean as float32."""
    d = (states - targets).double()
    return (d * d).sum(dim=(1, 2)).div(states.shape[1] * states.shape[2]).float()


def imagine_torch(arch, sd, mode, s0, horizon, goals=None, actions=None, z=None, eps=None, n=None, targets=None, noise=True,
                  teacher=None):
    """The rule on an `Arch` and a module's state dict.  goals / targets [H, rows, Db], actions [H, rows, Da], z / eps / n
    [H, rows, Z], all in the dtype of s0.  `teacher` [H, rows, Db] (tests): step t starts from teacher[t - 1] instead of
    its own s_t -- the device's states, so that one step's error is measured and not H steps' drift.
    Returns {"states", "actions", "z" (None in replay mode), "err" (None without targets)}."""
    check_mode(mode, arch.prior, goals, actions, z)
    if horizon < 1:
        raise ValueError("horizon %d < 1" % horizon)
    if mode == "track" and noise and eps is None and arch.prior in DRAWN_PRIORS:
        raise ValueError("imagine_torch cannot draw: pass eps")
    if mode == "prior" and z is None and n is None:
        raise ValueError("imagine_torch cannot draw: pass n")
    sd = {k: v.detach().to(s0.device) for k, v in sd.items() if k.split(".")[0] in NET_KEYS.values() and k.endswith(("weight", "bias"))}
    pick = lambda x, t: None if x is None else x[t]                                  # noqa: E731
    s, S, A, Zs = s0, [], [], []
    with torch.no_grad():
        for t in range(horizon):
            if teacher is not None and t > 0:
                s = teacher[t - 1].to(s0.dtype)
            a, zt, s = step_torch(arch, sd, mode, s, pick(goals, t), pick(actions, t), pick(z, t), pick(eps, t), pick(n, t), noise)
            S.append(s), A.append(a), Zs.append(zt)
    states = torch.stack(S)
    return {"states": states, "actions": torch.stack(A), "z": None if mode == "replay" else torch.stack(Zs),
            "err": None if targets is None else horizon_error(states, targets)}
