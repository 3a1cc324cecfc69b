"""Backpropagation through imagined rollouts and gradient-refined plans through the library: `HipEngine.imagine_grad` and
`HipEngine.refine` (include/pvae.h pvae_imagine_grad, pvae_plan_refine; the rule: refine.py).
"""
import ctypes as C

import torch

from . import _lib
from .refine import check_refine

GRAD_OUTPUTS = ("cost", "dz", "ds", "states")
REFINE_OUTPUTS = ("plan_z", "cost", "best_iter", "iter_cost", "a0", "s1", "z_iters", "grad")


class RefineSurface:
    """Base class of `HipEngine`, beside `ImagineSurface` (whose `_imagine_src` builds the sources) and `PlanSurface` (whose
    `_plan_dense` checks the dense inputs).  Expects of the engine: `lib`, `ctx`, `device`, `arch`, `max_batch`, `_need_gpu()`
    and `_stream()`.  Keeps `_refine_scratch`, `imagine_grad_launched` and `refine_launched` of its own."""

    def imagine_grad_launches(self, horizon=None, backward=True):
        """(fwd_per_step, bwd_per_step, per_call) as pvae_imagine_grad_launches states them -- or, with `horizon`, the
        number of launches of one call: per_call + H * fwd_per_step, and with the backward + H * bwd_per_step + (H - 1) *
        (fwd_per_step - 1)."""
        self._need_gpu()
        f, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self.lib.pvae_imagine_grad_launches(self.ctx, C.byref(f), C.byref(b), C.byref(c)), "pvae_imagine_grad_launches")
        if horizon is None:
            return f.value, b.value, c.value
        H = int(horizon)
        return c.value + H * f.value + (H * b.value + (H - 1) * (f.value - 1) if backward else 0)

    def refine_launches(self, horizon=None, steps=None):
        """(per_iter, per_call) as pvae_plan_refine_launches states them -- or, with `horizon` and `steps`, the number of
        launches of one call: steps * (imagine_grad's + per_iter) + imagine_grad's forward-only count + per_call."""
        self._need_gpu()
        a, b = C.c_int32(), C.c_int32()
        _lib.check(self.lib.pvae_plan_refine_launches(self.ctx, C.byref(a), C.byref(b)), "pvae_plan_refine_launches")
        if horizon is None:
            return a.value, b.value
        return (int(steps) * (self.imagine_grad_launches(horizon) + a.value) + self.imagine_grad_launches(horizon, backward=False)
                + b.value)

    def _refine_scratch_for(self, need):
        sc = getattr(self, "_refine_scratch", None)
        if sc is None or sc.numel() * 8 < need:
            sc = self._refine_scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        return sc

    def _refine_outputs(self, args, want, shapes, names, out, rename=None):
        res = {}
        for name in want:
            if name not in shapes:
                raise ValueError("want: names among %s" % (names,))
            dtype = torch.int32 if name == "best_iter" else torch.float32
            t = out.get(name) if out is not None else None
            if t is None or tuple(t.shape) != shapes[name] or t.dtype != dtype:
                t = torch.empty(shapes[name], dtype=dtype, device=self.device)
            res[name] = t
            setattr(args, (rename or {}).get(name, name), t.data_ptr())
        return res

    def imagine_grad(self, s0, z, targets, group=1, col_weight=None, step_weight=None, want=("cost", "dz"), out=None):
        """The planner's unroll on the codes z [H, E * group, Z] from the start states s0 [E, Db] against targets [H, E, Db]
        (dense tensors or in-place pairs over environments, as `plan`'s), and its backward through the decoder, the helper
        and the world model, in ONE library call; the rule is `refine.rollout_grad_torch`'s.  Returns a dict with the
        tensors named in `want` (among GRAD_OUTPUTS): "cost" [rows], "dz" [H, rows, Z], "ds" [H, rows, Db], "states"
        [H, rows, Db].  Without "dz" and "ds" the call is forward only.  The model's parameters get no gradient.
        `imagine_grad_launched` holds the number of launches the call enqueued, as the library returned it."""
        self._need_gpu()
        Db, Z = self.arch.Db, self.arch.Z
        G = int(group)
        E = int(s0[1].shape[0] if isinstance(s0, (tuple, list)) else s0.shape[0])
        if z.dim() != 3:
            raise ValueError("z: expected [H, rows, Z]")
        H = int(z.shape[0])
        check_refine(E, H, 0, 1.0, self.max_batch, G)
        rows = E * G
        keep = []
        args = _lib.ImagineGradArgs()
        args.envs, args.group, args.horizon = E, G, H
        args.s0 = self._imagine_src(s0, Db, None, E, "s0", keep)
        args.targets = self._imagine_src(targets, Db, H, E, "targets", keep)
        args.z = self._plan_dense(z, (H, rows, Z), "z", keep)
        args.col_weight = self._plan_dense(col_weight, (Db,), "col_weight", keep)
        args.step_weight = self._plan_dense(step_weight, (H,), "step_weight", keep)
        shapes = {"cost": (rows,), "dz": (H, rows, Z), "ds": (H, rows, Db), "states": (H, rows, Db)}
        res = self._refine_outputs(args, want, shapes, GRAD_OUTPUTS, out, {"states": "states_out"})
        sc = self._refine_scratch_for(self.lib.pvae_imagine_grad_scratch_bytes(self.ctx, H, rows))
        args.scratch, args.scratch_bytes = sc.data_ptr(), sc.numel() * 8
        self.imagine_grad_launched = _lib.check(self.lib.pvae_imagine_grad(self.ctx, C.byref(args), self._stream()), "pvae_imagine_grad")
        return res

    def refine(self, s0, targets, horizon, steps, lr, nominal=None, col_weight=None, step_weight=None,
               want=("plan_z", "cost", "best_iter", "iter_cost", "a0", "s1"), out=None):
        """`steps` Adam steps on the code sequences of E environments from `nominal` [H, E, Z] (None: zeros), each a forward
        and a backward through the `horizon`-step unroll, keeping the best iterate, in ONE library call (no torch op, no
        host synchronisation); the rule is `refine.refine_torch`'s.  s0 [E, Db] and targets [H, E, Db] as in `plan`;
        E <= max_batch.  Returns a dict with the tensors named in `want` (among REFINE_OUTPUTS).  `refine_launched` holds
        the number of launches the call enqueued, as the library returned it."""
        self._need_gpu()
        Db, Da, Z = self.arch.Db, self.arch.Da, self.arch.Z
        H, steps = int(horizon), int(steps)
        E = int(s0[1].shape[0] if isinstance(s0, (tuple, list)) else s0.shape[0])
        check_refine(E, H, steps, float(lr), self.max_batch)
        keep = []
        args = _lib.PlanRefineArgs()
        args.envs, args.horizon, args.steps, args.lr = E, H, steps, float(lr)
        args.s0 = self._imagine_src(s0, Db, None, E, "s0", keep)
        args.targets = self._imagine_src(targets, Db, H, E, "targets", keep)
        args.nominal = self._plan_dense(nominal, (H, E, Z), "nominal", keep)
        args.col_weight = self._plan_dense(col_weight, (Db,), "col_weight", keep)
        args.step_weight = self._plan_dense(step_weight, (H,), "step_weight", keep)
        shapes = {"plan_z": (H, E, Z), "cost": (E,), "best_iter": (E,), "iter_cost": (steps + 1, E), "a0": (E, Da), "s1": (E, Db),
                  "z_iters": (steps + 1, H, E, Z), "grad": (H, E, Z)}
        res = self._refine_outputs(args, want, shapes, REFINE_OUTPUTS, out)
        sc = self._refine_scratch_for(self.lib.pvae_plan_refine_scratch_bytes(self.ctx, H, E))
        args.scratch, args.scratch_bytes = sc.data_ptr(), sc.numel() * 8
        self.refine_launched = _lib.check(self.lib.pvae_plan_refine(self.ctx, C.byref(args), self._stream()), "pvae_plan_refine")
        return res
