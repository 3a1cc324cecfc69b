"""Planning over imagined rollouts through the library: `HipEngine.plan` (include/pvae.h pvae_plan; the rule: plan.py).
"""
import ctypes as C

import torch

from . import _lib
from .plan import check_plan

PLAN_OUTPUTS = ("plan_z", "best", "cost", "iter_cost", "a0", "s1", "z_cand", "noise_out", "states")


class PlanSurface:
    """Base class of `HipEngine`, beside `ImagineSurface` (whose `_imagine_src` builds the sources).  Expects of the engine:
    `lib`, `ctx`, `device`, `arch`, `max_batch`, `_need_gpu()` and `_stream()`.  Keeps `_plan_scratch` and `plan_launched`
    of its own."""

    def plan_launches(self):
        """(per_step, per_iter, closing) as pvae_plan_launches states them: a call issues iters * (H * per_step + per_iter)
        + closing launches."""
        self._need_gpu()
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self.lib.pvae_plan_launches(self.ctx, C.byref(a), C.byref(b), C.byref(c)), "pvae_plan_launches")
        return a.value, b.value, c.value

    def _plan_dense(self, x, shape, what, keep):
        if x is None:
            return None
        if tuple(x.shape) != shape:
            raise ValueError("%s: expected shape %s, got %s" % (what, shape, tuple(x.shape)))
        x = x.to(self.device, torch.float32).contiguous()
        keep.append(x)
        return x.data_ptr()

    def plan(self, s0, targets, horizon, candidates, iters=1, sigma=1.0, lam=0.0, nominal=None, noise=None, col_weight=None,
             step_weight=None, seed=0, offset=0, row0=0, want=("plan_z", "best", "cost", "iter_cost", "a0", "s1"), out=None):
        """`iters` rounds of `candidates` sampled code sequences per environment, unrolled `horizon` steps and scored against
        `targets`, in ONE library call (no torch op, no host synchronisation); the rule is `plan.plan_torch`'s.  s0 [E, Db]
        and targets [H, E, Db] are dense tensors or in-place pairs (tensor [N, Db], row_index int32 [E][, shift]) over
        environments, as `imagine`'s sources; E * candidates <= max_batch.  nominal [H, E, Z] (None: zeros); noise [iters, H,
        E * K, Z] supplied, or Philox at (seed, offset + i * H + t) with Philox row row0 + r; col_weight [Db], step_weight [H].
        Returns a dict with the tensors named in `want` (among PLAN_OUTPUTS; "z_cand", "noise_out" and "states" are the last
        iteration's).  `out`: a dict an earlier call of the same shape returned, overwritten instead of allocating.
        `plan_launched` holds the number of launches the call enqueued, as the library returned it."""
        self._need_gpu()
        Db, Da, Z = self.arch.Db, self.arch.Da, self.arch.Z
        H, K, iters = int(horizon), int(candidates), int(iters)
        E = int(s0[1].shape[0] if isinstance(s0, (tuple, list)) else s0.shape[0])
        check_plan(E, K, H, iters, float(sigma), float(lam), self.max_batch)
        rows = E * K
        keep = []
        args = _lib.PlanArgs()
        args.envs, args.candidates, args.horizon, args.iters = E, K, H, iters
        args.sigma, args.lam = float(sigma), float(lam)
        args.s0 = self._imagine_src(s0, Db, None, E, "s0", keep)
        args.targets = self._imagine_src(targets, Db, H, E, "targets", keep)
        args.nominal = self._plan_dense(nominal, (H, E, Z), "nominal", keep)
        args.noise = self._plan_dense(noise, (iters, H, rows, Z), "noise", keep)
        args.col_weight = self._plan_dense(col_weight, (Db,), "col_weight", keep)
        args.step_weight = self._plan_dense(step_weight, (H,), "step_weight", keep)
        args.rng_seed, args.rng_offset, args.row0 = int(seed), int(offset), int(row0)
        shapes = {"plan_z": (H, E, Z), "best": (E,), "cost": (E, K), "iter_cost": (iters, E), "a0": (E, Da), "s1": (E, Db),
                  "z_cand": (H, rows, Z), "noise_out": (H, rows, Z), "states": (H, rows, Db)}
        res = {}
        for name in want:
            if name not in shapes:
                raise ValueError("want: names among %s" % (PLAN_OUTPUTS,))
            dtype = torch.int32 if name == "best" else torch.float32
            t = out.get(name) if out is not None else None
            if t is None or tuple(t.shape) != shapes[name] or t.dtype != dtype:
                t = torch.empty(shapes[name], dtype=dtype, device=self.device)
            res[name] = t
            setattr(args, name, t.data_ptr())
        need = self.lib.pvae_plan_scratch_bytes(self.ctx, H, rows)
        sc = getattr(self, "_plan_scratch", None)
        if sc is None or sc.numel() * 8 < need:
            sc = self._plan_scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        args.scratch, args.scratch_bytes = sc.data_ptr(), sc.numel() * 8
        self.plan_launched = _lib.check(self.lib.pvae_plan(self.ctx, C.byref(args), self._stream()), "pvae_plan")
        return res
