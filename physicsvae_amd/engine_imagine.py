"""Imagined rollouts through the library: `HipEngine.imagine` (include/pvae.h pvae_imagine; the rule: imagine.py).
"""
import ctypes as C

import torch

from . import _lib
from .imagine import check_mode


class ImagineSurface:
    """Base class of `HipEngine`.  Expects of the engine: `lib`, `ctx`, `device`, `arch`, `max_batch`, `_need_gpu()` and
    `_stream()`.  Keeps `_imagine_scratch` and `imagine_launched` of its own."""

    def imagine_launches(self, mode):
        """(per_step, per_call) as pvae_imagine_launches states them: a call of H steps with `targets` issues
        per_step * H + per_call launches (prior mode under the learned prior: with z drawn)."""
        self._need_gpu()
        a, b = C.c_int32(), C.c_int32()
        _lib.check(self.lib.pvae_imagine_launches(self.ctx, _lib.IMAGINE_MODES[mode], C.byref(a), C.byref(b)), "pvae_imagine_launches")
        return a.value, b.value

    def _imagine_src(self, x, width, horizon, rows, what, keep):
        """pvae_imagine_src of a dense tensor [H, rows, width] ([rows, width] for s0) or of an in-place source
        (tensor [N, width], row_index int32 [rows][, shift]): element (t, r, :) = tensor[row_index[r] + shift + t]."""
        src = _lib.ImagineSrc()
        if x is None:
            return src
        if isinstance(x, (tuple, list)):
            data, index = x[0], x[1]
            shift = int(x[2]) if len(x) > 2 else 0
            if not (data.dtype == torch.float32 and data.device == self.device and data.dim() == 2 and data.is_contiguous()
                    and data.shape[1] == width):
                raise ValueError("%s: an in-place source is a contiguous float32 [N, %d] tensor on the engine's device" % (what, width))
            if not (index.dtype == torch.int32 and index.device == self.device and index.is_contiguous() and index.numel() >= rows):
                raise ValueError("%s: row_index is a contiguous int32 device tensor of at least %d entries" % (what, rows))
            keep += [data, index]
            src.base, src.ld, src.step, src.row_index = data.data_ptr() + 4 * shift * width, width, width, index.data_ptr()
            return src
        shape = (rows, width) if horizon is None else (horizon, rows, width)
        if tuple(x.shape) != shape:
            raise ValueError("%s: expected shape %s, got %s" % (what, shape, tuple(x.shape)))
        x = x.to(self.device, torch.float32).contiguous()
        keep.append(x)
        src.base, src.ld, src.step = x.data_ptr(), width, rows * width
        return src

    def imagine(self, mode, s0, horizon, goals=None, actions=None, z=None, eps=None, targets=None, noise=True, seed=0, offset=0,
                want=("states", "actions", "z"), out=None):
        """`horizon` closed-loop steps of the policy and the world model from the start states s0 in ONE library call (no
        torch op per step, no host synchronisation); the rule is `imagine.imagine_torch`'s.  mode "replay" (actions given),
        "track" (goals given; eps [H, rows, Z] supplied, or Philox at (seed, offset + t); noise False: z = mu) or "prior" (z
        given, or drawn where the prior kind allows).  Every source is a dense tensor ([H, rows, D]; s0 [rows, Db]) or an
        in-place pair (tensor [N, D], row_index int32 [rows][, shift]) read as tensor[row_index[r] + shift + t].  Returns a
        dict with the tensors named in `want` ("states" [H, rows, Db] = s_1 .. s_H, "actions", "z") and, with `targets`,
        "err" [H].  `out`: a dict an earlier call of the same shape returned, overwritten instead of allocating (as `infer`'s
        `out`).  `imagine_launched` holds the number of launches the last call enqueued, as the library returned it."""
        self._need_gpu()
        Db, Da, Z = self.arch.Db, self.arch.Da, self.arch.Z
        H = int(horizon)
        check_mode(mode, self.arch.prior, goals, actions, z)
        rows = int(s0[1].shape[0] if isinstance(s0, (tuple, list)) else s0.shape[0])
        keep = []
        args = _lib.ImagineArgs()
        args.mode, args.rows, args.horizon, args.noise = _lib.IMAGINE_MODES[mode], rows, H, 1 if noise else 0
        args.s0 = self._imagine_src(s0, Db, None, rows, "s0", keep)
        Hs = max(H, 1)
        args.goals = self._imagine_src(goals if mode == "track" else None, Db, Hs, rows, "goals", keep)
        args.actions = self._imagine_src(actions if mode == "replay" else None, Da, Hs, rows, "actions", keep)
        args.z = self._imagine_src(z if mode == "prior" else None, Z, Hs, rows, "z", keep)
        args.targets = self._imagine_src(targets, Db, Hs, rows, "targets", keep)
        if eps is not None and mode == "track":
            if tuple(eps.shape) != (H, rows, Z):
                raise ValueError("eps: expected shape %s, got %s" % ((H, rows, Z), tuple(eps.shape)))
            eps = eps.to(self.device, torch.float32).contiguous()
            keep.append(eps)
            args.eps = eps.data_ptr()
        args.rng_seed, args.rng_offset = int(seed), int(offset)
        res = {}
        widths = {"states": Db, "actions": Da, "z": Z}
        for name in want:
            if name not in widths:
                raise ValueError("want: names among %s" % sorted(widths))
            if name == "z" and mode == "replay":
                continue
            t = out.get(name) if out is not None else None
            if t is None or tuple(t.shape) != (Hs, rows, widths[name]):
                t = torch.empty(Hs, rows, widths[name], dtype=torch.float32, device=self.device)
            res[name] = t
            setattr(args, name + "_out", t.data_ptr())
        if targets is not None:
            e = out.get("err") if out is not None else None
            res["err"] = e if e is not None and tuple(e.shape) == (Hs,) else torch.empty(Hs, dtype=torch.float32, device=self.device)
            args.err = res["err"].data_ptr()
            need = self.lib.pvae_imagine_scratch_bytes(self.ctx, Hs)
            sc = getattr(self, "_imagine_scratch", None)
            if sc is None or sc.numel() * 8 < need:
                sc = self._imagine_scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
            args.scratch, args.scratch_bytes = sc.data_ptr(), sc.numel() * 8
        self.imagine_launched = _lib.check(self.lib.pvae_imagine(self.ctx, C.byref(args), self._stream()), "pvae_imagine")
        return res
