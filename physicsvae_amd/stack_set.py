"""`StackSetEngine`: the stack set (include/pvae.h `pvae_fc_*`) FullyConnectedPolicy and PhysicsVAE's value branch run on.
Its PPO learner surface is `engine_ppo.PpoSurface`.
"""
import ctypes as C

import torch

from . import _lib
from .engine_ppo import PpoSurface, make_ppo_batch


class StackSetEngine(PpoSurface):
    """A stack set (include/pvae.h `pvae_fc_*`): S fully connected stacks on ONE shared input, run together -- one launch
    per layer depth for all stacks.  Owns the flat parameter arena and the workspace.  `stacks`: [(Stack of the hidden
    layers, n_out)], at most four; every stack ends in a linear output layer (rmt:234-283 as FullyConnectedPolicy uses
    it, rmt:386-427).  There is no CPU fallback: the calls need a GPU, the layout queries do not."""

    def __init__(self, n_in, stacks, max_batch, device="cuda"):
        self.lib = _lib.load()
        self.n_in, self.max_batch = int(n_in), int(max_batch)
        self.stacks = [(st, int(n_out)) for st, n_out in stacks]
        if not 1 <= len(self.stacks) <= _lib.FC_MAX_STACKS:
            raise NotImplementedError("a stack set holds 1..%d stacks, got %d" % (_lib.FC_MAX_STACKS, len(self.stacks)))
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        cfg = _lib.FcConfig()
        cfg.n_in, cfg.n_stacks, cfg.max_batch = self.n_in, len(self.stacks), self.max_batch
        for s, (st, n_out) in enumerate(self.stacks):
            cfg.depth[s], cfg.n_out[s] = len(st.widths), n_out
            for i, (w, a) in enumerate(zip(st.widths, st.acts)):
                cfg.width[s][i], cfg.act[s][i] = w, _lib.LAYER_ACTS[a]
        self.cfg = cfg
        self.arena_floats = _lib.check(int(self.lib.pvae_fc_arena_floats(C.byref(cfg))), "pvae_fc_arena_floats")
        self.layers = []
        info = _lib.LayerInfo()
        for i in range(_lib.check(self.lib.pvae_fc_num_layers(C.byref(cfg)), "pvae_fc_num_layers")):
            _lib.check(self.lib.pvae_fc_layer(C.byref(cfg), i, C.byref(info)), "pvae_fc_layer")
            self.layers.append({f: getattr(info, f) for f, _ in _lib.LayerInfo._fields_})
        self.n_outs = [n for _, n in self.stacks]
        self._ppo_dims = (self.n_in, self.n_outs[0], None)
        self.params = torch.zeros(self.arena_floats, dtype=torch.float32, device=self.device)
        self.ctx = None
        self.workspace = None
        if self.device.type == "cuda":
            ctx = C.c_void_p()
            _lib.check(self.lib.pvae_fc_create(C.byref(cfg), C.byref(ctx)), "pvae_fc_create")
            self.ctx = ctx
            nbytes = self.lib.pvae_fc_workspace_bytes(C.byref(cfg))
            self.workspace = torch.zeros(nbytes // 4 + 64, dtype=torch.float32, device=self.device)
            _lib.check(self.lib.pvae_fc_bind(ctx, self.params.data_ptr(), self.workspace.data_ptr(), nbytes), "pvae_fc_bind")

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.pvae_fc_destroy(self.ctx)
                self.ctx = None
        except Exception:
            pass

    def stack_layers(self, s):
        return [l for l in self.layers if l["net"] == s]

    def views(self, s, arena=None):
        """[(weight [n_out, n_in], bias [n_out])] strided views of stack `s` into `arena` (default: the parameters)."""
        arena = self.params if arena is None else arena
        out = []
        for info in self.stack_layers(s):
            blk = arena[info["w_offset"]: info["w_offset"] + info["n_out_pad"] * info["ld"]].view(info["n_out_pad"], info["ld"])
            out.append((blk[: info["n_out"], : info["n_in"]], arena[info["b_offset"]: info["b_offset"] + info["n_out"]]))
        return out

    def _x(self, x):
        x = x.reshape(x.shape[0], -1).to(self.device, torch.float32).contiguous()
        assert x.shape[1] == self.n_in, "x must be [rows, %d], got %s" % (self.n_in, tuple(x.shape))
        assert 1 <= x.shape[0] <= self.max_batch, "rows %d outside [1, %d]" % (x.shape[0], self.max_batch)
        return x

    def forward(self, x, want=None):
        """x [rows <= max_batch, n_in] -> [out_s [rows, n_out_s] or None where `want[s]` is false]: ONE library call."""
        self._need_gpu()
        x = self._x(x)
        want = [True] * len(self.stacks) if want is None else list(want)
        outs = [torch.empty(x.shape[0], n, dtype=torch.float32, device=self.device) if w else None
                for n, w in zip(self.n_outs, want)]
        ptrs = (C.c_void_p * _lib.FC_MAX_STACKS)(*[o.data_ptr() if o is not None else None for o in outs])
        _lib.check(self.lib.pvae_fc_forward(self.ctx, x.data_ptr(), x.shape[0], ptrs, self._stream()), "pvae_fc_forward")
        return outs

    def backward(self, x, dys, want_dx, grad=None, grad_mask=0, accumulate=False):
        """`pvae_fc_backward`: dys[s] [rows, n_out_s] or None (that stack costs nothing); returns dx [rows, n_in] summed over
        the stacks (None unless `want_dx`).  `grad`: a flat buffer with the arena's layout; stack s writes its part when bit s
        of `grad_mask` is set -- added to it with `accumulate`."""
        self._need_gpu()
        x = self._x(x)
        rows = x.shape[0]
        dys = [None if d is None else d.reshape(rows, -1).to(self.device, torch.float32).contiguous() for d in dys]
        for d, n in zip(dys, self.n_outs):
            assert d is None or d.shape == (rows, n), "dy must be [rows, n_out]"
        if grad is not None:
            assert grad.dtype == torch.float32 and grad.device == self.device and grad.is_contiguous() \
                and grad.numel() == self.arena_floats, "grad must have the arena's layout: %d floats" % self.arena_floats
        dx = torch.empty(rows, self.n_in, dtype=torch.float32, device=self.device) if want_dx else None
        ptrs = (C.c_void_p * _lib.FC_MAX_STACKS)(*[d.data_ptr() if d is not None else None for d in dys])
        _lib.check(self.lib.pvae_fc_backward(self.ctx, x.data_ptr(), rows, ptrs, dx.data_ptr() if dx is not None else None,
                                             grad.data_ptr() if grad is not None else None, int(grad_mask),
                                             1 if accumulate else 0, self._stream()), "pvae_fc_backward")
        return dx

    # -- PPO learner (engine_ppo.PpoSurface; include/pvae.h "PPO learner step", "Train-batch preparation") --------
    _PPO, _PPO_GAE_LAUNCHES = "pvae_fc_ppo_", "pvae_fc_gae_launches"

    def ppo_batch(self, batch, need_obs=True):
        """(pvae_fc_ppo_batch, the tensors it points to) from a dict of device tensors under the names of the loss's
        specification: obs, actions, old_dist, old_logp, advantages, value_targets, vf_preds."""
        return make_ppo_batch(batch, self.device, self.n_outs[0], self.n_in if need_obs else None)

    def launches(self):
        """(forward, backward): kernel launches of the last call of each kind."""
        f, b = C.c_int32(), C.c_int32()
        _lib.check(self.lib.pvae_fc_launches(self.ctx, C.byref(f), C.byref(b)), "pvae_fc_launches")
        return f.value, b.value


def set_fc_per_stack(on):
    """The stack set's launches one per stack instead of one per layer depth (process-wide; the A/B baseline of the grouping
    and a cross-check: both schedules give the same bits)."""
    lib = _lib.load()
    _lib.check(lib.pvae_set_option(None, b"fc_per_stack", 1 if on else 0), "pvae_set_option(fc_per_stack)")
