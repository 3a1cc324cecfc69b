"""The engines: the Python side of libpvae_gfx950.so.  They own the device buffers the C-ABI library works on and wrap its
calls.  PyTorch is used for what it is good at here: device memory, streams, `torch.save`.  All arithmetic of the hot path
happens in the library (physicsvae_amd/csrc).  Split by job:

    arch.py            Stack, Arch, TENSOR_IDS: the architecture description (no GPU needed)
    engine.py          (this file) HipEngine's core -- ctx lifetime, arena views, dataset binding, train step, infer,
                       net_forward / net_backward, reparam -- GraphedInfer, make_step_params, gemm_probe
    engine_dp.py       DataParallelExchange: comm_*, p2p_*, dp_train_step (the supervised trainer's exchange)
    engine_rollout.py  RolloutClient: infer_host and the rollout server's client
    engine_imagine.py  ImagineSurface: imagine, the H-step closed-loop unroll of policy and world model (pvae_imagine)
    engine_plan.py     PlanSurface: plan, sampled candidate codes over imagined rollouts (pvae_plan)
    engine_refine.py   RefineSurface: imagine_grad and refine, backpropagation through the unroll and Adam on the codes
                       (pvae_imagine_grad, pvae_plan_refine)
    engine_ppo.py      PpoSurface: the PPO learner surface both engines inherit, its struct builders, ppo_loss, gae, ppo_order
    stack_set.py       StackSetEngine, set_fc_per_stack

HipEngine = core + DataParallelExchange + RolloutClient + ImagineSurface + PlanSurface + RefineSurface + PpoSurface;
StackSetEngine = core + PpoSurface.  The first seven of the other modules stand on `_lib` and torch alone; every name that
was importable from here still is.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import FLAG_FUSED_ADAM, FLAG_NO_BACKWARD, NET_MD, NET_MH, NET_NAMES, NET_PR, NET_TE, NET_WM, NUM_NETS
from .arch import TENSOR_IDS, Arch, Stack                                                                  # noqa: F401
from .engine_dp import DataParallelExchange
from .engine_ppo import (PPO_COLUMNS, PpoSurface, evaluate_plan, gae, gae_scratch_for, make_act, make_ppo_batch,   # noqa: F401
                         make_prepared, make_rollout, ppo_loss, ppo_loss_diag, ppo_order, prepare_plan)
from .engine_imagine import ImagineSurface
from .engine_plan import PlanSurface
from .engine_refine import RefineSurface
from .engine_rollout import RolloutClient
from .stack_set import StackSetEngine, set_fc_per_stack                                                    # noqa: F401


class GraphedInfer:
    """`HipEngine.infer` captured once into a HIP graph.  The rollout forward at B = 1 is 8-10 tiny
    launches and host-bound (~33 us of Python + launch calls for ~15 us of GPU work); replaying the
    captured sequence is one host call.  Inputs and outputs live in static tensors: `__call__` copies
    the observation (and the draws, when the sampler is on) in and returns the static outputs
    (a_hat, s2_hat|None, z) -- valid until the next call.  The graph reads the parameter arena in
    place, so optimizer steps or load_state_dict between calls are seen by the next replay."""

    def __init__(self, engine, rows, want_s2=True, noise=False):
        engine._need_gpu()
        self.engine, self.rows, self.noise = engine, int(rows), bool(noise)
        dev = engine.device
        self.obs = torch.zeros(self.rows, 2 * engine.arch.Db, dtype=torch.float32, device=dev)
        self.eps = torch.zeros(self.rows, engine.arch.Z, dtype=torch.float32, device=dev) if noise else None
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                      # warm-up outside the capture (allocations, lazy init)
            self.out = engine.infer(self.obs, eps=self.eps, noise=self.noise, want_s2=want_s2)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self.out = engine.infer(self.obs, eps=self.eps, noise=self.noise, want_s2=want_s2, out=self.out)

    def __call__(self, obs, eps=None):
        # The captured launches write the staging panels that were current at capture time.  A
        # prefetched train step swaps the current and alternate panels, so after an odd number of them
        # those panels hold the NEXT training minibatch: tell the ctx that whatever is staged or
        # prefetched is gone (the next train step gathers again; pvae_infer does the same on the eager
        # path).  Host-side bookkeeping only, nothing is launched.
        self.engine.invalidate_staging()
        self.obs.copy_(obs.reshape(self.rows, -1), non_blocking=True)
        if self.noise:
            if eps is not None:
                self.eps.copy_(eps, non_blocking=True)
            else:
                self.eps.normal_()
        self.graph.replay()
        return self.out


def make_step_params(lr, adam_t=(1, 1, 1), a_rec=1.0, kl=1.0, s_rec=0.0, cyc=1e-3,
                     global_rows=0, seed=0, offset=0, beta1=0.9, beta2=0.999, eps=1e-8, loss="MSE",
                     weight_decay=0.0):
    sp = _lib.StepParams()
    sp.loss_kind = {"MSE": _lib.LOSS_MSE, "L1": _lib.LOSS_L1, "MAE": _lib.LOSS_L1}[loss]
    sp.a_rec_coeff, sp.kl_coeff, sp.s_rec_coeff, sp.cycle_coeff = a_rec, kl, s_rec, cyc
    sp.lr, sp.beta1, sp.beta2, sp.adam_eps = lr, beta1, beta2, eps
    for i in range(NUM_NETS):                      # (TE, MD, WM[, PR]); a missing entry counts as step 1
        sp.adam_t[i] = int(adam_t[i]) if i < len(adam_t) else 1
    sp.global_rows = int(global_rows)
    sp.rng_seed, sp.rng_offset = int(seed), int(offset)
    sp.weight_decay = float(weight_decay)
    return sp


class HipEngine(PpoSurface, DataParallelExchange, RolloutClient, ImagineSurface, PlanSurface, RefineSurface):
    def __init__(self, arch, max_batch, device="cuda", lookahead=1):
        self.lib = _lib.load()
        self.arch = arch
        self._ppo_dims = (2 * arch.Db, arch.Da, arch.Z)
        self.max_batch = int(max_batch)
        self.lookahead = int(lookahead)          # steps unrolled per sample (tpv:277, 367-428)
        # the library's <= 4-row rollout path: the LIBRARY's effective setting (it reads PVAE_ROLLOUT_FUSED once per
        # process), asked -- not re-read from the environment here, where the two could disagree
        self.fused_rollout = bool(self.lib.pvae_rollout_is_fused()) and arch.mh is None    # (helper models: staged path, pvae.hip infer_impl)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            # an indexed device, so that comparisons with tensor.device (always indexed) are exact
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self.cfg = arch.config(max_batch, self.lookahead)
        n = self.lib.pvae_arena_floats(C.byref(self.cfg))
        _lib.check(int(n), "pvae_arena_floats")
        self.arena_floats = int(n)
        self.layers = []
        info = _lib.LayerInfo()
        for i in range(_lib.check(self.lib.pvae_num_layers(C.byref(self.cfg)))):
            _lib.check(self.lib.pvae_layer(C.byref(self.cfg), i, C.byref(info)))
            self.layers.append({f: getattr(info, f) for f, _ in _lib.LayerInfo._fields_})
        self.segments = {}
        for net in (NET_TE, NET_MD, NET_WM, NET_PR, NET_MH):
            off, cnt = C.c_int64(), C.c_int64()
            _lib.check(self.lib.pvae_net_segment(C.byref(self.cfg), net, C.byref(off), C.byref(cnt)))
            self.segments[net] = (off.value, cnt.value)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.params = torch.zeros(self.arena_floats, **f32)
        self.grads = torch.zeros(self.arena_floats, **f32)
        self.exp_avg = torch.zeros(self.arena_floats, **f32)
        self.exp_avg_sq = torch.zeros(self.arena_floats, **f32)
        self.ctx = None
        self.has_comm = False                    # RCCL communicator owned by the ctx (comm_init)
        self.has_p2p = False                     # peers' arenas mapped into this process (p2p_open)
        self._srv_io = None                      # buffers of the rollout server's calls (rollout_server_start)
        self.exchange_code = _lib.EXCHANGE_ALLREDUCE   # what comm_mode last selected (p2p_close falls back to all-reduce)
        self.workspace = None
        self.dataset = None
        self._loss_scratch = None
        if self.device.type == "cuda":
            self._create_ctx()

    # -- lifetime -------------------------------------------------------------------
    def _create_ctx(self):
        ctx = C.c_void_p()
        _lib.check(self.lib.pvae_create(C.byref(self.cfg), C.byref(ctx)), "pvae_create")
        self.ctx = ctx
        nbytes = self.lib.pvae_workspace_bytes(C.byref(self.cfg))
        self.workspace = torch.zeros(nbytes // 4 + 64, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pvae_bind_arenas(ctx, self.params.data_ptr(), self.grads.data_ptr(),
                                             self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()))
        _lib.check(self.lib.pvae_bind_workspace(ctx, self.workspace.data_ptr(), nbytes))
        _lib.apply_context_options(self.lib, ctx)          # (PVAE_PAIR, PVAE_DIRECT, ...: the library reads no environment)
        self._loss_scratch = torch.zeros(5, dtype=torch.float32, device=self.device)

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.pvae_destroy(self.ctx)
                self.ctx = None
        except Exception:
            pass

    # -- parameter views (checkpoint layout, rmt:234-283) -------------------------------
    def _view(self, arena, info, kind):
        if kind == "weight":
            blk = arena[info["w_offset"]: info["w_offset"] + info["n_out_pad"] * info["ld"]]
            return blk.view(info["n_out_pad"], info["ld"])[: info["n_out"], info["col0"]: info["col0"] + info["n_in"]]
        return arena[info["b_offset"]: info["b_offset"] + info["n_out"]]

    def named_views(self, arena=None):
        """{'<net>._model.<i>._model.0.weight|bias': strided view into the arena}."""
        arena = self.params if arena is None else arena
        out = {}
        for info in self.layers:
            base = "%s._model.%d._model.0." % (NET_NAMES[info["net"]], info["index"])
            out[base + "weight"] = self._view(arena, info, "weight")
            out[base + "bias"] = self._view(arena, info, "bias")
        return out

    def segment(self, arena, nets):
        """Contiguous slice of `arena` covering the given nets (arena order TE | MD | PR | WM: the stacks
        trained together in the joint phase are adjacent)."""
        offs = sorted(self.segments[n] for n in nets if self.segments[n][1] > 0)
        lo = offs[0][0]
        hi = offs[-1][0] + offs[-1][1]
        assert sum(c for _, c in offs) == hi - lo, "nets are not adjacent in the arena"
        return arena[lo:hi]

    # -- data ---------------------------------------------------------------------------
    def bind_dataset(self, states, actions, window_row, next_states=None, check=True):
        """`next_states` (optional, row-aligned with `states`): what the second half of x / the target s2
        is read from instead of the next state row (cond "rel", tpv:149-150).  `check=False`: `window_row` is a
        permutation of a table that was checked when it was bound (a shuffled epoch): no read-back, no host sync."""
        self._need_gpu()
        if self.dataset is not None and self.dataset[0] is states and self.dataset[1] is actions \
                and self.dataset[2] is window_row and self.dataset[3] is next_states:
            return                                # the very same device tensors are already bound
        states = states.to(self.device, torch.float32).contiguous()
        actions = actions.to(self.device, torch.float32).contiguous()
        window_row = window_row.to(self.device, torch.int32).contiguous()
        assert states.shape[1] == self.arch.Db and actions.shape[1] == self.arch.Da
        if check:
            assert int(window_row.max()) + self.lookahead < states.shape[0] + (1 if next_states is not None else 0)
        if next_states is not None:
            next_states = next_states.to(self.device, torch.float32).contiguous()
            assert next_states.shape == states.shape
        self.dataset = (states, actions, window_row, next_states)
        _lib.check(self.lib.pvae_bind_dataset(self.ctx, states.data_ptr(), actions.data_ptr(),
                                              window_row.data_ptr(), states.shape[0],
                                              window_row.shape[0]), "pvae_bind_dataset")
        if next_states is not None:
            _lib.check(self.lib.pvae_bind_dataset_next(self.ctx, next_states.data_ptr()), "pvae_bind_dataset_next")

    def set_direct(self, on=True):
        """Training steps read the demonstration set where it lies (no staging launch; include/pvae.h pvae_set_direct).
        Opt-in (default off: every step stages its input panels first -- same bits, and faster at 256 rows per GPU)."""
        self._need_gpu()
        _lib.check(self.lib.pvae_set_direct(self.ctx, 1 if on else 0), "pvae_set_direct")

    def set_joint_s_rec(self, on=True):
        """The joint phase runs with `world_model_s_rec_coeff` != 0 (tpv:411-414 with the world model frozen; include/pvae.h
        pvae_set_option "joint_s_rec").  Opt-in: a context that was not told keeps refusing that combination."""
        self._need_gpu()
        _lib.check(self.lib.pvae_set_option(self.ctx, b"joint_s_rec", 1 if on else 0), "pvae_set_option(joint_s_rec)")

    def set_ppo_priors(self, on=True):
        """The fused PPO passes run under the learned prior ("normal_state_mean_one_std") and the sphere prior
        ("hypersphere_uniform") too (include/pvae.h pvae_set_option "ppo_priors"; the rules: `ppo.py`'s module docstring).
        Opt-in: a context that was not told keeps refusing those two priors."""
        self._need_gpu()
        _lib.check(self.lib.pvae_set_option(self.ctx, b"ppo_priors", 1 if on else 0), "pvae_set_option(ppo_priors)")

    def direct_active(self, phase, rows, sp, fused=True):
        """Would a training step with these arguments take the direct path?"""
        self._need_gpu()
        return bool(_lib.check(int(self.lib.pvae_direct_active(self.ctx, phase, int(rows), C.byref(sp), 1 if fused else 0))))

    def invalidate_staging(self):
        """Forget the staged / prefetched minibatch (something else is about to overwrite the panels)."""
        if self.ctx is not None:
            _lib.check(self.lib.pvae_invalidate_staging(self.ctx), "pvae_invalidate_staging")

    def gather(self, first_window, rows):
        self._need_gpu()
        _lib.check(self.lib.pvae_gather(self.ctx, int(first_window), int(rows), self._stream()),
                   "pvae_gather")

    def set_batch(self, x, y):
        """x [B, L, 2Db] (L == 1 may be squeezed), y [B, L, Da] -- tpv:365-376."""
        self._need_gpu()
        x = x.reshape(x.shape[0], -1).to(self.device, torch.float32).contiguous()
        assert x.shape[1] == self.lookahead * 2 * self.arch.Db, "x must be [B, lookahead, 2*Db]"
        yp = None
        if y is not None:
            y = y.reshape(y.shape[0], -1).to(self.device, torch.float32).contiguous()
            assert y.shape[1] == self.lookahead * self.arch.Da, "y must be [B, lookahead, Da]"
            yp = y.data_ptr()
        self._keep = (x, y)
        _lib.check(self.lib.pvae_set_batch(self.ctx, x.data_ptr(), yp, x.shape[0], self._stream()),
                   "pvae_set_batch")
        return x.shape[0]

    # -- compute ------------------------------------------------------------------------
    def forward_backward(self, phase, rows, sp, eps=None, fused_adam=False, backward=True,
                         loss_out=None):
        self._need_gpu()
        flags = (FLAG_FUSED_ADAM if fused_adam else 0) | (0 if backward else FLAG_NO_BACKWARD)
        if eps is not None:
            eps = self._eps(eps, rows)
        out = self._loss_scratch if loss_out is None else loss_out
        _lib.check(self.lib.pvae_forward_backward(
            self.ctx, phase, int(rows), C.byref(sp), eps.data_ptr() if eps is not None else None,
            out.data_ptr(), flags, self._stream()), "pvae_forward_backward")
        return out

    def _eps(self, eps, rows):
        """[rows, Z] (lookahead 1) or [lookahead, rows, Z]: one slice per unrolled step."""
        eps = eps.to(self.device, torch.float32).contiguous()
        want = (self.lookahead, rows, self.arch.Z)
        assert tuple(eps.shape) == want or (self.lookahead == 1 and tuple(eps.shape) == want[1:]), \
            "eps must be [lookahead, rows, Z]"
        self._keep_eps = eps
        return eps

    def forward_seed(self, phase, rows, sp, eps=None):
        self._need_gpu()
        if eps is not None:
            eps = self._eps(eps, rows)
        _lib.check(self.lib.pvae_forward_seed(self.ctx, phase, int(rows), C.byref(sp),
                                              eps.data_ptr() if eps is not None else None, self._stream()),
                   "pvae_forward_seed")

    def backward_stage(self, phase, rows, sp, stage, loss_out=None):
        """Launch `stage` of the backward pass.  Returns (grad_slice | None, net, n_stages): the
        slice of the gradient arena that is final after this stage."""
        self._need_gpu()
        off, cnt, net, n = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
        _lib.check(self.lib.pvae_backward_stage(
            self.ctx, phase, int(rows), C.byref(sp), int(stage),
            loss_out.data_ptr() if loss_out is not None else None, self._stream(),
            C.byref(off), C.byref(cnt), C.byref(net), C.byref(n)), "pvae_backward_stage")
        seg = (off.value, cnt.value) if cnt.value else None
        return seg, net.value, n.value

    def backward_plan(self, phase, sp):
        """[(net, offset, count)] per stage of the backward pass, in stage order (count 0: the stage finishes no slice);
        nothing is launched.  Independent of the minibatch's rows (`pvae_backward_plan`)."""
        self._need_gpu()
        n = C.c_int()
        cap = 128
        off, cnt, net = (C.c_int64 * cap)(), (C.c_int64 * cap)(), (C.c_int * cap)()
        _lib.check(self.lib.pvae_backward_plan(self.ctx, phase, C.byref(sp), off, cnt, net, cap, C.byref(n)), "pvae_backward_plan")
        assert n.value <= cap
        return [(net[k], off[k], cnt[k]) for k in range(n.value)]

    def adam_segment(self, net, off, cnt, sp):
        self._need_gpu()
        _lib.check(self.lib.pvae_adam_segment(self.ctx, int(net), int(off), int(cnt), C.byref(sp), self._stream()),
                   "pvae_adam_segment")

    def adam(self, nets, sp):
        self._need_gpu()
        mask = 0
        for n in nets:
            mask |= 1 << n
        _lib.check(self.lib.pvae_adam(self.ctx, mask, C.byref(sp), self._stream()), "pvae_adam")

    def train_step(self, phase, first_window, rows, sp, eps=None, loss_out=None, next_span=None):
        """One fused optimizer step; `next_span` = (first_window, rows) of the minibatch that follows
        lets the library gather it inside this step's last launch (pvae_train_step_prefetch)."""
        self._need_gpu()
        if eps is not None:
            eps = self._eps(eps, rows)
        out = self._loss_scratch if loss_out is None else loss_out
        if next_span is not None:
            _lib.check(self.lib.pvae_train_step_prefetch(
                self.ctx, phase, int(first_window), int(rows), C.byref(sp),
                eps.data_ptr() if eps is not None else None, out.data_ptr(), int(next_span[0]), int(next_span[1]),
                self._stream()), "pvae_train_step_prefetch")
            return out
        _lib.check(self.lib.pvae_train_step(
            self.ctx, phase, int(first_window), int(rows), C.byref(sp),
            eps.data_ptr() if eps is not None else None, out.data_ptr(), self._stream()),
            "pvae_train_step")
        return out

    def read(self, name, rows, step=0):
        """Forward intermediate of time step `step` of the last batch."""
        self._need_gpu()
        width = {"mu": self.arch.Z, "logvar": self.arch.Z, "z": self.arch.Z, "eps": self.arch.Z,
                 "prior_mu": self.arch.Z, "a_hat": self.arch.Da, "s2_hat": self.arch.Db}[name]
        dst = torch.empty(rows, width, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pvae_read_tensor(self.ctx, TENSOR_IDS[name] + 8 * int(step), dst.data_ptr(), rows,
                                             self._stream()), "pvae_read_tensor")
        return dst

    def infer(self, obs, eps=None, noise=True, seed=0, offset=0, want_s2=True, out=None):
        """rmt:742-771 forward at rollout batch sizes: returns (a_hat, s2_hat|None, z).
        `out` = a tuple returned by an earlier call with the same row count: its tensors are
        overwritten instead of allocating new ones (the 30 Hz control loop calls this every step; at
        B = 1 the host side of the call costs as much as the GPU side)."""
        self._need_gpu()
        if not (obs.dtype == torch.float32 and obs.device == self.device and obs.dim() == 2 and obs.is_contiguous()):
            obs = obs.reshape(obs.shape[0], -1).to(self.device, torch.float32).contiguous()
        rows = obs.shape[0]
        if out is not None and out[0].shape[0] == rows and (out[1] is not None) == bool(want_s2):
            a_hat, s2, z = out
        else:
            a_hat = torch.empty(rows, self.arch.Da, dtype=torch.float32, device=self.device)
            s2 = torch.empty(rows, self.arch.Db, dtype=torch.float32, device=self.device) if want_s2 else None
            z = torch.empty(rows, self.arch.Z, dtype=torch.float32, device=self.device)
        if eps is not None:
            eps = eps.to(self.device, torch.float32).contiguous()
        _lib.check(self.lib.pvae_infer(
            self.ctx, obs.data_ptr(), rows, eps.data_ptr() if eps is not None else None,
            1 if noise else 0, int(seed), int(offset), a_hat.data_ptr(),
            s2.data_ptr() if s2 is not None else None, z.data_ptr(), self._stream()), "pvae_infer")
        return a_hat, s2, z

    def infer_logits(self, obs, log_std, eps=None, noise=True, seed=0, offset=0, want_s2=True):
        """`infer` with the module's output layout: returns (logits [rows, 2 Da] = [a_hat | log_std], s2_hat|None, z)
        -- the decoder's log-std vector (device tensor [Da]) is appended by the launch that writes the action
        (AppendLogStd, rmt:160-206), so `PhysicsVAE.forward` needs no concatenation of its own."""
        self._need_gpu()
        if not (obs.dtype == torch.float32 and obs.device == self.device and obs.dim() == 2 and obs.is_contiguous()):
            obs = obs.reshape(obs.shape[0], -1).to(self.device, torch.float32).contiguous()
        rows, Da = obs.shape[0], self.arch.Da
        logits = torch.empty(rows, 2 * Da, dtype=torch.float32, device=self.device)
        s2 = torch.empty(rows, self.arch.Db, dtype=torch.float32, device=self.device) if want_s2 else None
        z = torch.empty(rows, self.arch.Z, dtype=torch.float32, device=self.device)
        if eps is not None:
            eps = eps.to(self.device, torch.float32).contiguous()
        _lib.check(self.lib.pvae_infer_logits(
            self.ctx, obs.data_ptr(), rows, eps.data_ptr() if eps is not None else None,
            1 if noise else 0, int(seed), int(offset), logits.data_ptr(), 2 * Da, log_std.data_ptr(),
            s2.data_ptr() if s2 is not None else None, z.data_ptr(), self._stream()), "pvae_infer_logits")
        return logits, s2, z

    def mlp_forward(self, x, layers, act="relu", out_act=None):
        """A stack of Linear layers on caller-owned dense weights: `layers` = [(weight [n_out, n_in], bias)], hidden
        activation `act` (one name, or one per hidden layer), output layer linear or `out_act` (`pvae_mlp_forward`; the
        rollout model's value branch, rmt:846-853, and the motor decoder's helper, rmt:833-835)."""
        self._need_gpu()
        x = x.reshape(x.shape[0], -1).to(self.device, torch.float32)
        if x.stride(-1) != 1:
            x = x.contiguous()
        n = len(layers)
        acts = [act] * (n - 1) if isinstance(act, str) else ["linear" if a is None else a for a in act]
        assert len(acts) == n - 1, "one activation per hidden layer"
        key = tuple((w.data_ptr(), b.data_ptr(), w.stride(0)) for w, b in layers) + (tuple(acts),)
        plans = self.__dict__.setdefault("_mlp_plans", {})
        plan = plans.get(key)
        if plan is None:                                # pointer tables are rebuilt only when a tensor moved
            Pf = C.c_void_p * n
            Ii = C.c_int32 * n
            for w, b in layers:
                assert w.dtype == torch.float32 and w.device == self.device and w.stride(1) == 1 and b.is_contiguous()
            plan = (key, Pf(*[w.data_ptr() for w, _ in layers]), Pf(*[b.data_ptr() for _, b in layers]),
                    Ii(*[w.shape[1] for w, _ in layers]), Ii(*[w.shape[0] for w, _ in layers]),
                    Ii(*[w.stride(0) for w, _ in layers]), max([w.shape[0] for w, _ in layers[:-1]] or [1]),
                    (C.c_int32 * max(n - 1, 1))(*[_lib.LAYER_ACTS[a] for a in acts]))
            if len(plans) > 8:
                plans.clear()
            plans[key] = plan
        rows = x.shape[0]
        scratch = torch.empty(2 * rows * plan[6], dtype=torch.float32, device=self.device)
        out = torch.empty(rows, layers[-1][0].shape[0], dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pvae_mlp_forward(x.data_ptr(), rows, x.stride(0), n, plan[1], plan[2], plan[3], plan[4], plan[5],
                                             0 if out_act in (None, "linear") else (1 + _lib.LAYER_ACTS[out_act]) << 8,
                                             plan[7], scratch.data_ptr(), out.data_ptr(), out.shape[1],
                                             self._stream()), "pvae_mlp_forward")
        return out

    def graphed_infer(self, rows, want_s2=True, noise=False):
        """The rollout forward for a fixed row count as ONE replayable HIP graph (see GraphedInfer)."""
        return GraphedInfer(self, rows, want_s2=want_s2, noise=noise)

    def panel(self, kind, net=0, layer=0):
        """Workspace panel as a [Bp, width] view (inspection / tests).  kind: 'in', 'd_in',
        'act', 'dz', 's2', 'act_t', 'eps'."""
        kinds = {"in": 0, "d_in": 1, "act": 2, "dz": 3, "s2": 4, "act_t": 5, "eps": 6}
        off = _lib.check(int(self.lib.pvae_workspace_offset(C.byref(self.cfg), kinds[kind], net, layer)))
        bp = (self.max_batch + 31) // 32 * 32
        lays = [l for l in self.layers if l["net"] == net]
        pad64 = lambda v: (v + 63) // 64 * 64
        width = {"in": lays[0]["ld"], "d_in": lays[0]["ld"], "act": lays[layer]["n_out_pad"],
                 "dz": lays[layer]["n_out_pad"], "s2": pad64(self.arch.Db), "act_t": pad64(self.arch.Da),
                 "eps": self.arch.Z}[kind]
        return self.workspace[off: off + bp * width].view(bp, width)

    def kept_obs(self, rows):
        """The library's own copy of the observation rows of the last rollout call with <= 4 rows (workspace kind 7):
        a [rows, 2 Db] view that stays valid until the next such call, whatever the caller does with its buffer."""
        off = getattr(self, "_obs_keep_off", None)
        if off is None:
            off = self._obs_keep_off = _lib.check(int(self.lib.pvae_workspace_offset(C.byref(self.cfg), 7, 0, 0)))
        w = 2 * self.arch.Db
        return self.workspace[off: off + rows * w].view(rows, w)

    def net_in_width(self, net):
        """Columns of the dense input `net_forward` / `net_backward` read per row: the stack's full input width (a first layer
        on an input subset reads its window of it, include/pvae.h pvae_config.te_inputs)."""
        a = self.arch
        return {NET_TE: 2 * a.Db, NET_MD: a.Db + a.Z, NET_MH: a.Db + a.Z, NET_WM: a.Db + a.Da, NET_PR: a.Db}[net]

    def net_forward(self, net, x):
        self._need_gpu()
        x = x.reshape(x.shape[0], -1).to(self.device, torch.float32).contiguous()
        assert x.shape[1] == self.net_in_width(net), \
            "x must be [rows, %d] (the stack's full input width), got %s" % (self.net_in_width(net), tuple(x.shape))
        n_out = [l for l in self.layers if l["net"] == net][-1]["n_out"]
        out = torch.empty(x.shape[0], n_out, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pvae_net_forward(self.ctx, net, x.data_ptr(), x.shape[0], out.data_ptr(),
                                             self._stream()), "pvae_net_forward")
        return out

    def net_backward(self, net, x, dy, want_dx, grad=None, accumulate=False):
        """Backward of one arena stack (`pvae_net_backward`): `x` [rows, n_in] as `net_forward` took it, `dy` [rows, n_out] =
        dL/d(output).  Returns dx [rows, n_in] (None unless `want_dx`).  `grad`: a flat buffer of the stack's segment
        (`segments[net]` count floats, arena layout) that receives the parameter gradient -- added to it with `accumulate`;
        None: input gradient only.  At most `max_batch` rows; the forward is recomputed inside the call."""
        self._need_gpu()
        x = x.reshape(x.shape[0], -1).to(self.device, torch.float32).contiguous()
        dy = dy.reshape(dy.shape[0], -1).to(self.device, torch.float32).contiguous()
        rows = x.shape[0]
        lays = [l for l in self.layers if l["net"] == net]
        n_in = self.net_in_width(net)
        assert x.shape[1] == n_in, "x must be [rows, %d] (the stack's full input width), got %s" % (n_in, tuple(x.shape))
        assert dy.shape == (rows, lays[-1]["n_out"]), "dy must be [rows, n_out]"
        if grad is not None:
            assert grad.dtype == torch.float32 and grad.device == self.device and grad.is_contiguous() \
                and grad.numel() == self.segments[net][1], "grad must be the stack's segment: %d floats" % self.segments[net][1]
        dx = torch.empty(rows, n_in, dtype=torch.float32, device=self.device) if want_dx else None
        _lib.check(self.lib.pvae_net_backward(self.ctx, net, x.data_ptr(), rows, dy.data_ptr(),
                                              dx.data_ptr() if dx is not None else None,
                                              grad.data_ptr() if grad is not None else None, 1 if accumulate else 0,
                                              self._stream()), "pvae_net_backward")
        return dx

    def reparam_backward(self, mu_logvar, eps_used, dz, noise=True):
        """Backward of `reparam` (`pvae_reparam_backward`): d(mu_logvar) from dz [rows, Z], the draws the forward used
        (`eps_used` [rows, Z], None without noise or on the unit-sphere / no-prior encoders) and its mu_logvar."""
        self._need_gpu()
        ml = mu_logvar.to(self.device, torch.float32).contiguous()
        dz = dz.to(self.device, torch.float32).contiguous()
        out = torch.empty_like(ml)
        if eps_used is not None:
            eps_used = eps_used.to(self.device, torch.float32).contiguous()
        _lib.check(self.lib.pvae_reparam_backward(self.ctx, ml.data_ptr(), eps_used.data_ptr() if eps_used is not None else None,
                                                  dz.data_ptr(), ml.shape[0], 1 if noise else 0, out.data_ptr(),
                                                  self._stream()), "pvae_reparam_backward")
        return out

    def reparam(self, mu_logvar, eps=None, noise=True, seed=0, offset=0):
        self._need_gpu()
        ml = mu_logvar.to(self.device, torch.float32).contiguous()
        z = torch.empty(ml.shape[0], self.arch.Z, dtype=torch.float32, device=self.device)
        if eps is not None:
            eps = eps.to(self.device, torch.float32).contiguous()
        _lib.check(self.lib.pvae_reparam(self.ctx, ml.data_ptr(), ml.shape[0],
                                         eps.data_ptr() if eps is not None else None,
                                         1 if noise else 0, int(seed), int(offset), z.data_ptr(),
                                         self._stream()), "pvae_reparam")
        return z

    # -- PPO learner (engine_ppo.PpoSurface): what PhysicsVAE's calls add -- the value engine and the latent draws ----
    _PPO, _PPO_GAE_LAUNCHES, _PPO_NEEDS_LOG_STD = "pvae_ppo_", "pvae_ppo_gae_launches", True

    def ppo_batch(self, batch):
        """(pvae_fc_ppo_batch, the tensors it points to) from a dict of device tensors under the names of the loss's
        specification; obs is [n, 2 Db]."""
        return make_ppo_batch(batch, self.device, self.arch.Da, 2 * self.arch.Db)

    def _ppo_eps(self, eps, shape):
        if eps is None:
            return None
        eps = eps.to(self.device, torch.float32).contiguous()
        assert tuple(eps.shape) == shape, "eps must be %s, got %s" % (shape, tuple(eps.shape))
        return eps

    def _ppo_inline_draws(self, draws, lead):
        """`draws` = (eps [*lead, Z] or None: Philox at (seed, offset), noise, seed, offset), passed as four arguments."""
        eps, noise, seed, offset = draws
        eps = self._ppo_eps(eps, lead + (self.arch.Z,))
        return eps, (eps.data_ptr() if eps is not None else None, 1 if noise else 0, int(seed), int(offset))

    def _ppo_struct_draws(self, draws, n, out=None, want=False, used=None):
        """`draws` as above with eps [n, Z], passed as a pvae_ppo_draws; `want`: the rows are evaluated, so the draws used
        are written to out["latent_eps"] (allocated when not given); `used`: the tensor that receives them otherwise."""
        eps, noise, seed, offset = draws
        d = _lib.PpoDraws()
        eps = self._ppo_eps(eps, (n, self.arch.Z))
        if want:
            used = (out or {}).get("latent_eps")
            if used is None:
                used = torch.empty(n, self.arch.Z, dtype=torch.float32, device=self.device)
            assert used.dtype == torch.float32 and used.device == self.device and used.is_contiguous() \
                and tuple(used.shape) == (n, self.arch.Z), "out['latent_eps'] must be contiguous float32 [%d, %d]" % (n, self.arch.Z)
        if used is not None:
            d.eps_out = used.data_ptr()
        d.eps = eps.data_ptr() if eps is not None else None
        d.noise, d.rng_seed, d.rng_offset = 1 if noise else 0, int(seed), int(offset)
        return eps, (C.byref(d),), used

    def ppo_bind(self, value_engine, log_std, train_log_std=False):
        """`PpoSurface.ppo_bind` -- the buffers have the parameter arena's layout and are the PPO step's own, not the
        supervised trainer's `grads` / `exp_avg` / `exp_avg_sq`; log_std is Da contiguous floats on the device -- together
        with the one-stack `StackSetEngine` that carries the value branch (bound with it, kept alive while bound)."""
        return self._ppo_bind(log_std, train_log_std, value_engine)

    def ppo_step(self, batch, params, first, rows, index=None, eps=None, noise=True, seed=0, offset=0, stats_out=None):
        """`PpoSurface.ppo_step` with the latent draws: `eps` [rows, Z] or None (Philox at (seed, offset))."""
        return self._ppo_step(batch, params, first, rows, index, stats_out, (eps, noise, seed, offset))

    def ppo_sgd(self, batch, params, minibatch, num_sgd_iter, perm=None, eps=None, noise=True, seed=0, offset=0):
        """`PpoSurface.ppo_sgd` with the latent draws: step i uses `eps[i]` (eps [steps, minibatch, Z]) or Philox offset
        `offset + i`, and Adam time step `params.adam_t + i`."""
        return self._ppo_sgd(batch, params, minibatch, num_sgd_iter, perm, (eps, noise, seed, offset))

    def ppo_grad_step(self, batch, params, first, rows, index=None, eps=None, noise=True, seed=0, offset=0, stats_out=None):
        """`PpoSurface.ppo_grad_step` with the latent draws of `ppo_step`; the value branch's gradient lies in the value
        engine's `ppo_grad`."""
        return self._ppo_step(batch, params, first, rows, index, stats_out, (eps, noise, seed, offset), grad=True)

    def ppo_evaluate(self, rollout, params, eps=None, noise=True, seed=0, offset=0, out=None):
        """`PpoSurface.ppo_evaluate`, and latent_eps [N, Z], the draws used (when the rollout has obs and actions).  `eps`
        [N, Z]: the draws, row by row (None: Philox, chunk i at (seed, offset + i)); `noise` False: z = mu."""
        return self._ppo_evaluate(rollout, params, out, (eps, noise, seed, offset))

    def ppo_prepare(self, rollout, params, eps=None, noise=True, seed=0, offset=0, out=None):
        """`PpoSurface.ppo_prepare`, and latent_eps (None when the sampler's columns are given: nothing was drawn).  Draws
        as `ppo_evaluate`."""
        return self._ppo_prepare(rollout, params, out, (eps, noise, seed, offset))

    def ppo_act(self, obs, params, explore=True, noise=None, clip=None, eps=None, latent_noise=True, seed=0, offset=0,
                out=None, out_row=None):
        """`PpoSurface.ppo_act`, and latent_eps [., Z], the latent draws used.  `eps` [n, Z] / `latent_noise`: the latent
        draws as `ppo_evaluate` takes them; the action noise and the latent draws share (seed, offset + chunk)."""
        return self._ppo_act(obs, params, explore, noise, clip, seed, offset, out, out_row, (eps, latent_noise, seed, offset))


def gemm_probe(kind, a, b, c, bias_or_mask=None, relu=False, m=0, n=0, k=0):
    """Kernel-level entry (tests / roofline probes).  Tensors are dense fp32 on the GPU."""
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.pvae_gemm_probe(
        kind, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0),
        bias_or_mask.data_ptr() if bias_or_mask is not None else None,
        bias_or_mask.stride(0) if (bias_or_mask is not None and bias_or_mask.dim() == 2) else 0,
        m, n, k, 1 if relu else 0, st), "pvae_gemm_probe")
    return c
