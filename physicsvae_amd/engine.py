"""HipEngine -- owns the device buffers the C-ABI library works on and wraps its calls.

PyTorch is used for what it is good at here: device memory, streams, `torch.save`.  All
arithmetic of the hot path happens in libpvae_gfx950.so (physicsvae_amd/csrc).
"""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import ACT_KINDS, FLAG_FUSED_ADAM, FLAG_NO_BACKWARD, NET_MD, NET_MH, NET_NAMES, NET_PR, NET_TE, NET_WM, NUM_NETS, PRIOR_KINDS

TENSOR_IDS = {"mu": 0, "logvar": 1, "z": 2, "a_hat": 3, "s2_hat": 4, "eps": 5, "prior_mu": 6}


class Stack:
    """Hidden layers of one FC stack as `FC.__init__` accepts them (rmt:234-270): a width and an activation per
    layer ("linear" / None: none).  `gen_layers(width, depth)` (tpv:180-192) is the special case one width, one
    activation; `Stack.of((width, depth), act)` builds that."""

    def __init__(self, widths, acts="relu"):
        self.widths = tuple(int(w) for w in widths)
        if isinstance(acts, str) or acts is None:
            acts = [acts] * len(self.widths)
        self.acts = tuple("linear" if a is None else a for a in acts)
        if not self.widths or len(self.widths) > _lib.MAX_HIDDEN or min(self.widths) < 1:
            raise NotImplementedError("a stack needs 1..%d hidden layers of positive width, got %s" % (_lib.MAX_HIDDEN, self.widths))
        if len(self.acts) != len(self.widths):
            raise ValueError("one activation per hidden layer: %s vs %s" % (self.acts, self.widths))
        for a in self.acts:                      # "swish"/"silu": ray's Swish module (learnable beta), not offered
            if a not in _lib.LAYER_ACTS:
                raise NotImplementedError("hidden activation %r: the HIP path offers %s" % (a, sorted(_lib.LAYER_ACTS)))

    @classmethod
    def of(cls, spec, act="relu"):
        if isinstance(spec, Stack):
            return spec
        width, depth = spec
        return cls([width] * int(depth), act)

    def uniform(self, act):
        return len(set(self.widths)) == 1 and set(self.acts) == {act}

    def key(self):
        return (self.widths, self.acts)

    # (width, depth) of the first layer: what the uniform fields of pvae_config carry
    def __getitem__(self, i):
        return (self.widths[0], len(self.widths))[i]

    def __iter__(self):
        return iter((self.widths[0], len(self.widths)))


class Arch:
    """Dims of the trainable stacks (tpv:247-286 keys, gen_layers tpv:180-192).  `te` / `md` / `wm` / `pr`:
    (width, depth) with the one hidden activation `act` (everything the trainer can generate), or a `Stack`
    (per-layer widths and activations, what custom_model_config's *_layers can describe, rmt:462-510)."""

    def __init__(self, dim_body, dim_action, latent, te, md, wm, prior="normal_zero_mean_one_std", pr=None,
                 act="relu", te_inputs=("body", "task"), md_inputs=("body", "task"), mh=None, mh_range=0.5):
        self.Db, self.Da, self.Z = int(dim_body), int(dim_action), int(latent)
        # task_encoder_inputs / motor_decoder_inputs (rmt:470, 485): column windows of the full-width first layers
        self.te_inputs, self.md_inputs = tuple(te_inputs), tuple(md_inputs)
        for name, v in (("task_encoder_inputs", self.te_inputs), ("motor_decoder_inputs", self.md_inputs)):
            if v not in _lib.INPUT_BITS:
                raise NotImplementedError("%s = %r: a non-empty subset of ['body', 'task'], in that order" % (name, list(v)))
        if prior not in PRIOR_KINDS:
            raise NotImplementedError("Unknown latent_prior_type:%s" % (prior,))      # rmt:624-625
        self.prior = prior                       # latent_prior_type (rmt:614-635; oracle/refpath.py PRIORS)
        if act not in ACT_KINDS:                 # "swish"/"silu": ray's Swish module (learnable beta), not offered
            raise NotImplementedError("hidden activation %r: the HIP path offers %s" % (act, sorted(ACT_KINDS)))
        self.act = act                           # the trainer's "act_fn" (tpv:262): the default of every stack
        self.te, self.md, self.wm = Stack.of(te, act), Stack.of(md, act), Stack.of(wm, act)
        self.pr = Stack.of(pr, act) if pr is not None else self.te      # learned prior stack
        # the motor decoder's helper (rmt:490-498, 670-680): hidden layers `mh` (None: no helper), tanh output x mh_range
        self.mh = Stack.of(mh, act) if mh is not None else None
        self.mh_range = float(mh_range)
        if self.mh is not None and not self.mh_range > 0:
            raise AssertionError("motor_decoder_helper_range must be positive (rmt:673)")

    @property
    def te_out(self):
        return self.Z if (self.prior == "hypersphere_uniform" or self.prior is False) else 2 * self.Z   # rmt:618-623

    def config(self, max_batch, lookahead=1):
        cfg = _lib.Config(self.Db, self.Da, self.Z, self.te[0], self.te[1], self.md[0],
                          self.md[1], self.wm[0], self.wm[1], int(max_batch), int(lookahead),
                          PRIOR_KINDS[self.prior], self.pr[0], self.pr[1], ACT_KINDS[self.act])
        if self.mh is not None:
            cfg.mh_width, cfg.mh_depth, cfg.mh_range = self.mh[0], self.mh[1], self.mh_range
        for net, st in ((NET_TE, self.te), (NET_MD, self.md), (NET_WM, self.wm), (NET_PR, self.pr), (NET_MH, self.mh)):
            if st is None or st.uniform(self.act):             # (a zeroed row: the uniform stack the scalar fields describe)
                continue
            for i, (w, a) in enumerate(zip(st.widths, st.acts)):
                cfg.layer_width[net][i] = w
                cfg.layer_act[net][i] = 1 + _lib.LAYER_ACTS[a]
        cfg.te_inputs, cfg.md_inputs = _lib.INPUT_BITS[self.te_inputs], _lib.INPUT_BITS[self.md_inputs]
        return cfg

    def key(self):
        return (self.Db, self.Da, self.Z, self.te.key(), self.md.key(), self.wm.key(), self.prior, self.pr.key(), self.act,
                self.te_inputs, self.md_inputs, self.mh.key() if self.mh is not None else None, self.mh_range)


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


class HipEngine:
    def __init__(self, arch, max_batch, device="cuda", lookahead=1):
        self.lib = _lib.load()
        self.arch = arch
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

    def _need_gpu(self):
        if self.ctx is None:
            raise RuntimeError("HipEngine was created on %s: the HIP hot path needs a GPU "
                               "(there is no CPU fallback)" % self.device)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

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

    @property
    def in_library_exchange(self):
        """`dp_train_step` can run: the ctx has an RCCL communicator or its peers' arenas are mapped."""
        return self.has_comm or self.has_p2p

    # -- data-parallel exchange inside the library (RCCL) ----------------------------------------
    def comm_unique_id(self):
        buf = C.create_string_buffer(128)
        _lib.check(self.lib.pvae_comm_unique_id(buf), "pvae_comm_unique_id")
        return buf.raw

    def comm_init(self, rank, world, unique_id):
        self._need_gpu()
        assert len(unique_id) == 128
        _lib.check(self.lib.pvae_comm_init(self.ctx, int(rank), int(world), C.c_char_p(unique_id)), "pvae_comm_init")
        self.has_comm = True
        self._dp_env()

    def _dp_env(self):
        """PVAE_DP_BUCKET_MB / PVAE_DP_SHARDED / PVAE_P2P_TIMEOUT_MS of the environment, applied through the ABI (the
        library reads no environment variable)."""
        if "PVAE_DP_BUCKET_MB" in os.environ:
            self.comm_config(float(os.environ["PVAE_DP_BUCKET_MB"]))
        if self.has_comm and not self.has_p2p and "PVAE_DP_SHARDED" in os.environ:
            self.comm_mode(os.environ["PVAE_DP_SHARDED"][:1] == "1")
        if "PVAE_P2P_TIMEOUT_MS" in os.environ:
            _lib.check(self.lib.pvae_set_option(self.ctx, b"p2p_timeout_ms", int(os.environ["PVAE_P2P_TIMEOUT_MS"])))

    def comm_destroy(self):
        if self.ctx is not None and self.has_comm:
            _lib.check(self.lib.pvae_comm_destroy(self.ctx), "pvae_comm_destroy")
            self.has_comm = False

    def comm_info(self):
        """(rank, nranks) as the ctx's RCCL communicator reports them; (0, 0) without one."""
        r, n = C.c_int(), C.c_int()
        if self.ctx is None:
            return 0, 0
        _lib.check(self.lib.pvae_comm_info(self.ctx, C.byref(r), C.byref(n)), "pvae_comm_info")
        return r.value, n.value

    def comm_config(self, bucket_mb=0.0, test_delay_us=0):
        """Exchange settings of dp_train_step: bucket size in MiB (0, the default: one in-line
        reduction per stack; > 0: bucketed and overlapped on the library's exchange stream, see
        include/pvae.h) and, for ordering tests, a delay in front of every reduction."""
        _lib.check(self.lib.pvae_comm_config(self.ctx, int(bucket_mb * (1 << 20)), int(test_delay_us)), "pvae_comm_config")

    def comm_mode(self, mode):
        """Exchange form of dp_train_step (include/pvae.h): "allreduce" (False) = all-reduce + replicated Adam,
        "sharded" (True) = reduce-scatter -> Adam on the owned 1/N slice -> all-gather of the parameters, "p2p" /
        "p2p_push" = the same shape as ONE launch over peer-mapped arenas, no RCCL (needs p2p_open; pull: owners read
        their slice from the peers' arenas, push: every rank writes its contributions into the owners' staging)."""
        code = {False: _lib.EXCHANGE_ALLREDUCE, True: _lib.EXCHANGE_SHARDED, "allreduce": _lib.EXCHANGE_ALLREDUCE,
                "sharded": _lib.EXCHANGE_SHARDED, "p2p": _lib.EXCHANGE_P2P, "p2p_push": _lib.EXCHANGE_P2P_PUSH,
                "local": _lib.EXCHANGE_LOCAL}[mode]
        _lib.check(self.lib.pvae_comm_mode(self.ctx, code), "pvae_comm_mode")
        self.exchange_code = code

    @property
    def p2p_active(self):
        """The peer-mapped exchange is what dp_train_step runs (its peers are mapped AND one of its forms is selected)."""
        return self.has_p2p and self.exchange_code in (_lib.EXCHANGE_P2P, _lib.EXCHANGE_P2P_PUSH)

    # -- peer-mapped exchange (PVAE_EXCHANGE_P2P) -------------------------------------------------
    def p2p_export(self):
        """This rank's 256-byte description of its gradient / parameter arenas and flag block (IPC handles)."""
        self._need_gpu()
        buf = C.create_string_buffer(_lib.P2P_BLOB_BYTES)
        _lib.check(self.lib.pvae_p2p_export(self.ctx, buf), "pvae_p2p_export")
        return buf.raw

    def p2p_open(self, rank, world, blobs):
        """Map every peer's buffers (`blobs`: the exports of ranks 0 .. world-1 in rank order)."""
        self._need_gpu()
        assert len(blobs) == world and all(len(b) == _lib.P2P_BLOB_BYTES for b in blobs)
        if "PVAE_P2P_SELFTEST_FLAGS_ONLY" in os.environ:
            _lib.check(self.lib.pvae_set_option(self.ctx, b"p2p_selftest_flags_only", 1))
        _lib.check(self.lib.pvae_p2p_open(self.ctx, int(rank), int(world), C.c_char_p(b"".join(blobs))), "pvae_p2p_open")
        self.has_p2p = True
        self._dp_env()

    def p2p_exchange(self, net, off, cnt, sp):
        """One slice of the gradient arena through the peer-mapped exchange (sum over the ranks by the slice owners,
        Adam, updated parameters to every rank); every rank issues the same calls."""
        self._need_gpu()
        _lib.check(self.lib.pvae_p2p_exchange(self.ctx, int(net), int(off), int(cnt), C.byref(sp), self._stream()),
                   "pvae_p2p_exchange")

    def p2p_selftest(self):
        """Prove remote write, remote read and flag delivery between all mapped peers (every rank calls it)."""
        self._need_gpu()
        _lib.check(self.lib.pvae_p2p_selftest(self.ctx, self._stream()), "pvae_p2p_selftest")

    def p2p_clear_errors(self):
        """Zero the time-out count `p2p_status` reports (the caller has dealt with them: candidate dropped, snapshot restored)."""
        if self.ctx is not None:
            _lib.check(self.lib.pvae_p2p_clear_errors(self.ctx, self._stream()), "pvae_p2p_clear_errors")

    def p2p_close(self):
        if self.ctx is not None and self.has_p2p:
            _lib.check(self.lib.pvae_p2p_close(self.ctx), "pvae_p2p_close")
            self.has_p2p = False
            if self.exchange_code in (_lib.EXCHANGE_P2P, _lib.EXCHANGE_P2P_PUSH):
                self.exchange_code = _lib.EXCHANGE_ALLREDUCE          # (what the library falls back to)

    def p2p_status(self, sync=True):
        """(rank, world, waits that gave up).  world = 0: not open.  `sync`: read the time-out word (synchronises)."""
        r, n, t = C.c_int(), C.c_int(), C.c_uint32()
        if self.ctx is None:
            return 0, 0, 0
        _lib.check(self.lib.pvae_p2p_status(self.ctx, C.byref(r), C.byref(n), C.byref(t) if sync else None,
                                            self._stream()), "pvae_p2p_status")
        return r.value, n.value, t.value

    def owned_slices(self, phase, net):
        """[(offset, count, replicated)]: the arena ranges of stack `net` (trained in `phase`) for which this rank holds
        valid Adam moments under the current exchange mode (include/pvae.h pvae_owned_slices)."""
        n, cap = C.c_int32(), 64
        off, cnt, rep = (C.c_int64 * cap)(), (C.c_int64 * cap)(), (C.c_int32 * cap)()
        _lib.check(self.lib.pvae_owned_slices(self.ctx, int(phase), int(net), off, cnt, rep, cap, C.byref(n)), "pvae_owned_slices")
        return [(off[i], cnt[i], bool(rep[i])) for i in range(n.value)]

    def allreduce_grads(self, off, cnt):
        self._need_gpu()
        _lib.check(self.lib.pvae_allreduce_grads(self.ctx, int(off), int(cnt), self._stream()), "pvae_allreduce_grads")

    def dp_train_step(self, phase, first_window, rows, sp, eps=None, loss_out=None, next_span=None):
        self._need_gpu()
        nf, nr = (int(next_span[0]), int(next_span[1])) if next_span is not None else (0, 0)
        if eps is not None and rows:
            eps = self._eps(eps, rows)
        out = self._loss_scratch if loss_out is None else loss_out
        _lib.check(self.lib.pvae_dp_train_step(
            self.ctx, phase, int(first_window), int(rows), C.byref(sp),
            eps.data_ptr() if (eps is not None and rows) else None, out.data_ptr(), nf, nr, self._stream()),
            "pvae_dp_train_step")
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

    def infer_host(self, obs, noise=True, seed=0, offset=0, log_std=None, timeout_s=0.05):
        """The control loop's call (rmt:742-771 at 1-4 rows; callers envs/rllib_env_imitation.py:215-266) with the
        observation taken from, and the action delivered to, HOST memory by the kernels themselves: `obs` is a CPU
        tensor / array [rows, 2 Db] (it is placed in a pinned staging buffer that the first encoder launch reads over
        PCIe), and the decoder's last launch stores the action straight into a pinned result buffer.  No copy
        launches either way and no stream synchronisation: the result buffer is pre-filled with NaN and the host
        waits until every entry has been overwritten (each 4-byte store arrives whole; Philox draws only -- supplied
        draws would need a copy of their own).  Returns a CPU tensor [rows, Da] ([rows, 2 Da] = [a_hat | log_std]
        with `log_std`, a device tensor [Da]) that stays valid until the next call.  If an entry is still missing
        after `timeout_s` (e.g. the model itself produced a NaN) the call falls back to a stream synchronisation."""
        import time as _time
        import numpy as _np
        self._need_gpu()
        Da, Db = self.arch.Da, self.arch.Db
        if isinstance(obs, torch.Tensor):
            obs = obs.detach().cpu().numpy()
        obs = _np.asarray(obs, dtype=_np.float32).reshape(-1, 2 * Db)
        rows = obs.shape[0]
        if not (1 <= rows <= 4 and self.fused_rollout):
            raise ValueError("infer_host serves the control loop's 1-4 rows (the library's rollout path)")
        h = getattr(self, "_host_io", None)
        if h is None:
            h_obs = torch.empty(4, 2 * Db, dtype=torch.float32).pin_memory()
            h_out = torch.empty(4, 2 * Da, dtype=torch.float32).pin_memory()
            h = self._host_io = (h_obs, h_out, h_obs.numpy(), h_out.numpy())
        h_obs, h_out, n_obs, n_out = h
        n_obs[:rows] = obs
        width = 2 * Da if log_std is not None else Da
        res = n_out[:rows, :width]
        # "not written yet" = one particular quiet-NaN bit pattern no arithmetic produces (a NaN the MODEL computes is the
        # canonical 0x7fc00000 / 0xffc00000 and counts as delivered): compared as integers, never with isnan
        bits = res.view(_np.uint32)
        bits.fill(0x7FC0DEAD)
        if log_std is not None:
            _lib.check(self.lib.pvae_infer_logits(self.ctx, h_obs.data_ptr(), rows, None, 1 if noise else 0, int(seed),
                                                  int(offset), h_out.data_ptr(), 2 * Da, log_std.data_ptr(), None, None,
                                                  self._stream()), "pvae_infer_logits")
        else:
            _lib.check(self.lib.pvae_infer_logits(self.ctx, h_obs.data_ptr(), rows, None, 1 if noise else 0, int(seed),
                                                  int(offset), h_out.data_ptr(), 2 * Da, None, None, None,
                                                  self._stream()), "pvae_infer_logits")
        t0 = _time.perf_counter()
        while (bits == 0x7FC0DEAD).any():
            if _time.perf_counter() - t0 > timeout_s:
                torch.cuda.current_stream(self.device).synchronize()
                break
        return h_out[:rows, :width]

    # -- call-persistent rollout server (include/pvae.h pvae_rollout_server_*) ---------------------------------
    def rollout_server_start(self, idle_ms=100.0, lifetime_s=600.0, scope="auto"):
        """Launch the resident rollout kernel (encoder + decoder weights in LDS, request block written by the host).
        `scope`: "xcd" = 32 workgroups on one XCD (the rest of the chip stays free), "chip" = 256 workgroups over all CUs
        (stacks too big for one XCD, e.g. 4x1024: kernels that need more LDS than is left wait for the server to leave),
        "auto" = one XCD when the stacks fit.  Raises RuntimeError when nothing fits: keep using `infer` / `infer_host`.
        While it is resident, device-wide synchronisations wait for it (at most `idle_ms` after the last request)."""
        self._need_gpu()
        env = os.environ.get("PVAE_SERVER_SCOPE", "")[:1]         # (A/B: overrides the caller's choice, as the C getenv did)
        scope = {"x": "xcd", "c": "chip"}.get(env, scope)
        mbx = os.environ.get("PVAE_SERVER_MAILBOX", "")[:1]
        _lib.check(self.lib.pvae_set_option(self.ctx, b"server_mailbox", {"h": 1, "d": 2}.get(mbx, 0)), "pvae_set_option")
        _lib.check(self.lib.pvae_rollout_server_start(self.ctx, float(idle_ms), float(lifetime_s),
                                                      {"auto": 0, "xcd": 1, "chip": 2}[scope]), "pvae_rollout_server_start")
        if self._srv_io is None:
            import numpy as _np
            Da, Db, Z = self.arch.Da, self.arch.Db, self.arch.Z
            bufs = (_np.zeros(2 * Db, _np.float32), _np.zeros(Da, _np.float32), _np.zeros(2 * Z, _np.float32), _np.zeros(Z, _np.float32))
            self._srv_io = bufs + tuple(C.c_void_p(b.ctypes.data) for b in bufs)       # (argument objects built once)
            self._srv_fn = self.lib.pvae_rollout_server_infer

    def rollout_server_infer(self, obs, noise=True, seed=0, offset=0, reload=False, timeout_ms=1000.0):
        """obs [2 Db] (CPU array / tensor) -> (a_hat [Da], mu_logvar [2 Z], z [Z]) as numpy views that stay valid until
        the next call; the same values as `infer(obs[None], noise=noise, seed=seed, offset=offset)`, bit for bit.
        A plain host call: no launch, no stream operation.  `reload`: copy the weights from the arena into LDS first."""
        io = self._srv_io
        if io is None:
            raise RuntimeError("rollout server not started (rollout_server_start)")
        n_obs, n_a, n_ml, n_z, p_obs, p_a, p_ml, p_z = io
        if isinstance(obs, torch.Tensor):
            obs = obs.detach().cpu().numpy()
        n_obs[:] = obs.reshape(-1)
        rc = self._srv_fn(self.ctx, p_obs, 1 if noise else 0, seed, offset, 1 if reload else 0, p_a, p_ml, p_z, timeout_ms)
        if rc:
            _lib.check(rc, "pvae_rollout_server_infer")
        return n_a, n_ml, n_z

    def rollout_server_infer_rows(self, obs, noise=True, seed=0, offset=0, reload=False, timeout_ms=1000.0):
        """obs [rows, 2 Db], 1 <= rows <= 4 -> (a_hat [rows, Da], mu_logvar [rows, 2 Z], z [rows, Z]) as fresh numpy arrays:
        ONE request to the resident kernel (every weight fragment read from LDS feeds all rows); the same values as
        `infer(obs, noise=noise, seed=seed, offset=offset)`, bit for bit."""
        import numpy as _np
        if self._srv_io is None:
            raise RuntimeError("rollout server not started (rollout_server_start)")
        if isinstance(obs, torch.Tensor):
            obs = obs.detach().cpu().numpy()
        x = _np.ascontiguousarray(obs, dtype=_np.float32).reshape(-1, 2 * self.arch.Db)
        rows = x.shape[0]
        a = _np.empty((rows, self.arch.Da), _np.float32)
        ml = _np.empty((rows, 2 * self.arch.Z), _np.float32)
        z = _np.empty((rows, self.arch.Z), _np.float32)
        _lib.check(self.lib.pvae_rollout_server_infer_rows(self.ctx, x.ctypes.data, rows, 1 if noise else 0, int(seed), int(offset),
                                                           1 if reload else 0, a.ctypes.data, ml.ctypes.data, z.ctypes.data,
                                                           float(timeout_ms)), "pvae_rollout_server_infer_rows")
        return a, ml, z

    def params_changed(self, stream=None):
        """The parameter arena was written outside the library (load_state_dict, a torch optimizer): holders of a copy -- the
        rollout server's LDS -- refresh before their next answer.  Optimizer steps through the library count by themselves."""
        if self.ctx is not None:
            _lib.check(self.lib.pvae_params_changed(self.ctx, stream), "pvae_params_changed")

    def rollout_server_decode(self, s1_z, timeout_ms=1000.0):
        """forward_decoder at B = 1 through the resident kernel: s1_z = [s1 (Db) | z (Z)] (CPU array) -> a_hat [Da] (numpy view,
        valid until the next call); the same bits as `net_forward(NET_MD, s1_z[None])`."""
        import numpy as _np
        io = self._srv_io
        if io is None:
            raise RuntimeError("rollout server not started (rollout_server_start)")
        x = _np.ascontiguousarray(_np.asarray(s1_z, dtype=_np.float32).reshape(-1))
        assert x.size == self.arch.Db + self.arch.Z, "s1_z must hold [s1 (Db) | z (Z)]"
        rc = self.lib.pvae_rollout_server_decode(self.ctx, x.ctypes.data, io[5], float(timeout_ms))
        if rc:
            _lib.check(rc, "pvae_rollout_server_decode")
        return io[1]

    def rollout_server_selfbench(self, obs, n=1000, noise=True):
        """us per request of n back-to-back requests, timed on the host clock INSIDE the library call (no Python per request)."""
        import numpy as _np
        o = _np.ascontiguousarray(_np.asarray(obs, dtype=_np.float32).reshape(-1))
        us = _np.zeros(int(n), _np.float64)
        _lib.check(self.lib.pvae_rollout_server_selfbench(self.ctx, o.ctypes.data, 1 if noise else 0, int(n), us.ctypes.data),
                   "pvae_rollout_server_selfbench")
        return us

    def rollout_server_timeline(self):
        """Microseconds after workgroup 0 saw the LAST request: [0, layer 0 inputs in LDS, layer 0 outputs published, ...,
        completion word issued], and the shader clock during that request in MHz -> (stamps, mhz)."""
        import numpy as _np
        us, n = _np.zeros(64, _np.float64), C.c_int32()
        _lib.check(self.lib.pvae_rollout_server_timeline(self.ctx, us.ctypes.data, 64, C.byref(n)), "pvae_rollout_server_timeline")
        return us[: n.value - 1], float(us[n.value - 1])

    def rollout_server_stop(self):
        if self.ctx is not None:
            _lib.check(self.lib.pvae_rollout_server_stop(self.ctx), "pvae_rollout_server_stop")

    def rollout_server_mailbox(self):
        """Where the request block lives while the server runs: "device" (the host writes device memory through the BAR,
        the kernel polls local memory), "host" (pinned host memory the kernel pulls from), None (not serving)."""
        a = C.c_int32()
        if self.ctx is None:
            return None
        _lib.check(self.lib.pvae_rollout_server_status(self.ctx, C.byref(a), None, None), "pvae_rollout_server_status")
        return {0: None, 1: "host", 2: "device"}[a.value]

    def rollout_server_status(self):
        """(serving, requests served so far, LDS bytes per workgroup)."""
        a, b, c = C.c_int32(), C.c_uint32(), C.c_int32()
        if self.ctx is None:
            return False, 0, 0
        _lib.check(self.lib.pvae_rollout_server_status(self.ctx, C.byref(a), C.byref(b), C.byref(c)), "pvae_rollout_server_status")
        return bool(a.value), b.value, abs(c.value)

    def rollout_server_scope(self):
        """"xcd" / "chip": over how much of the GPU the resident kernel's workgroups are dealt (None: never planned)."""
        c = C.c_int32()
        if self.ctx is None:
            return None
        _lib.check(self.lib.pvae_rollout_server_status(self.ctx, None, None, C.byref(c)), "pvae_rollout_server_status")
        return None if c.value == 0 else ("xcd" if c.value > 0 else "chip")

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


    # -- PPO learner step (include/pvae.h "PPO learner step of PhysicsVAE") ----------------------------
    def ppo_bind(self, value_engine, log_std, train_log_std=False):
        """Allocate (once, lazily) the PPO step's gradient arena, Adam moments and scratch -- buffers of the parameter
        arena's layout of their own, not the supervised trainer's `grads` / `exp_avg` / `exp_avg_sq` -- and bind them
        together with the log-std vector (Da contiguous floats on the device; `train_log_std`: its moments live here too)
        and the one-stack `StackSetEngine` that carries the value branch."""
        self._need_gpu()
        if getattr(self, "ppo_grad", None) is None:
            z = lambda n: torch.zeros(n, dtype=torch.float32, device=self.device)      # noqa: E731
            self.ppo_grad, self.ppo_m, self.ppo_v = z(self.arena_floats), z(self.arena_floats), z(self.arena_floats)
            self.ppo_scratch_bytes = int(self.lib.pvae_ppo_workspace_bytes(C.byref(self.cfg)))
            self.ppo_scratch = z(self.ppo_scratch_bytes // 4 + 4)
            self.ppo_ls_m = self.ppo_ls_v = None
        assert log_std.dtype == torch.float32 and log_std.device == self.device and log_std.is_contiguous() \
            and log_std.numel() == self.arch.Da, "log_std must be %d contiguous floats on %s" % (self.arch.Da, self.device)
        if train_log_std and self.ppo_ls_m is None:
            self.ppo_ls_m, self.ppo_ls_v = torch.zeros_like(log_std), torch.zeros_like(log_std)
        value_engine.ppo_bind(None, False)
        self._ppo_keep = (log_std, value_engine)           # (kept alive while bound)
        moments = (self.ppo_ls_m, self.ppo_ls_v) if train_log_std else (None, None)
        _lib.check(self.lib.pvae_ppo_bind(
            self.ctx, self.ppo_grad.data_ptr(), self.ppo_m.data_ptr(), self.ppo_v.data_ptr(), self.ppo_scratch.data_ptr(),
            self.ppo_scratch_bytes, log_std.data_ptr(), moments[0].data_ptr() if moments[0] is not None else None,
            moments[1].data_ptr() if moments[1] is not None else None, value_engine.ctx), "pvae_ppo_bind")

    def ppo_reset(self):
        """Adam's moments of the PPO step back to zero (the gradient arena and the scratch are rewritten by every step)."""
        for t in (getattr(self, "ppo_m", None), getattr(self, "ppo_v", None), getattr(self, "ppo_ls_m", None),
                  getattr(self, "ppo_ls_v", None)):
            if t is not None:
                t.zero_()
        keep = getattr(self, "_ppo_keep", None)
        if keep is not None:
            keep[1].ppo_reset()

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

    def ppo_step(self, batch, params, first, rows, index=None, eps=None, noise=True, seed=0, offset=0, stats_out=None):
        """`pvae_ppo_step`: one minibatch -- rows `index[first : first + rows]` of the batch (index None: rows first ..) --
        forward, loss, backward and Adam in one call; `eps` [rows, Z] or None (Philox at (seed, offset)).  Returns the five
        stats (a device tensor, nothing synchronises)."""
        self._need_gpu()
        b, keep = batch if isinstance(batch, tuple) else self.ppo_batch(batch)
        if stats_out is None:
            stats_out = torch.empty(5, dtype=torch.float32, device=self.device)
        _check_index(index, int(b.n_rows), self.device)
        eps = self._ppo_eps(eps, (int(rows), self.arch.Z))
        _lib.check(self.lib.pvae_ppo_step(self.ctx, C.byref(b), index.data_ptr() if index is not None else None, int(first),
                                          int(rows), C.byref(params), eps.data_ptr() if eps is not None else None,
                                          1 if noise else 0, int(seed), int(offset), stats_out.data_ptr(), self._stream()),
                   "pvae_ppo_step")
        return stats_out

    def ppo_sgd(self, batch, params, minibatch, num_sgd_iter, perm=None, eps=None, noise=True, seed=0, offset=0):
        """`pvae_ppo_sgd`: `num_sgd_iter` passes over the batch in minibatches of `minibatch` rows (the last one short), pass
        p in the order `perm[p]`; step i uses `eps[i]` (eps [steps, minibatch, Z]) or Philox offset `offset + i`, and Adam
        time step `params.adam_t + i`.  Returns stats [steps, 5] on the device; nothing synchronises."""
        self._need_gpu()
        b, keep = batch if isinstance(batch, tuple) else self.ppo_batch(batch)
        n = int(b.n_rows)
        steps = int(num_sgd_iter) * ((n + int(minibatch) - 1) // int(minibatch))
        stats = torch.empty(steps, 5, dtype=torch.float32, device=self.device)
        if perm is not None:
            assert tuple(perm.shape) == (int(num_sgd_iter), n), "perm must be [num_sgd_iter, n_rows]"
        _check_index(perm, n, self.device)
        eps = self._ppo_eps(eps, (steps, int(minibatch), self.arch.Z))
        _lib.check(self.lib.pvae_ppo_sgd(self.ctx, C.byref(b), perm.data_ptr() if perm is not None else None, int(minibatch),
                                         int(num_sgd_iter), C.byref(params), eps.data_ptr() if eps is not None else None,
                                         1 if noise else 0, int(seed), int(offset), stats.data_ptr(), self._stream()),
                   "pvae_ppo_sgd")
        return stats

    def ppo_launches(self):
        """Kernel launches of the last PPO step."""
        n = C.c_int32()
        _lib.check(self.lib.pvae_ppo_launches(self.ctx, C.byref(n)), "pvae_ppo_launches")
        return n.value

    # -- gradient exchange between workers (include/pvae.h "Gradient exchange between workers") --------
    def ppo_grad_step(self, batch, params, first, rows, index=None, eps=None, noise=True, seed=0, offset=0, stats_out=None):
        """`pvae_ppo_grad`: `ppo_step` up to, not including, its Adam launch -- the gradient lies in `ppo_grad` and the value
        engine's `ppo_grad`, nothing else moved.  Returns (stats [5], ls_grad [Da]: the log-std vector's gradient, written
        for a trained vector only)."""
        self._need_gpu()
        b, keep = batch if isinstance(batch, tuple) else self.ppo_batch(batch)
        if stats_out is None:
            stats_out = torch.empty(5, dtype=torch.float32, device=self.device)
        _check_index(index, int(b.n_rows), self.device)
        eps = self._ppo_eps(eps, (int(rows), self.arch.Z))
        ls_grad = _ppo_ls_grad(self, self.arch.Da)
        _lib.check(self.lib.pvae_ppo_grad(self.ctx, C.byref(b), index.data_ptr() if index is not None else None, int(first),
                                          int(rows), C.byref(params), eps.data_ptr() if eps is not None else None,
                                          1 if noise else 0, int(seed), int(offset), stats_out.data_ptr(), ls_grad.data_ptr(),
                                          self._stream()), "pvae_ppo_grad")
        return stats_out, ls_grad

    def ppo_apply(self, params, grad_scale=1.0, ls_grad=None):
        """`pvae_ppo_apply`: Adam (time step `params.adam_t`) over the trained nets on `grad_scale` times what the gradient
        buffers hold, and over a trained log-std vector on `grad_scale * ls_grad`."""
        self._need_gpu()
        _lib.check(self.lib.pvae_ppo_apply(self.ctx, C.byref(params), float(grad_scale),
                                           ls_grad.data_ptr() if ls_grad is not None else None, self._stream()), "pvae_ppo_apply")

    def ppo_grad_arenas(self):
        """The gradient buffers a transport outside the library reduces: this engine's and the value engine's."""
        return [self.ppo_grad, self._ppo_keep[1].ppo_grad]

    def ppo_peer_export(self):
        return _ppo_peer_export(self, self.lib.pvae_ppo_peer_export, "pvae_ppo_peer_export")

    def ppo_peer_open(self, rank, world, blobs):
        _ppo_peer_open(self, self.lib.pvae_ppo_peer_open, "pvae_ppo_peer_open", rank, world, blobs)

    def ppo_peer_close(self):
        if self.ctx is not None:
            _lib.check(self.lib.pvae_ppo_peer_close(self.ctx), "pvae_ppo_peer_close")

    def ppo_peer_status(self, sync=True):
        """(rank, world, waits that gave up) of the PPO gradient exchange; (0, 0, n) when none is open."""
        return _ppo_peer_status(self, self.lib.pvae_ppo_peer_status, "pvae_ppo_peer_status", sync)

    # -- train-batch preparation (include/pvae.h "Train-batch preparation for PhysicsVAE") ------------
    def _ppo_draws(self, n, eps, noise, seed, offset, out, want):
        """(pvae_ppo_draws, eps kept alive, latent_eps or None): `eps` [n, Z] supplied draws or None (Philox); `want`: the
        rows are evaluated, so the draws used are written to out["latent_eps"] (allocated when not given)."""
        d = _lib.PpoDraws()
        eps = self._ppo_eps(eps, (n, self.arch.Z))
        used = None
        if want:
            used = (out or {}).get("latent_eps")
            if used is None:
                used = torch.empty(n, self.arch.Z, dtype=torch.float32, device=self.device)
            assert used.dtype == torch.float32 and used.device == self.device and used.is_contiguous() \
                and tuple(used.shape) == (n, self.arch.Z), "out['latent_eps'] must be contiguous float32 [%d, %d]" % (n, self.arch.Z)
            d.eps_out = used.data_ptr()
        d.eps = eps.data_ptr() if eps is not None else None
        d.noise, d.rng_seed, d.rng_offset = 1 if noise else 0, int(seed), int(offset)
        return d, eps, used

    def ppo_evaluate(self, rollout, params, eps=None, noise=True, seed=0, offset=0, out=None):
        """`pvae_ppo_evaluate`: the current policy and value function over a device-resident rollout, in chunks of
        `max_batch` rows -- vf_preds [N], old_dist [N, 2 Da] = [a_hat | log_std], old_logp [N] of `actions` and latent_eps
        [N, Z], the draws used (when the rollout has obs and actions), and last_value [S], the bootstrap values (when it has
        seg_done and boot_obs; 0 for a done segment, whose boot_obs row is never read).  `eps` [N, Z]: the draws, row by row
        (None: Philox, chunk i at (seed, offset + i)); `noise` False: z = mu.  `ppo_bind` must have been called.  Returns
        the dict of what was computed; nothing synchronises."""
        self._need_gpu()
        ro, need, names = evaluate_plan(rollout, self.device)
        r, keep = make_rollout(ro, need, self.device, 2 * self.arch.Db, self.arch.Da)
        o, res = make_prepared(int(r.n_rows), int(r.n_segs), names, out, self.device, self.arch.Da)
        d, eps, used = self._ppo_draws(int(r.n_rows), eps, noise, seed, offset, out, "vf_preds" in names)
        _lib.check(self.lib.pvae_ppo_evaluate(self.ctx, C.byref(r), C.byref(params), C.byref(d), C.byref(o), self._stream()),
                   "pvae_ppo_evaluate")
        if used is not None:
            res["latent_eps"] = used
        return res

    def ppo_prepare(self, rollout, params, eps=None, noise=True, seed=0, offset=0, out=None):
        """`pvae_ppo_prepare`: evaluate (unless the rollout carries the sampler's own vf_preds, old_dist and old_logp: all
        three or none), bootstrap, GAE and -- with `params.standardize` -- the standardisation, all enqueued on the current
        stream; nothing synchronises.  Returns {vf_preds, old_dist, old_logp, latent_eps, last_value, advantages,
        value_targets}; the sampler's columns, when given, come back as they are (and latent_eps is None: nothing was
        drawn).  Draws as `ppo_evaluate`; `out`: tensors to write into, by those names."""
        self._need_gpu()
        r, keep = make_rollout(rollout, ("obs", "actions", "rewards", "seg_start", "boot_obs"), self.device, 2 * self.arch.Db,
                               self.arch.Da)
        names, given = prepare_plan(rollout)
        o, res = make_prepared(int(r.n_rows), int(r.n_segs), names, out, self.device, self.arch.Da)
        d, eps, used = self._ppo_draws(int(r.n_rows), None if given else eps, noise, seed, offset, out, not given)
        scratch, nbytes = gae_scratch_for(self, r.n_segs)
        _lib.check(self.lib.pvae_ppo_prepare(self.ctx, C.byref(r), C.byref(params), C.byref(d), C.byref(o), scratch.data_ptr(),
                                             nbytes, self._stream()), "pvae_ppo_prepare")
        if given:
            res.update({name: rollout[name] for name in ("vf_preds", "old_dist", "old_logp")})
        res["latent_eps"] = used
        return res

    def ppo_act(self, obs, params, explore=True, noise=None, clip=None, eps=None, latent_noise=True, seed=0, offset=0,
                out=None, out_row=None):
        """`pvae_ppo_act`: one policy step -- the sampled actions, old_dist = [a_hat | log_std], old_logp of the stored
        action, vf_preds, the action noise used and latent_eps [., Z], the latent draws used -- in the launches of the
        evaluate pass over the same rows.  `eps` [n, Z] / `latent_noise`: the latent draws as `ppo_evaluate` takes them;
        the action noise and the latent draws share (seed, offset + chunk).  The rest as `make_act`.  `ppo_bind` must have
        been called.  Returns the dict of columns; nothing synchronises."""
        self._need_gpu()
        i, o, res, keep = make_act(obs, 2 * self.arch.Db, self.arch.Da, self.device, explore, noise, clip, seed, offset, out,
                                   out_row, latent=self.arch.Z)
        d = _lib.PpoDraws()
        eps = self._ppo_eps(eps, (int(i.n_rows), self.arch.Z))
        d.eps = eps.data_ptr() if eps is not None else None
        d.eps_out = res["latent_eps"].data_ptr()
        d.noise, d.rng_seed, d.rng_offset = 1 if latent_noise else 0, int(seed), int(offset)
        _lib.check(self.lib.pvae_ppo_act(self.ctx, C.byref(i), C.byref(params), C.byref(d), C.byref(o), self._stream()),
                   "pvae_ppo_act")
        return res

    def gae_launches(self):
        """(evaluate, rest): kernel launches of the last ppo_prepare / ppo_evaluate -- the pass over the rows, and bootstrap +
        GAE + standardisation."""
        e, r = C.c_int32(), C.c_int32()
        _lib.check(self.lib.pvae_ppo_gae_launches(self.ctx, C.byref(e), C.byref(r)), "pvae_ppo_gae_launches")
        return e.value, r.value


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


class StackSetEngine:
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

    def _need_gpu(self):
        if self.ctx is None:
            raise RuntimeError("StackSetEngine was created on %s: the HIP hot path needs a GPU "
                               "(there is no CPU fallback)" % self.device)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

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

    # -- PPO learner step (include/pvae.h "PPO learner step") ---------------------------------------
    def ppo_bind(self, log_std=None, train_log_std=False):
        """Allocate (once, lazily) the gradient arena, Adam's moments and the scratch buffer of the PPO step and bind them.
        `log_std`: the vector of k values of a constant / state-independent log-std (None: state-dependent, a third
        stack); `train_log_std`: it is trained (its moments live here too)."""
        self._need_gpu()
        if getattr(self, "ppo_grad", None) is None:
            z = lambda n: torch.zeros(n, dtype=torch.float32, device=self.device)      # noqa: E731
            self.ppo_grad, self.ppo_m, self.ppo_v = z(self.arena_floats), z(self.arena_floats), z(self.arena_floats)
            self.ppo_scratch_bytes = int(self.lib.pvae_fc_ppo_workspace_bytes(C.byref(self.cfg)))
            self.ppo_scratch = z(self.ppo_scratch_bytes // 4 + 4)
            self.ppo_ls_m = self.ppo_ls_v = None
        if log_std is not None:
            assert log_std.dtype == torch.float32 and log_std.device == self.device and log_std.is_contiguous() \
                and log_std.numel() == self.n_outs[0], "log_std must be %d contiguous floats on %s" % (self.n_outs[0], self.device)
            if train_log_std and self.ppo_ls_m is None:
                self.ppo_ls_m, self.ppo_ls_v = torch.zeros_like(log_std), torch.zeros_like(log_std)
        self._ppo_log_std = log_std              # (kept alive while bound)
        moments = (self.ppo_ls_m, self.ppo_ls_v) if (log_std is not None and train_log_std) else (None, None)
        _lib.check(self.lib.pvae_fc_ppo_bind(
            self.ctx, self.ppo_grad.data_ptr(), self.ppo_m.data_ptr(), self.ppo_v.data_ptr(), self.ppo_scratch.data_ptr(),
            self.ppo_scratch_bytes, log_std.data_ptr() if log_std is not None else None,
            moments[0].data_ptr() if moments[0] is not None else None,
            moments[1].data_ptr() if moments[1] is not None else None), "pvae_fc_ppo_bind")

    def ppo_reset(self):
        """Adam's moments back to zero (the gradient arena and the scratch are rewritten by every step)."""
        for t in (getattr(self, "ppo_m", None), getattr(self, "ppo_v", None), getattr(self, "ppo_ls_m", None),
                  getattr(self, "ppo_ls_v", None)):
            if t is not None:
                t.zero_()

    def ppo_batch(self, batch, need_obs=True):
        """(pvae_fc_ppo_batch, the tensors it points to) from a dict of device tensors under the names of the loss's
        specification: obs, actions, old_dist, old_logp, advantages, value_targets, vf_preds."""
        return make_ppo_batch(batch, self.device, self.n_outs[0], self.n_in if need_obs else None)

    def ppo_step(self, batch, params, first, rows, index=None, stats_out=None):
        """`pvae_fc_ppo_step`: one minibatch -- rows `index[first : first + rows]` of the batch (index None: rows first ..) --
        forward, loss, backward and Adam in one call; returns the five stats (a device tensor, nothing synchronises)."""
        self._need_gpu()
        b, keep = batch if isinstance(batch, tuple) else self.ppo_batch(batch)
        if stats_out is None:
            stats_out = torch.empty(5, dtype=torch.float32, device=self.device)
        _check_index(index, int(b.n_rows), self.device)
        _lib.check(self.lib.pvae_fc_ppo_step(self.ctx, C.byref(b), index.data_ptr() if index is not None else None, int(first),
                                             int(rows), C.byref(params), stats_out.data_ptr(), self._stream()),
                   "pvae_fc_ppo_step")
        return stats_out

    def ppo_sgd(self, batch, params, minibatch, num_sgd_iter, perm=None):
        """`pvae_fc_ppo_sgd`: `num_sgd_iter` passes over the batch in minibatches of `minibatch` rows (the last one short),
        pass p in the order `perm[p]` (int32 [num_sgd_iter, n_rows] on the device; None: row order); `params.adam_t` is the
        first step's time step.  Returns stats [steps, 5] on the device; every launch is enqueued, nothing synchronises."""
        self._need_gpu()
        b, keep = batch if isinstance(batch, tuple) else self.ppo_batch(batch)
        n = int(b.n_rows)
        steps = int(num_sgd_iter) * ((n + int(minibatch) - 1) // int(minibatch))
        stats = torch.empty(max(steps, 0), 5, dtype=torch.float32, device=self.device)
        if perm is not None:
            assert tuple(perm.shape) == (int(num_sgd_iter), n), "perm must be [num_sgd_iter, n_rows]"
        _check_index(perm, n, self.device)
        _lib.check(self.lib.pvae_fc_ppo_sgd(self.ctx, C.byref(b), perm.data_ptr() if perm is not None else None, int(minibatch),
                                            int(num_sgd_iter), C.byref(params), stats.data_ptr(), self._stream()),
                   "pvae_fc_ppo_sgd")
        return stats

    def ppo_launches(self):
        """Kernel launches of the last PPO step."""
        n = C.c_int32()
        _lib.check(self.lib.pvae_fc_ppo_launches(self.ctx, C.byref(n)), "pvae_fc_ppo_launches")
        return n.value

    # -- gradient exchange between workers (include/pvae.h "Gradient exchange between workers") --------
    def ppo_grad_step(self, batch, params, first, rows, index=None, stats_out=None):
        """`pvae_fc_ppo_grad`: `ppo_step` up to, not including, its Adam launch -- the gradient lies in `ppo_grad`, nothing
        else moved.  Returns (stats [5], ls_grad [k]: the log-std vector's gradient, written for a trained vector only)."""
        self._need_gpu()
        b, keep = batch if isinstance(batch, tuple) else self.ppo_batch(batch)
        if stats_out is None:
            stats_out = torch.empty(5, dtype=torch.float32, device=self.device)
        _check_index(index, int(b.n_rows), self.device)
        ls_grad = _ppo_ls_grad(self, self.n_outs[0])
        _lib.check(self.lib.pvae_fc_ppo_grad(self.ctx, C.byref(b), index.data_ptr() if index is not None else None, int(first),
                                             int(rows), C.byref(params), stats_out.data_ptr(), ls_grad.data_ptr(),
                                             self._stream()), "pvae_fc_ppo_grad")
        return stats_out, ls_grad

    def ppo_apply(self, params, grad_scale=1.0, ls_grad=None):
        """`pvae_fc_ppo_apply`: Adam (time step `params.adam_t`) over the trained stacks on `grad_scale` times what `ppo_grad`
        holds, and over a trained log-std vector on `grad_scale * ls_grad`."""
        self._need_gpu()
        _lib.check(self.lib.pvae_fc_ppo_apply(self.ctx, C.byref(params), float(grad_scale),
                                              ls_grad.data_ptr() if ls_grad is not None else None, self._stream()),
                   "pvae_fc_ppo_apply")

    def ppo_grad_arenas(self):
        """The gradient buffers a transport outside the library reduces."""
        return [self.ppo_grad]

    def ppo_peer_export(self):
        return _ppo_peer_export(self, self.lib.pvae_fc_ppo_peer_export, "pvae_fc_ppo_peer_export")

    def ppo_peer_open(self, rank, world, blobs):
        _ppo_peer_open(self, self.lib.pvae_fc_ppo_peer_open, "pvae_fc_ppo_peer_open", rank, world, blobs)

    def ppo_peer_close(self):
        if self.ctx is not None:
            _lib.check(self.lib.pvae_fc_ppo_peer_close(self.ctx), "pvae_fc_ppo_peer_close")

    def ppo_peer_status(self, sync=True):
        """(rank, world, waits that gave up) of the PPO gradient exchange; (0, 0, n) when none is open."""
        return _ppo_peer_status(self, self.lib.pvae_fc_ppo_peer_status, "pvae_fc_ppo_peer_status", sync)

    # -- train-batch preparation (include/pvae.h "Train-batch preparation") --------------------------
    def _rollout(self, ro, need):
        return make_rollout(ro, need, self.device, self.n_in, self.n_outs[0])

    def _prepared(self, n, s, names, out):
        return make_prepared(n, s, names, out, self.device, self.n_outs[0])

    def _gae_scratch(self, n_segs):
        return gae_scratch_for(self, n_segs)

    def ppo_evaluate(self, rollout, params, out=None):
        """`pvae_fc_ppo_evaluate`: the current policy and value function over a device-resident rollout, in chunks of
        `max_batch` rows -- vf_preds [N], old_dist [N, 2k] = [mean | log_std], old_logp [N] of `actions` (when the rollout
        has obs and actions) and last_value [S], the bootstrap values (when it has seg_done and boot_obs; 0 for a done
        segment, whose boot_obs row is never read).  `params`: `PPOConfig.gae_params(kind, base)`; the log-std vector of a
        constant / state-independent kind is the one `ppo_bind` bound.  Returns the dict of what was computed."""
        self._need_gpu()
        ro, need, names = evaluate_plan(rollout, self.device)
        r, keep = self._rollout(ro, need)
        o, res = self._prepared(int(r.n_rows), int(r.n_segs), names, out)
        _lib.check(self.lib.pvae_fc_ppo_evaluate(self.ctx, C.byref(r), C.byref(params), C.byref(o), self._stream()),
                   "pvae_fc_ppo_evaluate")
        return res

    def ppo_prepare(self, rollout, params, out=None):
        """`pvae_fc_ppo_prepare`: evaluate (unless the rollout carries the sampler's own vf_preds, old_dist and old_logp: all
        three or none), bootstrap, GAE and -- with `params.standardize` -- the standardisation, all enqueued on the current
        stream; nothing synchronises.  Returns {vf_preds, old_dist, old_logp, last_value, advantages, value_targets}; the
        sampler's columns, when given, come back as they are.  `out`: tensors to write into, by those names."""
        self._need_gpu()
        r, keep = self._rollout(rollout, ("obs", "actions", "rewards", "seg_start", "boot_obs"))
        names, given = prepare_plan(rollout)
        o, res = self._prepared(int(r.n_rows), int(r.n_segs), names, out)
        scratch, nbytes = self._gae_scratch(r.n_segs)
        _lib.check(self.lib.pvae_fc_ppo_prepare(self.ctx, C.byref(r), C.byref(params), C.byref(o), scratch.data_ptr(), nbytes,
                                                self._stream()), "pvae_fc_ppo_prepare")
        if given:
            res.update({name: rollout[name] for name in ("vf_preds", "old_dist", "old_logp")})
        return res

    def ppo_act(self, obs, params, explore=True, noise=None, clip=None, seed=0, offset=0, out=None, out_row=None):
        """`pvae_fc_ppo_act`: one policy step -- the sampled actions, old_dist = [mean | log_std], old_logp of the stored
        action, vf_preds and the action noise used -- in the launches of the evaluate pass over the same rows.  `params`:
        `PPOConfig.gae_params(kind, base)` (the log-std kind; the vector of kinds 0 / 1 is the one `ppo_bind` bound); the
        rest as `make_act`.  Returns the dict of columns; nothing synchronises."""
        self._need_gpu()
        i, o, res, keep = make_act(obs, self.n_in, self.n_outs[0], self.device, explore, noise, clip, seed, offset, out, out_row)
        _lib.check(self.lib.pvae_fc_ppo_act(self.ctx, C.byref(i), C.byref(params), C.byref(o), self._stream()), "pvae_fc_ppo_act")
        return res

    def gae_launches(self):
        """(evaluate, rest): kernel launches of the last ppo_prepare / ppo_evaluate -- the pass over the rows, and bootstrap +
        GAE + standardisation."""
        e, r = C.c_int32(), C.c_int32()
        _lib.check(self.lib.pvae_fc_gae_launches(self.ctx, C.byref(e), C.byref(r)), "pvae_fc_gae_launches")
        return e.value, r.value

    def launches(self):
        """(forward, backward): kernel launches of the last call of each kind."""
        f, b = C.c_int32(), C.c_int32()
        _lib.check(self.lib.pvae_fc_launches(self.ctx, C.byref(f), C.byref(b)), "pvae_fc_launches")
        return f.value, b.value


def make_rollout(ro, need, device, n_in, k):
    """(pvae_fc_rollout, [tensors kept alive]) from a dict of device tensors: obs, actions, rewards, seg_start (int32
    [S + 1]), seg_done (bool / uint8 [S]), boot_obs ([S, n_in]) and, optionally, the sampler's vf_preds / old_dist /
    old_logp.  `need`: the names that must be there.  A `seg_start` given on the host is checked (its ends) and
    uploaded; one on the device is taken under the caller's contract: it runs from 0 to the number of rows.  Shared by
    the stack set's and PhysicsVAE's train-batch preparation (`n_in` inputs per observation, `k` actions per row)."""
    f32 = torch.float32
    r, keep = _lib.FcRollout(), []
    n = next((int(ro[c].shape[0]) for c in ("actions", "rewards", "obs") if ro.get(c) is not None), 1)
    s = int(ro["seg_done"].shape[0])
    shapes = {"obs": (n, n_in), "actions": (n, k), "rewards": (n,), "boot_obs": (s, n_in), "vf_preds": (n,),
              "old_dist": (n, 2 * k), "old_logp": (n,)}
    for name in need:
        if ro.get(name) is None:
            raise KeyError("rollout lacks %s" % name)
    for name, shape in shapes.items():
        t = ro.get(name)
        if t is None:
            continue
        t = t.reshape(t.shape[0], -1) if name in ("obs", "boot_obs") else t
        t = t.to(device, f32).contiguous()
        assert tuple(t.shape) == shape, "%s must be %s, got %s" % (name, shape, tuple(t.shape))
        keep.append(t)
        setattr(r, name, t.data_ptr())
    done = ro["seg_done"]
    done = done.to(device).contiguous()
    assert done.dtype in (torch.bool, torch.uint8) and done.dim() == 1, "seg_done must be bool or uint8 [S]"
    keep.append(done)
    r.seg_done = done.data_ptr()
    r.n_rows, r.n_segs, r.k = n, s, k
    r.seg_first, r.seg_last = 0, n
    if ro.get("seg_start") is not None:
        seg, (r.seg_first, r.seg_last) = _seg_start(ro["seg_start"], s, n, device)
        keep.append(seg)
        r.seg_start = seg.data_ptr()
    return r, keep


def make_prepared(n, s, names, out, device, k):
    """(pvae_fc_prepared, {name: tensor}) for the columns `names` of n rows and s segments: taken from `out` where it has
    them, allocated otherwise."""
    shapes = {"vf_preds": (n,), "old_dist": (n, 2 * k), "old_logp": (n,), "last_value": (s,), "advantages": (n,),
              "value_targets": (n,)}
    o, res = _lib.FcPrepared(), {}
    for name in names:
        t = (out or {}).get(name)
        if t is None:
            t = torch.empty(shapes[name], dtype=torch.float32, device=device)
        assert t.dtype == torch.float32 and t.device == device and t.is_contiguous() and tuple(t.shape) == shapes[name], \
            "out[%r] must be contiguous float32 %s on %s" % (name, shapes[name], device)
        res[name] = t
        setattr(o, name, t.data_ptr())
    return o, res


def gae_scratch_for(engine, n_segs):
    """(the engine's GAE scratch, grown when n_segs asks for more; the bytes `pvae_fc_gae_workspace_bytes` wants)"""
    need = int(engine.lib.pvae_fc_gae_workspace_bytes(int(n_segs)))
    if getattr(engine, "gae_scratch", None) is None or engine.gae_scratch.numel() * 8 < need:
        engine.gae_scratch = torch.zeros(need // 8 + 2, dtype=torch.float64, device=engine.device)
    return engine.gae_scratch, need


def evaluate_plan(rollout, device):
    """What an evaluate call computes from what the rollout holds: (rollout dict, needed names, output names)."""
    rows = rollout.get("obs") is not None
    boot = rollout.get("boot_obs") is not None
    ro = {c: rollout.get(c) for c in ("obs", "actions", "seg_done", "boot_obs")}
    if not boot:
        ro["seg_done"] = torch.zeros(1, dtype=torch.uint8, device=device)
    need = (("obs", "actions") if rows else ()) + (("boot_obs",) if boot else ())
    names = (("vf_preds", "old_dist", "old_logp") if rows else ()) + (("last_value",) if boot else ())
    return ro, need, names


def prepare_plan(rollout):
    """The output names of a prepare call, and whether the sampler's own columns are given (all three or none)."""
    given = [rollout.get(name) is not None for name in ("vf_preds", "old_dist", "old_logp")]
    if any(given) and not all(given):
        raise ValueError("the sampler's vf_preds, old_dist and old_logp go together: all three or none")
    names = (() if all(given) else ("vf_preds", "old_dist", "old_logp")) + ("last_value", "advantages", "value_targets")
    return names, all(given)


def make_act(obs, n_in, k, device, explore, noise, clip, seed, offset, out, out_row, latent=None):
    """(pvae_ppo_act_in, pvae_ppo_act_out, {name: column}, [tensors kept alive]) of one policy step (include/pvae.h "Action
    sampling").  obs [n, n_in]; `noise` [n, k] supplied action noise or None (Philox at (seed, offset + chunk)); `clip`:
    None or (low, high); `out`: the caller's columns by name -- actions, env_actions (with clip), old_dist, old_logp,
    vf_preds, action_noise, latent_eps (`latent` = Z: PhysicsVAE) and optionally obs --, every one of the same number of
    rows, allocated with n rows where missing (obs never; action_noise only when exploring); `out_row`: int32 [n] on the
    device, the row of those columns each input row is written to (None: row r to row r).  Shared by both engines."""
    f32 = torch.float32
    obs = obs.reshape(obs.shape[0], -1).to(device, f32).contiguous()
    n = int(obs.shape[0])
    assert tuple(obs.shape) == (n, n_in), "obs must be [n, %d], got %s" % (n_in, tuple(obs.shape))
    out = dict(out or {})
    n_dst = next((int(t.shape[0]) for t in out.values() if t is not None), n)
    i, o, keep = _lib.PpoActIn(), _lib.PpoActOut(), [obs]
    if explore and noise is not None:
        noise = noise.to(device, f32).contiguous()
        assert tuple(noise.shape) == (n, k), "noise must be [%d, %d], got %s" % (n, k, tuple(noise.shape))
        keep.append(noise)
        i.noise = noise.data_ptr()
    if out_row is not None:
        _check_index(out_row, n_dst, device)
        assert out_row.numel() == n, "out_row must name one destination row per input row"
        keep.append(out_row)
        i.out_row = out_row.data_ptr()
    i.obs, i.n_rows, i.n_dst_rows, i.k, i.explore = obs.data_ptr(), n, n_dst, k, 1 if explore else 0
    i.rng_seed, i.rng_offset = int(seed), int(offset)
    if clip is not None:
        i.clip, i.clip_low, i.clip_high = 1, float(clip[0]), float(clip[1])
    shapes = {"actions": (n_dst, k), "old_dist": (n_dst, 2 * k), "old_logp": (n_dst,), "vf_preds": (n_dst,)}
    if clip is not None:
        shapes["env_actions"] = (n_dst, k)
    if explore or out.get("action_noise") is not None:
        shapes["action_noise"] = (n_dst, k)
    if latent is not None:
        shapes["latent_eps"] = (n_dst, latent)
    if out.get("obs") is not None:
        shapes["obs"] = (n_dst, n_in)
    res = {}
    for name, shape in shapes.items():
        t = out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=f32, device=device)
        assert t.dtype == f32 and t.device == torch.device(device) and t.is_contiguous() and tuple(t.shape) == shape, \
            "out[%r] must be contiguous float32 %s on %s" % (name, shape, device)
        res[name] = t
        field = {"action_noise": "noise_out", "obs": "obs_dst", "latent_eps": None}.get(name, name)
        if field is not None:
            setattr(o, field, t.data_ptr())
    return i, o, res, keep


def set_fc_per_stack(on):
    """The stack set's launches one per stack instead of one per layer depth (process-wide; the A/B baseline of the grouping
    and a cross-check: both schedules give the same bits)."""
    lib = _lib.load()
    _lib.check(lib.pvae_set_option(None, b"fc_per_stack", 1 if on else 0), "pvae_set_option(fc_per_stack)")


PPO_COLUMNS = ("actions", "old_dist", "old_logp", "advantages", "value_targets", "vf_preds")


# -- the PPO learners' gradient exchange between workers: what HipEngine and StackSetEngine share ------------------------------
def _ppo_ls_grad(engine, k):
    """The k floats `*_ppo_grad` writes the log-std vector's gradient to (allocated once, kept with the engine)."""
    if getattr(engine, "ppo_ls_grad", None) is None:
        engine.ppo_ls_grad = torch.zeros(k, dtype=torch.float32, device=engine.device)
    return engine.ppo_ls_grad


def _ppo_peer_export(engine, fn, what):
    """The blob the peers open (IPC handles of the bound gradient buffers and the flag block, sizes).  `ppo_bind` first."""
    engine._need_gpu()
    buf = C.create_string_buffer(_lib.P2P_BLOB_BYTES)
    _lib.check(fn(engine.ctx, buf), what)
    return buf.raw


def _ppo_peer_open(engine, fn, what, rank, world, blobs):
    """Map the peers' gradient buffers and flag blocks (`blobs`: every rank's, in rank order) and run the attach-time check."""
    engine._need_gpu()
    assert len(blobs) == world and all(len(b) == _lib.P2P_BLOB_BYTES for b in blobs)
    _lib.check(fn(engine.ctx, int(rank), int(world), b"".join(blobs)), what)


def _ppo_peer_status(engine, fn, what, sync):
    if engine.ctx is None:
        return (0, 0, 0)
    r, w, t = C.c_int(), C.c_int(), C.c_uint32()
    _lib.check(fn(engine.ctx, C.byref(r), C.byref(w), C.byref(t) if sync else None, engine._stream()), what)
    return (r.value, w.value, t.value)


def make_ppo_batch(batch, device, k, n_in=None):
    """(pvae_fc_ppo_batch, [tensors kept alive]) from a dict of float32 device tensors; `n_in` None: no observations
    (`pvae_ppo_loss`).  Nothing is copied unless a column is not contiguous float32 on `device`."""
    device = torch.device(device)
    n = int(batch["actions"].shape[0])
    shapes = {"obs": (n, n_in), "actions": (n, k), "old_dist": (n, 2 * k), "old_logp": (n,), "advantages": (n,),
              "value_targets": (n,), "vf_preds": (n,)}
    b, keep = _lib.FcPpoBatch(), []
    for name in (("obs",) if n_in is not None else ()) + PPO_COLUMNS:
        t = batch[name]
        if name == "obs":
            t = t.reshape(t.shape[0], -1)
        t = t.to(device, torch.float32).contiguous()
        assert tuple(t.shape) == shapes[name], "%s must be %s, got %s" % (name, shapes[name], tuple(t.shape))
        keep.append(t)
        setattr(b, name, t.data_ptr())
    b.n_rows, b.k = n, int(k)
    return b, keep


def _check_index(index, n_rows, device):
    if index is not None:
        assert index.dtype == torch.int32 and index.is_contiguous() and index.device == torch.device(device), \
            "row indices must be contiguous int32 on %s" % device


def ppo_loss(mean, log_std, value, batch, params, index=None):
    """`pvae_ppo_loss`: the loss head alone on dense tensors.  mean [rows, k]; log_std [rows, k] (a row stride of 0 -- an
    expanded vector -- is passed as it is); value [rows]; `batch`: the columns (dict, or what `make_ppo_batch` returned),
    row r read at index[r].  Returns (stats [5], d_mean, d_log_std [rows, k], d_value): the gradients of stats[0]."""
    lib = _lib.load()
    dev = mean.device
    assert dev.type == "cuda", "pvae_ppo_loss needs a GPU (there is no CPU fallback)"
    rows, k = mean.shape
    mean = mean.float().contiguous()
    value = value.float().reshape(rows).contiguous()
    assert tuple(log_std.shape) == (rows, k)
    if not (log_std.dtype == torch.float32 and (k == 1 or log_std.stride(1) == 1) and log_std.stride(0) in (0, k)):
        log_std = log_std.float().contiguous()
    stride = 0 if (rows > 1 and log_std.stride(0) == 0) else k
    b, keep = batch if isinstance(batch, tuple) else make_ppo_batch(batch, dev, k)
    assert b.k == k
    _check_index(index, int(b.n_rows), dev)
    assert index is None or index.numel() >= rows
    d_mean, d_ls, d_val = torch.empty_like(mean), torch.empty(rows, k, dtype=torch.float32, device=dev), torch.empty_like(value)
    stats = torch.empty(5, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pvae_ppo_loss(mean.data_ptr(), log_std.data_ptr(), stride, value.data_ptr(), C.byref(b),
                                     index.data_ptr() if index is not None else None, rows, C.byref(params),
                                     d_mean.data_ptr(), d_ls.data_ptr(), d_val.data_ptr(), stats.data_ptr(),
                                     torch.cuda.current_stream(dev).cuda_stream), "pvae_ppo_loss")
    return stats, d_mean, d_ls, d_val


def _seg_start(seg_start, n_segs, n_rows, device):
    """(int32 device tensor [S + 1], (first, last)): a table on the host has its ends read; one already on the device cannot
    be read without a synchronisation and is taken under the caller's contract (0 .. n_rows)."""
    device = torch.device(device)
    seg = torch.as_tensor(seg_start)
    assert seg.dim() == 1 and seg.shape[0] == n_segs + 1, "seg_start must be [S + 1] = [%d], got %s" % (n_segs + 1, tuple(seg.shape))
    assert seg.dtype in (torch.int32, torch.int64), "seg_start must hold integers"
    ends = (int(seg[0]), int(seg[-1])) if seg.device.type == "cpu" else (0, n_rows)
    return seg.to(device, torch.int32).contiguous(), ends


_gae_scratch = {}


def gae(rewards, vf_preds, last_values, seg_start, gamma, lambda_, standardize=True, seg_done=None, out=None, info=None):
    """`pvae_gae`: GAE and the standardisation on dense device columns, no stack set (the specification: `ppo.gae_torch`,
    `ppo.standardize_torch`).  rewards / vf_preds [N], last_values [S] (read as 0 where `seg_done`), seg_start [S + 1].
    Returns (advantages, value_targets); `out`: a pair of tensors to write into; `info`: a dict that receives the number
    of kernel launches.  Nothing synchronises."""
    from .ppo import make_gae_params
    lib = _lib.load()
    dev = rewards.device
    assert dev.type == "cuda", "pvae_gae needs a GPU (there is no CPU fallback)"
    n, s = int(rewards.shape[0]), int(last_values.shape[0])
    cols = [t.to(dev, torch.float32).contiguous() for t in (rewards, vf_preds, last_values)]
    assert tuple(cols[1].shape) == (n,) and cols[0].dim() == 1 and cols[2].dim() == 1
    seg, ends = _seg_start(seg_start, s, n, dev)
    if seg_done is not None:
        seg_done = seg_done.to(dev).contiguous()
        assert seg_done.dtype in (torch.bool, torch.uint8) and tuple(seg_done.shape) == (s,), "seg_done must be bool or uint8 [S]"
    adv, vtarg = out if out is not None else (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
    for t in (adv, vtarg):
        assert t.dtype == torch.float32 and t.device == dev and t.is_contiguous() and tuple(t.shape) == (n,)
    need = int(lib.pvae_fc_gae_workspace_bytes(s))
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    scratch = _gae_scratch.get(key)
    if scratch is None or scratch.numel() * 8 < need:
        scratch = _gae_scratch[key] = torch.zeros(need // 8 + 2, dtype=torch.float64, device=dev)
    params = make_gae_params(gamma, lambda_, standardize)
    with torch.cuda.device(dev):
        rc = _lib.check(lib.pvae_gae(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), seg.data_ptr(),
                                     seg_done.data_ptr() if seg_done is not None else None, n, s, ends[0], ends[1],
                                     C.byref(params), adv.data_ptr(), vtarg.data_ptr(), scratch.data_ptr(), need, key[1]),
                        "pvae_gae")
    if info is not None:
        info["launches"] = rc
    return adv, vtarg
