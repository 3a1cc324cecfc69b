"""The PPO learner surface of both engines (`PpoSurface`), the structs its calls take (`make_ppo_batch`, `make_rollout`,
`make_prepared`, `make_act`, the evaluate / prepare plans) and the entry points that need no engine (`ppo_loss`, `gae`,
`ppo_order`).
"""
import ctypes as C

import torch

from . import _lib

PPO_COLUMNS = ("actions", "old_dist", "old_logp", "advantages", "value_targets", "vf_preds")
NO_DRAWS = (None, (), None)                  # what `_ppo_struct_draws` returns, for a model without a latent


class PpoSurface:
    """The PPO learner surface of an engine, written once: `HipEngine` (PhysicsVAE, C symbols `pvae_ppo_*`) and
    `StackSetEngine` (`pvae_fc_ppo_*`) both inherit it.  The two libraries' calls differ only in what the engine class
    supplies:

        _PPO, _PPO_GAE_LAUNCHES    the symbol prefix, and the one name that does not follow it
        _PPO_NEEDS_LOG_STD         `ppo_bind` insists on a log-std vector (the stack set's third stack can stand in for it)
        _ppo_dims                  (inputs per observation, actions per row, latent width or None), set by `__init__`
        _ppo_inline_draws(), _ppo_struct_draws()
                                   how latent draws become call arguments, for a model that has a latent: the `_ppo_*`
                                   bodies take `draws` = None (nothing is passed) or what these two understand
        ppo_batch(batch)           the engine's `make_ppo_batch`

    and, where its argument list carries draws or a companion engine, a one-line method of that signature over the
    `_ppo_*` body here.  Companion engines (PhysicsVAE's value engine) are kept in `_ppo_keep` behind the log-std vector;
    `ppo_bind`, `ppo_reset` and `ppo_grad_arenas` forward to them.  Expects of the engine: `lib`, `ctx`, `cfg`, `device`,
    `arena_floats`."""

    _PPO = _PPO_GAE_LAUNCHES = None
    _PPO_NEEDS_LOG_STD = False

    # -- what every call of either engine starts with ------------------------------------------------
    def _need_gpu(self):
        if self.ctx is None:
            raise RuntimeError("%s was created on %s: the HIP hot path needs a GPU "
                               "(there is no CPU fallback)" % (type(self).__name__, self.device))

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _ppo(self, name, *args):
        """`<prefix><name>(ctx, *args)`, checked under the C function's name.  (The calls made once per step or per
        action spell these two lines out: a frame less on a host path of tens of microseconds.)"""
        what = self._PPO + name
        return _lib.check(getattr(self.lib, what)(self.ctx, *args), what)

    # -- PPO learner step (include/pvae.h "PPO learner step", "PPO learner step of PhysicsVAE") --------
    def ppo_bind(self, log_std=None, train_log_std=False):
        """Allocate (once, lazily) the gradient arena, Adam's moments and the scratch buffer of the PPO step and bind them.
        `log_std`: the vector of k values of a constant / state-independent log-std (None: state-dependent, a third
        stack); `train_log_std`: it is trained (its moments live here too)."""
        return self._ppo_bind(log_std, train_log_std)

    def _ppo_bind(self, log_std, train_log_std, *companions):
        self._need_gpu()
        if getattr(self, "ppo_grad", None) is None:
            z = lambda n: torch.zeros(n, dtype=torch.float32, device=self.device)      # noqa: E731
            self.ppo_grad, self.ppo_m, self.ppo_v = z(self.arena_floats), z(self.arena_floats), z(self.arena_floats)
            self.ppo_scratch_bytes = int(getattr(self.lib, self._PPO + "workspace_bytes")(C.byref(self.cfg)))
            self.ppo_scratch = z(self.ppo_scratch_bytes // 4 + 4)
            self.ppo_ls_m = self.ppo_ls_v = None
        k = self._ppo_dims[1]
        if log_std is not None or self._PPO_NEEDS_LOG_STD:
            assert log_std.dtype == torch.float32 and log_std.device == self.device and log_std.is_contiguous() \
                and log_std.numel() == k, "log_std must be %d contiguous floats on %s" % (k, self.device)
            if train_log_std and self.ppo_ls_m is None:
                self.ppo_ls_m, self.ppo_ls_v = torch.zeros_like(log_std), torch.zeros_like(log_std)
        ctxs = []
        for e in companions:
            e._ppo_bind(None, False)
            ctxs.append(e.ctx)
        self._ppo_keep = (log_std,) + companions           # (kept alive while bound)
        moments = (self.ppo_ls_m, self.ppo_ls_v) if (log_std is not None and train_log_std) else (None, None)
        what = self._PPO + "bind"
        _lib.check(getattr(self.lib, what)(
            self.ctx, self.ppo_grad.data_ptr(), self.ppo_m.data_ptr(), self.ppo_v.data_ptr(), self.ppo_scratch.data_ptr(),
            self.ppo_scratch_bytes, log_std.data_ptr() if log_std is not None else None,
            moments[0].data_ptr() if moments[0] is not None else None,
            moments[1].data_ptr() if moments[1] is not None else None, *ctxs), what)

    def ppo_reset(self):
        """Adam's moments of the PPO step back to zero (the gradient arena and the scratch are rewritten by every step)."""
        for t in (getattr(self, "ppo_m", None), getattr(self, "ppo_v", None), getattr(self, "ppo_ls_m", None),
                  getattr(self, "ppo_ls_v", None)):
            if t is not None:
                t.zero_()
        for e in (getattr(self, "_ppo_keep", None) or ())[1:]:
            e.ppo_reset()

    def ppo_step(self, batch, params, first, rows, index=None, stats_out=None):
        """`*_ppo_step`: one minibatch -- rows `index[first : first + rows]` of the batch (index None: rows first ..) --
        forward, loss, backward and Adam in one call; returns the five stats (a device tensor, nothing synchronises)."""
        return self._ppo_step(batch, params, first, rows, index, stats_out)

    def _ppo_step(self, batch, params, first, rows, index, stats_out, draws=None, grad=False):
        self._need_gpu()
        b, keep = batch if isinstance(batch, tuple) else self.ppo_batch(batch)
        if stats_out is None:
            stats_out = torch.empty(5, dtype=torch.float32, device=self.device)
        _check_index(index, int(b.n_rows), self.device)
        eps, draws = (None, ()) if draws is None else self._ppo_inline_draws(draws, (int(rows),))
        outs = (stats_out, self._ppo_ls_grad()) if grad else (stats_out,)
        what = self._PPO + ("grad" if grad else "step")
        _lib.check(getattr(self.lib, what)(self.ctx, C.byref(b), index.data_ptr() if index is not None else None, int(first),
                                           int(rows), C.byref(params), *draws, *[t.data_ptr() for t in outs], self._stream()), what)
        return outs if grad else stats_out

    def ppo_sgd(self, batch, params, minibatch, num_sgd_iter, perm=None):
        """`*_ppo_sgd`: `num_sgd_iter` passes over the batch in minibatches of `minibatch` rows (the last one short),
        pass p in the order `perm[p]` (int32 [num_sgd_iter, n_rows] on the device; None: row order); `params.adam_t` is the
        first step's time step.  Returns stats [steps, 5] on the device; every launch is enqueued, nothing synchronises."""
        return self._ppo_sgd(batch, params, minibatch, num_sgd_iter, perm)

    def _ppo_sgd(self, batch, params, minibatch, num_sgd_iter, perm, draws=None):
        self._need_gpu()
        b, keep = batch if isinstance(batch, tuple) else self.ppo_batch(batch)
        n = int(b.n_rows)
        steps = int(num_sgd_iter) * ((n + int(minibatch) - 1) // int(minibatch))
        stats = torch.empty(max(steps, 0), 5, dtype=torch.float32, device=self.device)
        if perm is not None:
            assert tuple(perm.shape) == (int(num_sgd_iter), n), "perm must be [num_sgd_iter, n_rows]"
        _check_index(perm, n, self.device)
        eps, draws = (None, ()) if draws is None else self._ppo_inline_draws(draws, (steps, int(minibatch)))
        what = self._PPO + "sgd"
        _lib.check(getattr(self.lib, what)(self.ctx, C.byref(b), perm.data_ptr() if perm is not None else None, int(minibatch),
                                           int(num_sgd_iter), C.byref(params), *draws, stats.data_ptr(), self._stream()), what)
        return stats

    def ppo_diag(self, buffer=None, row=0):
        """`*_ppo_diag`: bind the learner-diagnostics rows (`ppo.diag_buffer`: float32 [steps, PPO_DIAG] on this device)
        from row `row` on, or unbind (None).  While bound `ppo_step` writes the first bound row, `ppo_grad_step` its entries
        0..3, `ppo_apply` its entry 4 and `ppo_sgd` one row per step (it refuses a buffer with fewer rows); see `ppo.DIAG`.
        The partial-sum scratch is allocated once and kept with the engine."""
        self._need_gpu()
        what = self._PPO + "diag"
        if buffer is None:
            self._ppo_diag_keep = None
            return _lib.check(getattr(self.lib, what)(self.ctx, None, 0, None, 0), what)
        check_diag(buffer, None, self.device)
        rows = int(buffer.shape[0]) - int(row)
        assert rows >= 1, "row %d outside the %d diagnostics rows" % (row, buffer.shape[0])
        if getattr(self, "ppo_diag_scratch", None) is None:
            cfg = C.byref(self.cfg) if self._PPO == "pvae_fc_ppo_" else self.ctx
            self.ppo_diag_bytes = int(getattr(self.lib, self._PPO + "diag_bytes")(cfg, 1))
            self.ppo_diag_scratch = torch.zeros(self.ppo_diag_bytes // 8 + 2, dtype=torch.float64, device=self.device)
        self._ppo_diag_keep = (buffer, int(row))              # (kept alive while bound)
        _lib.check(getattr(self.lib, what)(self.ctx, buffer.data_ptr() + 4 * _lib.PPO_DIAG * int(row), rows,
                                           self.ppo_diag_scratch.data_ptr(), self.ppo_diag_bytes), what)

    def ppo_diag_bound(self):
        """(buffer, row) as `ppo_diag` bound them last, or None: what a caller that binds rows of its own for one call
        puts back afterwards (`ppo_diag(*bound)`)."""
        return getattr(self, "_ppo_diag_keep", None)

    def ppo_grad_clip(self, max_norm=None):
        """`*_ppo_grad_clip`: bind global-norm gradient clipping at `max_norm` (a positive finite float) into the fused
        steps, or unbind (None).  While bound `ppo_step` / `ppo_sgd` clip this worker's gradient ahead of Adam (one launch
        more), `ppo_grad_step` leaves the clipped gradient behind and `ppo_apply` does not clip again; see `ppo.py`'s module
        docstring for the rule and `ppo.DIAG_CLIP` for the two diagnostics entries.  The scratch is allocated once and kept
        with the engine."""
        self._need_gpu()
        what = self._PPO + "grad_clip"
        if max_norm is None:
            self._ppo_clip_keep = None
            return _lib.check(getattr(self.lib, what)(self.ctx, 0.0, None, 0), what)
        if getattr(self, "ppo_clip_scratch", None) is None:
            cfg = C.byref(self.cfg) if self._PPO == "pvae_fc_ppo_" else self.ctx
            self.ppo_clip_bytes = int(getattr(self.lib, what + "_bytes")(cfg))
            self.ppo_clip_scratch = torch.zeros(self.ppo_clip_bytes // 8 + 2, dtype=torch.float64, device=self.device)
        _lib.check(getattr(self.lib, what)(self.ctx, float(max_norm), self.ppo_clip_scratch.data_ptr(), self.ppo_clip_bytes), what)
        self._ppo_clip_keep = float(max_norm)

    def ppo_grad_clip_bound(self):
        """`max_norm` as `ppo_grad_clip` bound it last, or None: what a caller that binds a clip of its own for one call puts
        back afterwards."""
        return getattr(self, "_ppo_clip_keep", None)

    def ppo_launches(self):
        """Kernel launches of the last PPO step."""
        n = C.c_int32()
        self._ppo("launches", C.byref(n))
        return n.value

    # -- gradient exchange between workers (include/pvae.h "Gradient exchange between workers") --------
    def ppo_grad_step(self, batch, params, first, rows, index=None, stats_out=None):
        """`*_ppo_grad`: `ppo_step` up to, not including, its Adam launch -- the gradient lies in `ppo_grad` (and the
        companion engines' `ppo_grad`), nothing else moved.  Returns (stats [5], ls_grad [k]: the log-std vector's
        gradient, written for a trained vector only)."""
        return self._ppo_step(batch, params, first, rows, index, stats_out, grad=True)

    def _ppo_ls_grad(self):
        """The k floats `*_ppo_grad` writes the log-std vector's gradient to (allocated once, kept with the engine)."""
        if getattr(self, "ppo_ls_grad", None) is None:
            self.ppo_ls_grad = torch.zeros(self._ppo_dims[1], dtype=torch.float32, device=self.device)
        return self.ppo_ls_grad

    def ppo_apply(self, params, grad_scale=1.0, ls_grad=None):
        """`*_ppo_apply`: Adam (time step `params.adam_t`) over the trained stacks on `grad_scale` times what the gradient
        buffers hold, and over a trained log-std vector on `grad_scale * ls_grad`."""
        self._need_gpu()
        what = self._PPO + "apply"
        _lib.check(getattr(self.lib, what)(self.ctx, C.byref(params), float(grad_scale),
                                           ls_grad.data_ptr() if ls_grad is not None else None, self._stream()), what)

    def ppo_grad_arenas(self):
        """The gradient buffers a transport outside the library reduces: this engine's and its companions'."""
        return [self.ppo_grad] + [e.ppo_grad for e in self._ppo_keep[1:]]

    def ppo_peer_export(self):
        """The blob the peers open (IPC handles of the bound gradient buffers and the flag block, sizes).  `ppo_bind` first."""
        self._need_gpu()
        buf = C.create_string_buffer(_lib.P2P_BLOB_BYTES)
        self._ppo("peer_export", buf)
        return buf.raw

    def ppo_peer_open(self, rank, world, blobs):
        """Map the peers' gradient buffers and flag blocks (`blobs`: every rank's, in rank order) and run the attach-time check."""
        self._need_gpu()
        assert len(blobs) == world and all(len(b) == _lib.P2P_BLOB_BYTES for b in blobs)
        self._ppo("peer_open", int(rank), int(world), b"".join(blobs))

    def ppo_peer_close(self):
        if self.ctx is not None:
            self._ppo("peer_close")

    def ppo_peer_status(self, sync=True):
        """(rank, world, waits that gave up) of the PPO gradient exchange; (0, 0, n) when none is open."""
        if self.ctx is None:
            return (0, 0, 0)
        r, w, t = C.c_int(), C.c_int(), C.c_uint32()
        self._ppo("peer_status", C.byref(r), C.byref(w), C.byref(t) if sync else None, self._stream())
        return (r.value, w.value, t.value)

    # -- train-batch preparation (include/pvae.h "Train-batch preparation", "... for PhysicsVAE") ------
    def ppo_evaluate(self, rollout, params, out=None):
        """`*_ppo_evaluate`: the current policy and value function over a device-resident rollout, in chunks of
        `max_batch` rows -- vf_preds [N], old_dist [N, 2k] = [mean | log_std], old_logp [N] of `actions` (when the rollout
        has obs and actions) and last_value [S], the bootstrap values (when it has seg_done and boot_obs; 0 for a done
        segment, whose boot_obs row is never read).  `params`: `PPOConfig.gae_params(kind, base)`; the log-std vector of a
        constant / state-independent kind is the one `ppo_bind` bound.  Returns the dict of what was computed."""
        return self._ppo_evaluate(rollout, params, out)

    def _ppo_evaluate(self, rollout, params, out, draws=None):
        self._need_gpu()
        n_in, k, _ = self._ppo_dims
        ro, need, names = evaluate_plan(rollout, self.device)
        r, keep = make_rollout(ro, need, self.device, n_in, k)
        o, res = make_prepared(int(r.n_rows), int(r.n_segs), names, out, self.device, k)
        eps, d, used = NO_DRAWS if draws is None else self._ppo_struct_draws(draws, int(r.n_rows), out, "vf_preds" in names)
        what = self._PPO + "evaluate"
        _lib.check(getattr(self.lib, what)(self.ctx, C.byref(r), C.byref(params), *d, C.byref(o), self._stream()), what)
        if used is not None:
            res["latent_eps"] = used
        return res

    def ppo_prepare(self, rollout, params, out=None):
        """`*_ppo_prepare`: evaluate (unless the rollout carries the sampler's own vf_preds, old_dist and old_logp: all
        three or none), bootstrap, GAE and -- with `params.standardize` -- the standardisation, all enqueued on the current
        stream; nothing synchronises.  Returns {vf_preds, old_dist, old_logp, last_value, advantages, value_targets}; the
        sampler's columns, when given, come back as they are.  `out`: tensors to write into, by those names."""
        return self._ppo_prepare(rollout, params, out)

    def _ppo_prepare(self, rollout, params, out, draws=None):
        self._need_gpu()
        n_in, k, _ = self._ppo_dims
        r, keep = make_rollout(rollout, ("obs", "actions", "rewards", "seg_start", "boot_obs"), self.device, n_in, k)
        names, given = prepare_plan(rollout)
        o, res = make_prepared(int(r.n_rows), int(r.n_segs), names, out, self.device, k)
        if given and draws is not None:
            draws = (None,) + tuple(draws[1:])            # (nothing is evaluated: supplied draws are not looked at)
        eps, d, used = NO_DRAWS if draws is None else self._ppo_struct_draws(draws, int(r.n_rows), out, not given)
        scratch, nbytes = gae_scratch_for(self, r.n_segs)
        what = self._PPO + "prepare"
        _lib.check(getattr(self.lib, what)(self.ctx, C.byref(r), C.byref(params), *d, C.byref(o), scratch.data_ptr(), nbytes,
                                           self._stream()), what)
        if given:
            res.update({name: rollout[name] for name in ("vf_preds", "old_dist", "old_logp")})
        if draws is not None:
            res["latent_eps"] = used
        return res

    def ppo_act(self, obs, params, explore=True, noise=None, clip=None, seed=0, offset=0, out=None, out_row=None):
        """`*_ppo_act`: one policy step -- the sampled actions, old_dist = [mean | log_std], old_logp of the stored
        action, vf_preds and the action noise used -- in the launches of the evaluate pass over the same rows.  `params`:
        `PPOConfig.gae_params(kind, base)` (the log-std kind; the vector of kinds 0 / 1 is the one `ppo_bind` bound); the
        rest as `make_act`.  Returns the dict of columns; nothing synchronises."""
        return self._ppo_act(obs, params, explore, noise, clip, seed, offset, out, out_row)

    def _ppo_act(self, obs, params, explore, noise, clip, seed, offset, out, out_row, draws=None):
        self._need_gpu()
        n_in, k, latent = self._ppo_dims
        i, o, res, keep = make_act(obs, n_in, k, self.device, explore, noise, clip, seed, offset, out, out_row, latent=latent)
        eps, d, _ = NO_DRAWS if draws is None else self._ppo_struct_draws(draws, int(i.n_rows), used=res["latent_eps"])
        what = self._PPO + "act"
        _lib.check(getattr(self.lib, what)(self.ctx, C.byref(i), C.byref(params), *d, C.byref(o), self._stream()), what)
        return res

    def gae_launches(self):
        """(evaluate, rest): kernel launches of the last ppo_prepare / ppo_evaluate -- the pass over the rows, and bootstrap +
        GAE + standardisation."""
        e, r = C.c_int32(), C.c_int32()
        what = self._PPO_GAE_LAUNCHES
        _lib.check(getattr(self.lib, what)(self.ctx, C.byref(e), C.byref(r)), what)
        return e.value, r.value


class PpoPolicy:
    """The PPO learner surface of a model, written once: `FullyConnectedPolicy` and `PhysicsVAE` both mix it in and keep
    the public methods (`ppo_learn`, `ppo_prepare`, `compute_actions`: their signatures and docstrings differ) as one-line
    calls of the `_policy_*` bodies here.  What the model class supplies (`call`: "learn", "prepare" or "act"):

        engine, _ppo_stacks()      a `PpoSurface`; the (name, FC stack) pairs a train mask has a bit for, in bit order
        _ppo_refusals()            what prepare, act and the data-parallel state refuse first (default: nothing)
        _ppo_learn_mask(config)    a learn call's refusals, in the class's own order -> `train_mask` of the step params
        _ppo_bind_engine()         bind the learner's buffers -> (log-std kind, base, the vector is trained)
        _ppo_draws(call, eps, dp_shape=None)    the draw keywords of the engine's call; `dp_shape` = (steps, minibatch):
                                   the torch transport takes supplied draws as one tensor
        _ppo_after(call, n)        n steps or chunks drew at the module's RNG counter; the last forward's results are gone
                                   (call "order", after "learn" under perm="philox": the minibatch order was drawn; it moves
                                   the counter only of a model whose learner draws nothing else)
        _ppo_order_key()           (seed, offset) the minibatch order is drawn at: the counter + 1 as the learn call finds it
        _ppo_dp_tensors(train_ls)  what `PPODataParallel.attach` copies from rank 0, after `_ppo_bind_engine`
        _PPO_PARTIAL_SAMPLER       prepare hands the sampler's columns on when only some are there (the library refuses them)
    """

    _PPO_PARTIAL_SAMPLER = False

    def _ppo_refusals(self):
        pass

    def _ppo_train_mask(self):
        """Bit s: stack s of `_ppo_stacks()` is trained.  Each is trained or frozen as a whole."""
        from . import autograd as AG
        mask = 0
        for s, (name, fn) in enumerate(self._ppo_stacks()):
            flags = [p.requires_grad for p in AG.stack_params(fn)]
            if any(flags) and not all(flags):
                raise NotImplementedError("%s is partially frozen: the fused PPO step trains or freezes a stack as a whole"
                                          % name)
            mask |= (1 << s) if all(flags) else 0
        return mask

    def _policy_learn(self, batch, config, perm, eps, dp, diag_out):
        from . import ppo as P
        eng = self.engine
        drawn = isinstance(perm, str)
        if drawn and perm not in P.ORDERS:
            raise ValueError("perm=%r: the minibatch order is None (row order), an int32 tensor [num_sgd_iter, n_rows] or "
                             "one of %s" % (perm, ", ".join('"%s"' % o for o in P.ORDERS)))
        train_mask = self._ppo_learn_mask(config)
        kind, base, train_ls = self._ppo_bind_engine()
        if kind == "state_independent" and not train_ls:
            kind = "constant"                    # a frozen vector is a constant one to the step
        cols = eng.ppo_batch(P.batch_columns(batch))
        n = int(cols[0].n_rows)
        t = self.__dict__.get("_ppo_t", 0)
        params = config.params(kind, base, adam_t=t + 1, train_mask=train_mask)
        if drawn:                                # its own library call; from here on it is a caller's tensor
            perm = ppo_order(n, config.num_sgd_iter, *self._ppo_order_key(), eng.device)
        elif perm is not None:
            perm = perm.to(eng.device, torch.int32).contiguous()
        if dp is not None:
            dp.check_steps(n, config, eng.device)
        if diag_out is not None:
            check_diag(diag_out, P.dp_steps(n, config.sgd_minibatch_size, config.num_sgd_iter), eng.device)
            bound = eng.ppo_diag_bound()
            eng.ppo_diag(diag_out)
        clip = getattr(config, "grad_clip", None)
        clip_bound = eng.ppo_grad_clip_bound() if clip is not None else None
        try:
            if clip is not None:                 # (`ppo.ClippedPPOConfig`: bound in the library for this call)
                eng.ppo_grad_clip(clip)
            if dp is not None and dp.transport == "torch":
                shape = (P.dp_steps(n, config.sgd_minibatch_size, config.num_sgd_iter), config.sgd_minibatch_size)
                stats = dp.sgd(eng, cols, lambda i: config.params(kind, base, adam_t=t + 1 + i, train_mask=train_mask), n,
                               config, perm, train_ls, diag_out=diag_out,
                               **self._ppo_draws("learn", eps, dp_shape=shape))
            else:
                stats = eng.ppo_sgd(cols, params, config.sgd_minibatch_size, config.num_sgd_iter, perm,
                                    **self._ppo_draws("learn", eps))
        finally:
            if clip is not None:
                eng.ppo_grad_clip(clip_bound)                 # what the caller had bound before comes back
            if diag_out is not None:
                eng.ppo_diag(*(bound or (None,)))             # what the caller had bound before comes back
        self.__dict__["_ppo_t"] = t + stats.shape[0]
        self._ppo_after("learn", stats.shape[0])
        if drawn:
            self._ppo_after("order", 1)
        return stats

    def _policy_prepare(self, rollout, config, eps):
        from . import ppo as P
        eng = self.engine
        self._ppo_refusals()
        eng._need_gpu()
        missing = [k for k in P.ROLLOUT_KEYS if rollout.get(k) is None]
        if missing:
            raise KeyError("rollout lacks %s" % ", ".join(missing))
        kind, base, _ = self._ppo_bind_engine()
        ro = {k: rollout[k] for k in ("obs", "actions", "rewards", "seg_start", "seg_done")}
        ro["boot_obs"] = rollout["next_obs_last"]
        given = [rollout.get(k) is not None for k in P.SAMPLER_KEYS]
        if all(given) or (self._PPO_PARTIAL_SAMPLER and any(given)):
            ro.update(vf_preds=rollout.get("vf_preds"), old_dist=rollout.get("action_dist_inputs"),
                      old_logp=rollout.get("action_logp"))
        res = eng.ppo_prepare(ro, config.gae_params(kind, base), **self._ppo_draws("prepare", eps))
        chunks = (int(rollout["actions"].shape[0]) + eng.max_batch - 1) // eng.max_batch
        self._ppo_after("prepare", 0 if all(given) else chunks)
        out = {"obs": rollout["obs"], "actions": rollout["actions"], "action_dist_inputs": res["old_dist"],
               "action_logp": res["old_logp"], "vf_preds": res["vf_preds"], "advantages": res["advantages"],
               "value_targets": res["value_targets"], "last_value": res["last_value"]}
        if "latent_eps" in res:
            out["latent_eps"] = res["latent_eps"]
        return out

    def _policy_act(self, obs, explore, noise, eps, clip, out, step):
        from . import ppo as P
        eng = self.engine
        self._ppo_refusals()
        eng._need_gpu()
        assert (out is None) == (step is None), "out (a RolloutBuffer) and step go together"
        kind, base, _ = self._ppo_bind_engine()
        cols, out_row = out.step_out(step, clip) if out is not None else (None, None)
        res = eng.ppo_act(obs.float(), P.make_gae_params(0.0, 0.0, False, kind, base), explore=explore, noise=noise, clip=clip,
                          out=cols, out_row=out_row, **self._ppo_draws("act", eps))
        self._ppo_after("act", (int(obs.shape[0]) + eng.max_batch - 1) // eng.max_batch)
        res = P.act_result(res, out, step)
        if not explore:
            res.pop("action_noise", None)
        return res

    def _ppo_dp_state(self):
        """Bind the PPO buffers and return what `PPODataParallel.attach` copies from rank 0: the parameters, the log-std
        vector and the PPO step's Adam moments (the step counter travels beside them)."""
        self._ppo_refusals()
        _, _, train_ls = self._ppo_bind_engine()
        return [t for t in self._ppo_dp_tensors(train_ls) if t is not None]

    def reset_ppo_optimizer(self):
        """Forget the PPO step's Adam state: moments to zero, time step to zero."""
        self.engine.ppo_reset()
        self.__dict__["_ppo_t"] = 0


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


def check_diag(diag, steps, device):
    """A diagnostics buffer is contiguous float32 [rows >= steps, PPO_DIAG] on `device`: a ValueError names what was
    given and what is wanted (`steps` None: any number of rows)."""
    want = "contiguous float32 [%s, %d] on %s" % ("rows" if steps is None else ">= %d" % steps, _lib.PPO_DIAG, torch.device(device))
    ok = torch.is_tensor(diag) and diag.dtype == torch.float32 and diag.dim() == 2 and diag.shape[1] == _lib.PPO_DIAG \
        and diag.is_contiguous() and diag.device == torch.device(device) and (steps is None or diag.shape[0] >= steps)
    if not ok:
        got = "%s %s on %s" % (diag.dtype, list(diag.shape), diag.device) if torch.is_tensor(diag) else repr(type(diag))
        raise ValueError("diag_out must be %s (ppo.diag_buffer), got %s" % (want, got))


def _check_index(index, n_rows, device):
    if index is not None:
        assert index.dtype == torch.int32 and index.is_contiguous() and index.device == torch.device(device), \
            "row indices must be contiguous int32 on %s" % device


def ppo_loss(mean, log_std, value, batch, params, index=None):
    """`pvae_ppo_loss`: the loss head alone on dense tensors.  mean [rows, k]; log_std [rows, k] (a row stride of 0 -- an
    expanded vector -- is passed as it is); value [rows]; `batch`: the columns (dict, or what `make_ppo_batch` returned),
    row r read at index[r].  Returns (stats [5], d_mean, d_log_std [rows, k], d_value): the gradients of stats[0]."""
    return _ppo_loss(mean, log_std, value, batch, params, index, None)


def ppo_loss_diag(mean, log_std, value, batch, params, index=None, diag_out=None):
    """`pvae_ppo_loss_diag`: `ppo_loss` with the learner diagnostics of the same rows.  `diag_out`: float32 [PPO_DIAG] on
    the device (None: allocated), filled with entries 0..3 of `ppo.DIAG` and 0 in the rest.  Returns `ppo_loss`'s four
    tensors, bit for bit, and the diagnostics row.  (Its own name: `ppo_loss`'s signature is pinned.)"""
    if diag_out is None:
        diag_out = torch.zeros(_lib.PPO_DIAG, dtype=torch.float32, device=mean.device)
    return _ppo_loss(mean, log_std, value, batch, params, index, diag_out) + (diag_out,)


def _ppo_loss(mean, log_std, value, batch, params, index, diag_out):
    lib = _lib.load()
    dev = mean.device
    assert dev.type == "cuda", "pvae_ppo_loss needs a GPU (there is no CPU fallback)"
    rows, k = mean.shape
    mean = mean.float().contiguous()
    value = value.float().reshape(rows).contiguous()
    assert tuple(log_std.shape) == (rows, k)
    assert log_std.device == dev and value.device == dev, "mean, log_std and value must be on one device (%s)" % dev
    if not (log_std.dtype == torch.float32 and (k == 1 or log_std.stride(1) == 1) and log_std.stride(0) in (0, k)):
        log_std = log_std.float().contiguous()
    stride = 0 if (rows > 1 and log_std.stride(0) == 0) else k
    b, keep = batch if isinstance(batch, tuple) else make_ppo_batch(batch, dev, k)
    assert b.k == k
    _check_index(index, int(b.n_rows), dev)
    assert index is None or index.numel() >= rows
    d_mean, d_ls, d_val = torch.empty_like(mean), torch.empty(rows, k, dtype=torch.float32, device=dev), torch.empty_like(value)
    stats = torch.empty(5, dtype=torch.float32, device=dev)
    if diag_out is not None:
        check_diag(diag_out.view(1, -1) if torch.is_tensor(diag_out) and diag_out.dim() == 1 else diag_out, 1, dev)
    with torch.cuda.device(dev):
        args = (mean.data_ptr(), log_std.data_ptr(), stride, value.data_ptr(), C.byref(b),
                index.data_ptr() if index is not None else None, rows, C.byref(params),
                d_mean.data_ptr(), d_ls.data_ptr(), d_val.data_ptr(), stats.data_ptr())
        st = torch.cuda.current_stream(dev).cuda_stream
        if diag_out is None:
            _lib.check(lib.pvae_ppo_loss(*args, st), "pvae_ppo_loss")
        else:
            _lib.check(lib.pvae_ppo_loss_diag(*args, diag_out.data_ptr(), st), "pvae_ppo_loss_diag")
    return stats, d_mean, d_ls, d_val


_order_scratch = {}


def ppo_order(n_rows, num_sgd_iter, seed, offset, device, out=None, info=None):
    """`pvae_ppo_order`: the minibatch order of `num_sgd_iter` passes over `n_rows` rows at (seed, offset) of the Philox
    stream (the rule: `ppo.py`'s module docstring; `ppo.minibatch_order` gives the same bits on the host).  Returns int32
    [num_sgd_iter, n_rows] on `device`, what `ppo_sgd` takes as `perm`; `out`: the tensor to write into; `info`: a dict
    that receives the number of kernel launches.  Enqueued on the current stream, nothing synchronises; the scratch is
    made once per (device, stream, size) and kept."""
    lib = _lib.load()
    dev = torch.device(device)
    assert dev.type == "cuda", "pvae_ppo_order needs a GPU (there is no CPU fallback)"
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    n, passes = int(n_rows), int(num_sgd_iter)
    need = int(lib.pvae_ppo_order_workspace_bytes(n, passes))
    if need == 0:
        _lib.check(-1, "pvae_ppo_order_workspace_bytes")
    if out is None:
        out = torch.empty(passes, n, dtype=torch.int32, device=dev)
    assert out.dtype == torch.int32 and out.device == dev and out.is_contiguous() and tuple(out.shape) == (passes, n), \
        "out must be contiguous int32 [%d, %d] on %s" % (passes, n, dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        key = (out.device, st, need)
        scratch = _order_scratch.get(key)
        if scratch is None:
            scratch = _order_scratch[key] = torch.empty(need // 8, dtype=torch.int64, device=out.device)
        rc = _lib.check(lib.pvae_ppo_order(n, passes, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), out.data_ptr(),
                                           scratch.data_ptr(), need, st), "pvae_ppo_order")
    if info is not None:
        info["launches"] = rc
    return out


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
