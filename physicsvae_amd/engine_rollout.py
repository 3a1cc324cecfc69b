"""The control loop's side of the rollout paths that answer in host memory: `infer_host` (the kernels read and write pinned
buffers) and the client of the call-persistent rollout server (`rollout_server_*`, `params_changed`).
"""
import ctypes as C
import os

import torch

from . import _lib


class RolloutClient:
    """Base class of `HipEngine`.  Expects of the engine: `lib`, `ctx`, `device`, `arch`, `fused_rollout`, `_need_gpu()`,
    `_stream()` and `_srv_io` (None until `rollout_server_start` built the request buffers; `__init__` sets it).  Keeps
    `_host_io` and `_srv_fn` of its own."""

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
