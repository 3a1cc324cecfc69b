"""The data-parallel exchange of the supervised trainer inside the library: the RCCL communicator (`comm_*`), the
peer-mapped exchange (`p2p_*`) and the step that uses them (`dp_train_step`).
"""
import ctypes as C
import os

from . import _lib


class DataParallelExchange:
    """Base class of `HipEngine`.  Expects of the engine: `lib`, `ctx`, `_need_gpu()`, `_stream()`, `_eps(eps, rows)`,
    `_loss_scratch`, and the state its `__init__` sets: `has_comm` (the ctx owns an RCCL communicator), `has_p2p` (the
    peers' arenas are mapped) and `exchange_code` (what `comm_mode` last selected)."""

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
