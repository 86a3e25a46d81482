"""ctypes binding of liblgx.so (include/lgx.h). The product path calls ONLY this
library for the env step; if it is missing it raises. A HIP device index runs the
kernels (buffers on that device); device -1 runs the library's host backend (buffers in
host memory) — chosen explicitly by --sim_device=cpu, never as a fallback."""
import ctypes as C
import os

from . import _abi, _cbind

LIB_PATH = os.environ.get("LGX_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "liblgx.so")
_lib = None


class LgxError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        _lib = _cbind.load(LIB_PATH, "liblgx", _abi.SIGNATURES, _abi.STRUCTS, ("lgx_abi_version", _abi.ABI_VERSION),
                           _abi.SIZEOF, LgxError)
    return _lib


EXPORTED = list(_abi.SIGNATURES)


class NativeEnv:
    """Owns one lgx_env handle; buffers are torch tensors owned by the caller."""

    def __init__(self, model_struct, params_struct, device_index):
        self._L = lib()
        self.model = model_struct
        self.params = params_struct
        self.device_index = int(device_index)
        self._dev_type = "cpu" if self.device_index < 0 else "cuda"
        self.handle = C.c_void_p()
        rc = self._L.lgx_create(C.byref(model_struct), C.byref(params_struct), device_index, C.byref(self.handle))
        self._check(rc, "lgx_create")
        self.buffers = _abi.Buffers()
        self._keep = {}

    def _check(self, rc, what):
        if rc != 0:
            msg = self._L.lgx_last_error(self.handle).decode() if self.handle else "?"
            raise LgxError(f"{what} failed ({rc}): {msg}")

    def bind(self, tensors):
        """tensors: dict field -> torch tensor (contiguous; on the HIP device, or on the CPU for
        device -1) or None."""
        for name in _abi.BUFFER_FIELDS:
            t = tensors.get(name)
            if t is None:
                setattr(self.buffers, name, None)
                continue
            if not t.is_contiguous():
                raise LgxError(f"buffer {name} must be contiguous")
            if t.device.type != self._dev_type:
                where = "host memory (device -1)" if self._dev_type == "cpu" else "the HIP device"
                raise LgxError(f"buffer {name} must live in {where} (got {t.device})")
            setattr(self.buffers, name, t.data_ptr())
            self._keep[name] = t
        self._check(self._L.lgx_bind(self.handle, C.byref(self.buffers)), "lgx_bind")

    def set_envs_per_wave(self, n):
        """lgx_set_envs_per_wave: 2 (default where it applies), 1, or 0 (default)."""
        self._check(self._L.lgx_set_envs_per_wave(self.handle, int(n)), "lgx_set_envs_per_wave")

    def step(self, seed, step_counter, stream):
        self._check(self._L.lgx_step(self.handle, seed, step_counter, C.c_void_p(stream)), "lgx_step")

    def step_dev(self, seed, step_counter_tensor, stream):
        """lgx_step_dev: the step counter lives in a device uint64/int64 scalar tensor."""
        self._check(self._L.lgx_step_dev(self.handle, seed, C.c_void_p(step_counter_tensor.data_ptr()),
                                         C.c_void_p(stream)), "lgx_step_dev")

    def post_physics(self, seed, step_counter, stream):
        self._check(self._L.lgx_post_physics(self.handle, seed, step_counter, C.c_void_p(stream)), "lgx_post_physics")

    def reset_envs(self, mask, seed, call, stream):
        self._keep["_mask"] = mask
        self._check(self._L.lgx_reset_envs(self.handle, C.c_void_p(mask.data_ptr()), seed, call, C.c_void_p(stream)),
                    "lgx_reset_envs")

    def command_curriculum(self, seed, step, global_sum_count, stream):
        """lgx_command_curriculum; `step`: a device int64 scalar (the step counter lgx_step_dev
        read) or an int; global_sum_count: None or a device float64 [2] {sum, count}."""
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        dev = hasattr(step, "data_ptr")
        self._check(self._L.lgx_command_curriculum(self.handle, seed, 0 if dev else int(step), p(step) if dev else None,
                                                   p(global_sum_count), C.c_void_p(stream)), "lgx_command_curriculum")

    def episode_extras(self, means, level_mean, time_outs, stream, step_dev=None):
        """lgx_episode_extras into the given device tensors (level_mean / time_outs: None = skip);
        consumes episode_stats and, with step_dev (a device int64 scalar), advances it by one."""
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        self._check(self._L.lgx_episode_extras(self.handle, p(means), p(level_mean), p(time_outs), p(step_dev),
                                               C.c_void_p(stream)), "lgx_episode_extras")

    def _fill(self, struct, label, table):
        """The check every tensor of a buffers struct gets, then struct.name = its address (struct None:
        check only). table: (name, tensor, shape or None for any, dtype, required) each; label names
        the struct in the LgxError. An optional tensor that is None leaves its member NULL."""
        for name, t, shape, dtype, required in table:
            if t is None:
                if required:
                    raise LgxError(f"{label} {name} is required")
                continue
            if (shape is not None and tuple(t.shape) != tuple(shape)) or str(t.dtype) != "torch." + dtype \
                    or not t.is_contiguous() or t.device.type != self._dev_type:
                raise LgxError(f"{label} {name} must be a contiguous {dtype} tensor"
                               f"{'' if shape is None else ' ' + str(list(shape))} in the env's memory space")
            if struct is not None:
                setattr(struct, name, t.data_ptr())

    def eval_buffers(self, acc, status, cells, overflow, cell_ids=None, push_rec=None, push_cells=None,
                     settle_tol=0.0, cmd_switch_step=None, cmd_rec=None, cmd_cells=None, yaw_tol=0.0, steady_after=0):
        """lgx_eval_buffers over the given tensors: acc [N, 8] fp32, status [N] uint8, cells
        [rows, cols, 12] float64, overflow [1] int32, all in the env's memory space. Optional
        (ABI 9; None = unset): cell_ids [N] int32 (the free cell key), push_rec [N, 4] fp32 with
        settle_tol, push_cells [rows, cols, 5] float64 (needs push_rec). ABI 10: cmd_switch_step [N]
        int32, cmd_rec [N, 8] fp32 with settle_tol, yaw_tol and steady_after (steps), cmd_cells
        [rows, cols, 9] float64 (needs cmd_rec; cmd_rec without cmd_switch_step is refused by the
        lgx_eval_* calls)."""
        n = self.params.num_envs
        if push_cells is not None and push_rec is None:
            raise LgxError("eval buffer push_cells needs push_rec")
        if not 0.0 <= float(settle_tol) < float("inf"):
            raise LgxError(f"settle_tol must be finite and >= 0 (got {settle_tol})")
        if cmd_cells is not None and cmd_rec is None:
            raise LgxError("eval buffer cmd_cells needs cmd_rec")
        if not 0.0 <= float(yaw_tol) < float("inf"):
            raise LgxError(f"yaw_tol must be finite and >= 0 (got {yaw_tol})")
        if not 0 <= int(steady_after) < 2 ** 31:
            raise LgxError(f"steady_after must be a step count >= 0 (got {steady_after})")
        ev = _abi.EvalBuffers()
        ev.settle_tol, ev.yaw_tol, ev.steady_after = float(settle_tol), float(yaw_tol), int(steady_after)
        if cells.dim() != 3 or cells.shape[2] != _abi.EVAL_CELL_COLS:
            raise LgxError(f"eval buffer cells must be [rows, cols, {_abi.EVAL_CELL_COLS}]")
        rc = tuple(cells.shape[:2])
        self._fill(ev, "eval buffer", [  # (a required one left None stays NULL: the lgx_eval_* calls refuse it)
            ("acc", acc, (n, _abi.EVAL_METRICS), "float32", False), ("status", status, (n,), "uint8", False),
            ("cells", cells, None, "float64", False), ("overflow", overflow, (1,), "int32", False),
            ("cell_ids", cell_ids, (n,), "int32", False), ("push_rec", push_rec, (n, _abi.EVAL_PUSH_REC), "float32", False),
            ("push_cells", push_cells, rc + (_abi.EVAL_PUSH_COLS,), "float64", False),
            ("cmd_switch_step", cmd_switch_step, (n,), "int32", False),
            ("cmd_rec", cmd_rec, (n, _abi.EVAL_CMD_REC), "float32", False),
            ("cmd_cells", cmd_cells, rc + (_abi.EVAL_CMD_COLS,), "float64", False)])
        ev.cell_rows, ev.cell_cols = int(cells.shape[0]), int(cells.shape[1])
        ev._keep = (acc, status, cells, overflow, cell_ids, push_rec, push_cells, cmd_switch_step, cmd_rec, cmd_cells)
        return ev

    def eval_begin(self, ev, stream):
        """lgx_eval_begin: zero the records (ev: eval_buffers(...))."""
        self._check(self._L.lgx_eval_begin(self.handle, C.byref(ev), C.c_void_p(stream)), "lgx_eval_begin")

    def eval_accumulate(self, ev, stream):
        """lgx_eval_accumulate: one sample per running env from the step just run."""
        self._check(self._L.lgx_eval_accumulate(self.handle, C.byref(ev), C.c_void_p(stream)), "lgx_eval_accumulate")

    def eval_reduce(self, ev, stream):
        """lgx_eval_reduce: records -> cells (and the out-of-grid count in ev.overflow)."""
        self._check(self._L.lgx_eval_reduce(self.handle, C.byref(ev), C.c_void_p(stream)), "lgx_eval_reduce")

    def trace_buffers(self, ring, count, status):
        """lgx_trace_buffers (ABI 11) over the given tensors: ring [N, depth, 76] fp32, count [N]
        int32, status [N] uint8, all in the env's memory space; depth is the ring's second dimension
        (>= 1). The ring takes N * depth * 304 bytes."""
        n = self.params.num_envs
        if ring is not None and (ring.dim() != 3 or ring.shape[1] < 1):
            raise LgxError(f"trace buffer ring must be [N, depth >= 1, {_abi.TRACE_COLS}] (depth = 0 holds no row)")
        tb = _abi.TraceBuffers()
        self._fill(tb, "trace buffer", [
            ("ring", ring, None if ring is None else (n, ring.shape[1], _abi.TRACE_COLS), "float32", True),
            ("count", count, (n,), "int32", True), ("status", status, (n,), "uint8", True)])
        tb.depth = int(ring.shape[1])
        tb._keep = (ring, count, status)
        return tb

    def trace_begin(self, tb, stream):
        """lgx_trace_begin: zero the rings, counts and statuses (tb: trace_buffers(...))."""
        self._check(self._L.lgx_trace_begin(self.handle, C.byref(tb), C.c_void_p(stream)), "lgx_trace_begin")

    def trace_record(self, tb, stream):
        """lgx_trace_record: one row per recording env from the step just run."""
        self._check(self._L.lgx_trace_record(self.handle, C.byref(tb), C.c_void_p(stream)), "lgx_trace_record")

    def trace_gather(self, tb, ids, out, out_len, stream):
        """lgx_trace_gather: unroll the rings of the envs ids [m] int32 into out [m, depth, 76] fp32 and
        out_len [m] int32 (all in the env's memory space). An id outside [0, N) gives zero rows and
        out_len -1."""
        m = int(ids.shape[0])
        self._fill(None, "trace gather", [("ids", ids, (m,), "int32", True),
                                          ("out", out, (m, tb.depth, _abi.TRACE_COLS), "float32", True),
                                          ("out_len", out_len, (m,), "int32", True)])
        self._check(self._L.lgx_trace_gather(self.handle, C.byref(tb), C.c_void_p(ids.data_ptr()), m,
                                             C.c_void_p(out.data_ptr()), C.c_void_p(out_len.data_ptr()),
                                             C.c_void_p(stream)), "lgx_trace_gather")

    def _record_buffers(self, kind, records, status, cells, overflow, cell_ids, **scalars):
        """The buffers struct of a record family (_abi.RECORD_KINDS[kind]) over the given tensors:
        records are its two record tensors in member order, scalars its extra scalar members."""
        cls, members, cell_cols, extra = _abi.RECORD_KINDS[kind]
        n = self.params.num_envs
        if cells is not None and (cells.dim() != 3 or cells.shape[2] != cell_cols):
            raise LgxError(f"{kind} buffer cells must be [rows, cols, {cell_cols}]")
        b = cls()
        self._fill(b, kind + " buffer", [
            *((name, t, (n,) + shape, "float32", True) for (name, shape), t in zip(members, records)),
            ("status", status, (n,), "uint8", True), ("cells", cells, None, "float64", True),
            ("overflow", overflow, (1,), "int32", True), ("cell_ids", cell_ids, (n,), "int32", False)])
        b.cell_rows, b.cell_cols = int(cells.shape[0]), int(cells.shape[1])
        for name in extra:
            setattr(b, name, float(scalars[name]))
        b._keep = (*records, status, cells, overflow, cell_ids)
        return b

    def _record_call(self, symbol, bufs, stream):
        """One lgx_<kind>_begin / _record / _reduce call on a family's buffers."""
        self._check(getattr(self._L, symbol)(self.handle, C.byref(bufs), C.c_void_p(stream)), symbol)

    def gait_buffers(self, foot, body, status, cells, overflow, cell_ids=None):
        """lgx_gait_buffers (ABI 12) over the given tensors: foot [N, 4, 16] fp32, body [N, 12] fp32,
        status [N] uint8, cells [rows, cols, 61] float64, overflow [1] int32 and, optional, cell_ids
        [N] int32 (the free cell key), all in the env's memory space."""
        return self._record_buffers("gait", (foot, body), status, cells, overflow, cell_ids)

    def gait_begin(self, gb, stream):
        """lgx_gait_begin: zero the records, the statuses and the overflow count (gb: gait_buffers(...))."""
        self._record_call("lgx_gait_begin", gb, stream)

    def gait_record(self, gb, stream):
        """lgx_gait_record: one sample per recording env from the step just run."""
        self._record_call("lgx_gait_record", gb, stream)

    def gait_reduce(self, gb, stream):
        """lgx_gait_reduce: records -> cells (and the out-of-grid count in gb.overflow)."""
        self._record_call("lgx_gait_reduce", gb, stream)

    def joint_buffers(self, joint, body, status, cells, overflow, cell_ids=None):
        """lgx_joint_buffers (ABI 13) over the given tensors: joint [N, 12, 16] fp32, body [N, 4] fp32,
        status [N] uint8, cells [rows, cols, 246] float64, overflow [1] int32 and, optional, cell_ids
        [N] int32 (the free cell key), all in the env's memory space."""
        return self._record_buffers("joint", (joint, body), status, cells, overflow, cell_ids)

    def joint_begin(self, jb, stream):
        """lgx_joint_begin: zero the records, the statuses and the overflow count (jb: joint_buffers(...))."""
        self._record_call("lgx_joint_begin", jb, stream)

    def joint_record(self, jb, stream):
        """lgx_joint_record: one sample per recording env from the step just run."""
        self._record_call("lgx_joint_record", jb, stream)

    def joint_reduce(self, jb, stream):
        """lgx_joint_reduce: records -> cells (and the out-of-grid count in jb.overflow)."""
        self._record_call("lgx_joint_reduce", jb, stream)

    def contact_buffers(self, body, env, status, cells, overflow, cell_ids=None, edge_tol=0.0):
        """lgx_contact_buffers (ABI 14) over the given tensors: body [N, 24, 12] fp32, env [N, 8] fp32,
        status [N] uint8, cells [rows, cols, 320] float64, overflow [1] int32 and, optional, cell_ids
        [N] int32 (the free cell key), all in the env's memory space; edge_tol: the relief (m) above
        which a contact onset counts as on an edge."""
        return self._record_buffers("contact", (body, env), status, cells, overflow, cell_ids, edge_tol=edge_tol)

    def contact_begin(self, cb, stream):
        """lgx_contact_begin: zero the records, the statuses and the overflow count and set the env rows'
        terminal columns to "none" (cb: contact_buffers(...))."""
        self._record_call("lgx_contact_begin", cb, stream)

    def contact_record(self, cb, stream):
        """lgx_contact_record: one sample per recording env from the step just run."""
        self._record_call("lgx_contact_record", cb, stream)

    def contact_reduce(self, cb, stream):
        """lgx_contact_reduce: records -> cells (and the out-of-grid count in cb.overflow)."""
        self._record_call("lgx_contact_reduce", cb, stream)

    def __del__(self):
        try:
            if self.handle:
                self._L.lgx_destroy(self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass
