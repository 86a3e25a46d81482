"""LeggedRobot — drop-in for legged_gym/envs/base/legged_robot.py:21-1152.

The whole env step (legged_robot.py:67-100: clip, decimation x {PD torque, simulate},
post_physics_step, obs clip) is ONE HIP kernel launch of liblgx.so (lgx_step), one
wavefront per env (--sim_device=cpu: the same entry point on the library's host backend). This class owns the torch buffers (same names/shapes as the
reference, env-major), builds the model/params once, binds the buffers to the native
env, and keeps the reference's Python-visible surface: step/reset/reset_idx, the
8-tuple return, extras['time_outs'/'episode'], common_step_counter, buffer attributes.
"""
import math
import os

import numpy as np
import torch

from legged_gym_custom_amd import LEGGED_GYM_ROOT_DIR, _abi, _native
from legged_gym_custom_amd import model as mdl
from legged_gym_custom_amd import params as prm
from legged_gym_custom_amd.envs.base.base_task import BaseTask
from legged_gym_custom_amd.utils import terrain_utils
from legged_gym_custom_amd.utils.helpers import class_to_dict
from legged_gym_custom_amd.utils.terrain import Terrain


class LeggedRobot(BaseTask):
    TASK_KIND = _abi.TASK_LEGGED

    def __init__(self, cfg, sim_params, physics_engine, sim_device, headless):
        self.cfg = cfg
        self.sim_params = sim_params
        self.height_samples = None
        self.debug_viz = False
        self.init_done = False
        self._parse_cfg(self.cfg)
        self.num_envs = self.cfg.env.num_envs
        self.seed = int(getattr(cfg, "seed", 1))
        if self.seed < 0:
            self.seed = 1
        # env sharding across ranks (one process per GPU): global env ids are used for
        # the RNG counter and terrain_types, so a sharded run draws what one GPU would.
        rank, world = 0, 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
        self.env_id_offset = rank * self.num_envs
        self.num_envs_total = world * self.num_envs
        super().__init__(self.cfg, sim_params, physics_engine, sim_device, headless)
        self._init_buffers()
        self._prepare_reward_function()
        self.init_done = True

    # ------------------------------------------------------------------ step
    def step(self, actions):
        """legged_robot.py:67-100 as one kernel launch; returns the reference's 8-tuple."""
        if actions.data_ptr() != self.actions_in.data_ptr():  # the PPO act head may write it in place
            self.actions_in.copy_(actions, non_blocking=True)
        # the counter the kernel reads lives on the device (lgx_step_dev; it holds the NEXT
        # step's number and lgx_episode_extras advances it), so a captured rollout replays with
        # the right step numbers; the host mirror follows
        self._csc += 1
        if not self._captured and self.sim_device_id >= 0 and torch.cuda.is_current_stream_capturing():
            self._captured = True  # a graph now holds this binding's addresses (set_motor_strength)
        self._native.step_dev(self.seed, self._step_dev, self._stream())
        if self._cmd_curriculum:
            self._command_curriculum()
        self._update_extras(advance_step=True)
        return (self.obs_buf, self.privileged_obs_buf, self.critic_obs_buf, self.estimated_obs_buf, self.scan_obs_buf,
                self.rew_buf, self.reset_buf, self.extras)

    def _command_curriculum(self):
        """update_command_curriculum for the step just run (one launch; a no-op unless the
        step is a multiple of max_episode_length). Env shards: the mean runs over the reset
        envs of every rank — one all-reduce of {sum, count} on those steps (the host knows
        them: common_step_counter), so the rollout of such a run is not graph-captured."""
        gsc = None
        if self.num_envs_total > self.num_envs and self._csc % int(self.max_episode_length) == 0:
            m = self.reset_buf
            gsc = torch.stack([torch.where(m, self._curriculum_vals, 0.0).double().sum(), m.double().sum()])
            torch.distributed.all_reduce(gsc)
        self._native.command_curriculum(self.seed, self._step_dev, gsc, self._stream())

    @property
    def graph_capturable(self):
        """Whether the runner may capture the rollout as one graph (not with a sharded
        command curriculum: it all-reduces on host-known steps)."""
        return not (self._cmd_curriculum and self.num_envs_total > self.num_envs)

    def reset_idx(self, env_ids):
        """reset_idx outside a step (BaseTask.reset): masked reset on device (RNG stream 1)."""
        if isinstance(env_ids, torch.Tensor):
            env_ids = env_ids.to(self.device)
        mask = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device)
        mask[env_ids] = 1
        self._native.reset_envs(mask, self.seed, self._reset_calls, self._stream())
        self._reset_calls += 1
        self.reset_buf[env_ids] = True
        self._update_extras()

    def _update_extras(self, advance_step=False):
        """extras['episode'] / ['time_outs'] with the reference's stale-when-no-reset
        semantics (go2.py:246-263, Appendix B Q5): one lgx_episode_extras launch (no host
        sync); _update_extras_torch states the same in torch ops (tests compare them)."""
        cur, to = self.cfg.terrain.curriculum, self.cfg.env.send_timeouts
        self._native.episode_extras(self._episode_means, self._terrain_level_mean if cur else None,
                                    self._extras_time_outs if to else None,
                                    self._stream(),
                                    self._step_dev if advance_step else None)
        self._publish_extras()

    def _publish_extras(self):
        if "episode" not in self.extras:
            self.extras["episode"] = {"rew_" + k: self._episode_means[i] for i, k in enumerate(self._episode_keys)}
            if self.cfg.terrain.curriculum:
                self.extras["episode"]["terrain_level"] = self._terrain_level_mean
            if self._cmd_curriculum:  # go2.py:255-259 / legged_robot.py:206-209
                keys = (["max_command_x", "min_command_x", "max_command_y", "max_command_yaw"]
                        if self.TASK_KIND == _abi.TASK_GO2 else ["max_command_x", "max_command_y", "max_command_yaw"])
                for i, k in enumerate(keys):
                    self.extras["episode"][k] = self._command_range_log[i]
        if self.cfg.env.send_timeouts:
            self.extras["time_outs"] = self._extras_time_outs

    def _update_extras_torch(self):
        st = self.episode_stats
        cnt = st[-1]
        means = st[:-1] / torch.clamp(cnt, min=1.0) / self.max_episode_length_s
        # in place on static buffers: a captured rollout keeps the stale-value chain
        self._episode_means.copy_(torch.where(cnt > 0, means, self._episode_means))
        if self.cfg.terrain.curriculum:  # go2.py:252-253 (mean level, refreshed when envs reset)
            self._terrain_level_mean.copy_(torch.where(cnt > 0, self.terrain_levels.float().mean(),
                                                       self._terrain_level_mean))
        if self.cfg.env.send_timeouts:
            self._extras_time_outs.copy_(torch.where(self.reset_buf.any(), self.time_out_buf, self._extras_time_outs))
        self._publish_extras()

    # ------------------------------------------------------------------ policy evaluation
    def _zeros(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, device=self.device, dtype=dtype)

    def _eval_buffers(self):
        """The evaluation's tensors (include/lgx.h lgx_eval_buffers), allocated once so a captured
        loop replays on fixed addresses: eval_acc [N, 8] and eval_status [N] (each env's first
        episode since eval_begin), the cells [terrain rows, terrain cols, 12] (1 x 1 without a
        terrain grid) and the out-of-grid counter."""
        if getattr(self, "_eval", None) is None:
            grid = getattr(self, "terrain_levels", None) is not None
            rows, cols = (int(self.cfg.terrain.num_rows), int(self.cfg.terrain.num_cols)) if grid else (1, 1)
            z = self._zeros
            self.eval_acc = z(self.num_envs, _abi.EVAL_METRICS)
            self.eval_status = z(self.num_envs, dtype=torch.uint8)
            self._eval_cells = z(rows, cols, _abi.EVAL_CELL_COLS, dtype=torch.float64)
            self._eval_overflow = z(1, dtype=torch.int32)
            self._eval = self._native.eval_buffers(self.eval_acc, self.eval_status, self._eval_cells,
                                                   self._eval_overflow)
        return self._eval

    def push_eval_buffers(self, rows, cols, settle_tol):
        """A second set of evaluation tensors for the push test (lgx_eval_buffers with cell_ids,
        push_rec and push_cells, ABI 9), allocated once per (rows, cols, settle_tol) so a captured
        loop replays on fixed addresses: push_cell_ids [N] int32 (the caller writes each env's bin
        in place), push_rec [N, 4] and, after eval_push_cells, cells [rows, cols, 12] and push cells
        [rows, cols, 5]. Pass the result as `ev` to eval_begin / eval_accumulate."""
        return self._bin_eval_buffers("push", int(rows), int(cols), _abi.EVAL_PUSH_REC, _abi.EVAL_PUSH_COLS,
                                      settle_tol=float(settle_tol))

    def _bin_eval_buffers(self, p, rows, cols, rec_cols, cell_cols, **tols):
        """The allocator behind push_eval_buffers (p = "push") and cmd_eval_buffers (p = "cmd"): eval
        tensors with a free cell key, a per-env record of rec_cols columns and its cells of
        cell_cols columns, allocated once per (rows, cols, the tolerances). The tensors become the
        attributes <p>_eval_acc, <p>_eval_status, <p>_cell_ids, <p>_rec (and cmd_switch_step),
        _<p>_eval_cells, _<p>_cells and _<p>_eval_overflow; returns the lgx_eval_buffers _<p>_eval."""
        key = (rows, cols) + tuple(tols.values())
        if getattr(self, f"_{p}_eval_key", None) != key:
            z, n = self._zeros, self.num_envs
            acc, status, ids, rec = z(n, _abi.EVAL_METRICS), z(n, dtype=torch.uint8), z(n, dtype=torch.int32), z(n, rec_cols)
            cells, bins = (z(rows, cols, k, dtype=torch.float64) for k in (_abi.EVAL_CELL_COLS, cell_cols))
            overflow = z(1, dtype=torch.int32)
            extra = {"cmd_switch_step": z(n, dtype=torch.int32)} if p == "cmd" else {}
            ev = self._native.eval_buffers(acc, status, cells, overflow, cell_ids=ids, **extra, **tols,
                                           **{f"{p}_rec": rec, f"{p}_cells": bins})
            vars(self).update({f"{p}_eval_acc": acc, f"{p}_eval_status": status, f"{p}_cell_ids": ids, f"{p}_rec": rec,
                               f"_{p}_eval_cells": cells, f"_{p}_cells": bins, f"_{p}_eval_overflow": overflow,
                               f"_{p}_eval": ev, f"_{p}_eval_key": key}, **extra)
        return getattr(self, f"_{p}_eval")

    def eval_begin(self, ev=None):
        """lgx_eval_begin: start recording every env's next (first) episode (ev: another set of
        eval buffers, push_eval_buffers(...); default: the plain evaluation's)."""
        self._native.eval_begin(self._eval_buffers() if ev is None else ev, self._stream())

    def eval_accumulate(self, ev=None):
        """lgx_eval_accumulate for the step just run (call after every step(); stream-ordered,
        no host sync, capturable)."""
        self._native.eval_accumulate(self._eval_buffers() if ev is None else ev, self._stream())

    def eval_push_cells(self):
        """lgx_eval_reduce on the push test's buffers, then (cells [rows, cols, 12], push cells
        [rows, cols, 5]: n, sum of peak tilt, sum of peak tracking error, survivors, sum of the
        survivors' settle steps) float64 on the host. Synchronises. A cell id outside the grid is
        an error."""
        return self._reduced_cells("lgx_eval_reduce", self._push_eval, self._push_eval_overflow, "a cell id",
                                   self._push_eval_cells, self._push_cells)

    def _reduced_cells(self, call, bufs, overflow, what, *cells):
        """The readers' common part: the native reduce `call` on bufs, the host read of its out-of-grid
        count (synchronises; any such env is an error that names `what` lay outside the grid), then
        the cell tensors cloned to the host."""
        getattr(self._native, call[len("lgx_"):])(bufs, self._stream())
        bad = int(overflow.item())
        if bad:
            raise _native.LgxError(f"{call}: {bad} envs have {what} outside the {bufs.cell_rows} x {bufs.cell_cols} "
                                   f"cell grid (cells not written)")
        return tuple(c.cpu().clone() for c in cells)

    def cmd_eval_buffers(self, rows, cols, settle_tol, yaw_tol, steady_after):
        """A set of evaluation tensors of its own for the command test (lgx_eval_buffers with
        cell_ids, cmd_switch_step, cmd_rec and cmd_cells, ABI 10), allocated once per (rows, cols,
        settle_tol, yaw_tol, steady_after) so a captured loop replays on fixed addresses:
        cmd_cell_ids [N] int32 and cmd_switch_step [N] int32 (the caller writes each env's bin and
        the episode step its record counts from in place; <= 0: no record), cmd_rec [N, 8] and,
        after eval_command_cells, cells [rows, cols, 12] and command cells [rows, cols, 9]. Pass
        the result as `ev` to eval_begin / eval_accumulate."""
        return self._bin_eval_buffers("cmd", int(rows), int(cols), _abi.EVAL_CMD_REC, _abi.EVAL_CMD_COLS,
                                      settle_tol=float(settle_tol), yaw_tol=float(yaw_tol),
                                      steady_after=int(steady_after))

    def eval_command_cells(self):
        """lgx_eval_reduce on the command test's buffers, then (cells [rows, cols, 12], command
        cells [rows, cols, 9]: n, survivors, the survivors' sums of linear and yaw settle steps, sum
        of peak tilt, the survivors' sums of steady samples and of achieved vx, vy, yaw rate) float64
        on the host. Synchronises. A cell id outside the grid is an error."""
        return self._reduced_cells("lgx_eval_reduce", self._cmd_eval, self._cmd_eval_overflow, "a cell id",
                                   self._cmd_eval_cells, self._cmd_cells)

    def sensor_eval_buffers(self, rows, cols):
        """A set of evaluation tensors of its own for the sensor test (lgx_eval_buffers with the free
        cell key cell_ids and the plain record, no per-env record of its own), allocated once per
        (rows, cols) so a captured loop replays on fixed addresses: sensor_cell_ids [N] int32 (the
        caller writes each env's bin in place), sensor_eval_acc [N, 8], sensor_eval_status [N] and,
        after eval_sensor_cells, cells [rows, cols, 12]. Pass the result as `ev` to eval_begin /
        eval_accumulate."""
        key = (int(rows), int(cols))
        if getattr(self, "_sensor_eval_key", None) != key:
            z, n = self._zeros, self.num_envs
            self.sensor_eval_acc, self.sensor_eval_status = z(n, _abi.EVAL_METRICS), z(n, dtype=torch.uint8)
            self.sensor_cell_ids = z(n, dtype=torch.int32)
            self._sensor_eval_cells = z(*key, _abi.EVAL_CELL_COLS, dtype=torch.float64)
            self._sensor_eval_overflow = z(1, dtype=torch.int32)
            self._sensor_eval = self._native.eval_buffers(self.sensor_eval_acc, self.sensor_eval_status,
                                                          self._sensor_eval_cells, self._sensor_eval_overflow,
                                                          cell_ids=self.sensor_cell_ids)
            self._sensor_eval_key = key
        return self._sensor_eval

    def eval_sensor_cells(self):
        """lgx_eval_reduce on the sensor test's buffers, then the cells [rows, cols, 12] float64 on
        the host. Synchronises. A cell id outside the grid is an error."""
        return self._reduced_cells("lgx_eval_reduce", self._sensor_eval, self._sensor_eval_overflow, "a cell id",
                                   self._sensor_eval_cells)[0]

    def scan_eval_buffers(self, rows, cols):
        """sensor_eval_buffers for the scan test (PolicyEvaluator.run_scan_test): scan_cell_ids [N]
        int32, scan_eval_acc [N, 8], scan_eval_status [N] and, after eval_scan_cells, cells
        [rows, cols, 12]; allocated once per (rows, cols)."""
        key = (int(rows), int(cols))
        if getattr(self, "_scan_eval_key", None) != key:
            z, n = self._zeros, self.num_envs
            self.scan_eval_acc, self.scan_eval_status = z(n, _abi.EVAL_METRICS), z(n, dtype=torch.uint8)
            self.scan_cell_ids = z(n, dtype=torch.int32)
            self._scan_eval_cells = z(*key, _abi.EVAL_CELL_COLS, dtype=torch.float64)
            self._scan_eval_overflow = z(1, dtype=torch.int32)
            self._scan_eval = self._native.eval_buffers(self.scan_eval_acc, self.scan_eval_status, self._scan_eval_cells,
                                                        self._scan_eval_overflow, cell_ids=self.scan_cell_ids)
            self._scan_eval_key = key
        return self._scan_eval

    def eval_scan_cells(self):
        """lgx_eval_reduce on the scan test's buffers, then the cells [rows, cols, 12] float64 on the
        host. Synchronises. A cell id outside the grid is an error."""
        return self._reduced_cells("lgx_eval_reduce", self._scan_eval, self._scan_eval_overflow, "a cell id",
                                   self._scan_eval_cells)[0]

    def eval_cells(self):
        """lgx_eval_reduce, then the cells [rows, cols, 12] float64 on the host: n_envs, n_timeout,
        n_fall, n_blowup and the sums of the 8 record columns over each cell's finished envs.
        Synchronises. An env whose terrain level / type lies outside the grid is an error."""
        return self._reduced_cells("lgx_eval_reduce", self._eval_buffers(), self._eval_overflow,
                                   "a terrain level / type", self._eval_cells)[0]

    # ------------------------------------------------------------------ flight recorder
    def trace_buffers(self, depth):
        """The flight recorder's tensors (include/lgx.h lgx_trace_buffers, ABI 11), allocated once
        per depth so a captured loop replays on fixed addresses: trace_ring [N, depth, 76] (the last
        `depth` control steps of each env's first episode since trace_begin; row i of an env lives in
        slot i % depth), trace_count [N] int32 (rows written, may exceed depth) and trace_status [N]
        (the eval_status rule). Each depth asked for keeps its tensors; the call makes that depth's
        recorder the current one, which trace_begin / trace_record / trace_gather and the three
        attributes refer to. Memory: the ring takes N x depth x 304 B, 124 MB at 4096 envs and
        depth 100 (2 s of go2)."""
        depth = int(depth)
        if depth < 1:
            raise ValueError(f"trace depth must be >= 1 (got {depth})")
        if not hasattr(self, "_traces"):
            self._traces = {}  # depth -> lgx_trace_buffers: a loop captured at a depth keeps its rings
        if depth not in self._traces:
            z = self._zeros
            self._traces[depth] = self._native.trace_buffers(
                z(self.num_envs, depth, _abi.TRACE_COLS), z(self.num_envs, dtype=torch.int32),
                z(self.num_envs, dtype=torch.uint8))
        self._trace = self._traces[depth]  # the current recorder: trace_begin / _record / _gather use it
        self.trace_ring, self.trace_count, self.trace_status = self._trace._keep
        return self._trace

    def _trace_buffers(self):
        if getattr(self, "_trace", None) is None:
            raise RuntimeError("no flight recorder: call trace_buffers(depth) first")
        return self._trace

    def trace_begin(self):
        """lgx_trace_begin: empty the rings and record every env's next (first) episode."""
        self._native.trace_begin(self._trace_buffers(), self._stream())

    def trace_record(self):
        """lgx_trace_record for the step just run (call after every step(); stream-ordered, no host
        sync, capturable)."""
        self._native.trace_record(self._trace_buffers(), self._stream())

    def trace_gather(self, ids):
        """lgx_trace_gather: the unrolled traces of the envs `ids` (a list or an integer tensor;
        duplicates allowed), oldest row first and newest last, zero rows in front of a trace shorter
        than the depth. Returns (out [m, depth, 76] fp32, out_len [m] int32) in the env's memory
        space: only the selection is unrolled. ValueError: an id outside [0, num_envs)."""
        tb = self._trace_buffers()
        ids = torch.as_tensor(ids).reshape(-1)
        if ids.numel() and (ids.dtype.is_floating_point or ids.dtype == torch.bool):
            raise ValueError(f"trace_gather: env ids must be integers (got {ids.dtype})")
        bad = ids[(ids < 0) | (ids >= self.num_envs)]
        if bad.numel():
            raise ValueError(f"trace_gather: env id {int(bad[0])} is outside [0, {self.num_envs})")
        ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        out = torch.empty(ids.shape[0], tb.depth, _abi.TRACE_COLS, device=self.device, dtype=torch.float32)
        out_len = torch.empty(ids.shape[0], device=self.device, dtype=torch.int32)
        self._native.trace_gather(tb, ids, out, out_len, self._stream())
        return out, out_len

    # ------------------------------------------------------------------ record families
    # kind -> the attributes its current set is published under: the two records, the status, the
    # cells, the overflow count (the set's tensors in this order) and the set itself
    _RECORD_ATTRS = {
        "gait": ("gait_foot", "gait_body", "gait_status", "_gait_cells", "_gait_overflow", "_gait"),
        "joint": ("joint_rec", "joint_body", "joint_status", "_joint_cells", "_joint_overflow", "_joint"),
        "contact": ("contact_body", "contact_env", "contact_status", "_contact_cells", "_contact_overflow", "_contact"),
    }

    def _record_set(self, kind, rows, cols, cell_ids, **scalars):
        """The tensors of a record family (_abi.RECORD_KINDS[kind]), allocated once per (rows, cols,
        cell_ids tensor, scalars) so a captured loop replays on fixed addresses. rows / cols None:
        the terrain grid (1 x 1 without one). Every key asked for keeps its tensors (a loop captured
        on one set never replays on freed memory); the call makes that set the current one and
        publishes it under the kind's _RECORD_ATTRS."""
        if rows is None or cols is None:
            grid = getattr(self, "terrain_levels", None) is not None
            rows, cols = (int(self.cfg.terrain.num_rows), int(self.cfg.terrain.num_cols)) if grid else (1, 1)
        key = (int(rows), int(cols), None if cell_ids is None else cell_ids.data_ptr(), *scalars.values())
        if not hasattr(self, "_record_sets"):
            self._record_sets = {}  # kind -> key -> the buffers struct (which keeps its tensors, cell_ids included)
        sets = self._record_sets.setdefault(kind, {})
        if key not in sets:
            z, n = self._zeros, self.num_envs
            _, members, cell_cols, _ = _abi.RECORD_KINDS[kind]
            sets[key] = self._native._record_buffers(
                kind, [z(n, *shape) for _, shape in members], z(n, dtype=torch.uint8),
                z(key[0], key[1], cell_cols, dtype=torch.float64), z(1, dtype=torch.int32), cell_ids, **scalars)
        cur = sets[key]
        for attr, value in zip(self._RECORD_ATTRS[kind], (*cur._keep[:5], cur)):
            setattr(self, attr, value)
        return cur

    def _record_current(self, kind):
        cur = getattr(self, self._RECORD_ATTRS[kind][5], None)
        if cur is None:
            raise RuntimeError(f"no {kind} record: call {kind}_buffers(...) first")
        return cur

    def record_begin(self, kind):
        """lgx_<kind>_begin on the kind's current set."""
        self._native._record_call(f"lgx_{kind}_begin", self._record_current(kind), self._stream())

    def record_step(self, kind):
        """lgx_<kind>_record on the kind's current set, for the step just run."""
        self._native._record_call(f"lgx_{kind}_record", self._record_current(kind), self._stream())

    def record_cells(self, kind):
        """lgx_<kind>_reduce on the kind's current set, then its cells float64 on the host."""
        cur = self._record_current(kind)
        return self._reduced_cells(f"lgx_{kind}_reduce", cur, cur._keep[4], "a terrain level / type (or cell id)",
                                   cur._keep[3])[0]

    def gait_buffers(self, rows=None, cols=None, cell_ids=None):
        """The gait record's tensors (include/lgx.h lgx_gait_buffers, ABI 12), allocated once per
        (rows, cols, cell_ids tensor) so a captured loop replays on fixed addresses: gait_foot
        [N, 4, 16] and gait_body [N, 12] (each env's first episode since gait_begin), gait_status [N]
        (the eval_status rule) and the cells [rows, cols, 61]. rows / cols None: the terrain grid
        (1 x 1 without one). cell_ids: an int32 [N] tensor with each env's cell (written in place by
        the caller), instead of terrain level x type. Every key asked for keeps its tensors (a loop
        captured on one set never replays on freed memory); the call makes that set the current
        one, which gait_begin / gait_record / gait_cells and the three attributes refer to."""
        return self._record_set("gait", rows, cols, cell_ids)

    def gait_begin(self):
        """lgx_gait_begin: zero the gait records and record every env's next (first) episode."""
        self.record_begin("gait")

    def gait_record(self):
        """lgx_gait_record for the step just run (call after every step(); stream-ordered, no host
        sync, capturable)."""
        self.record_step("gait")

    def gait_cells(self):
        """lgx_gait_reduce, then the cells [rows, cols, 61] float64 on the host: the number of
        finished envs with samples, the sums of their 12 body columns and of columns 4..15 of each
        foot. Synchronises. An env whose cell lies outside the grid is an error."""
        return self.record_cells("gait")

    def joint_buffers(self, rows=None, cols=None, cell_ids=None):
        """The joint-load record's tensors (include/lgx.h lgx_joint_buffers, ABI 13), allocated once
        per (rows, cols, cell_ids tensor) so a captured loop replays on fixed addresses: joint_rec
        [N, 12, 16] and joint_body [N, 4] (each env's first episode since joint_begin), joint_status
        [N] (the eval_status rule) and the cells [rows, cols, 246]. rows, cols and cell_ids as in
        gait_buffers; every key asked for keeps its tensors, and the call makes that set the current
        one, which joint_begin / joint_record / joint_cells and the three attributes refer to."""
        return self._record_set("joint", rows, cols, cell_ids)

    def joint_begin(self):
        """lgx_joint_begin: zero the joint records and record every env's next (first) episode."""
        self.record_begin("joint")

    def joint_record(self):
        """lgx_joint_record for the step just run (call after every step(); stream-ordered, no host
        sync, capturable)."""
        self.record_step("joint")

    def joint_cells(self):
        """lgx_joint_reduce, then the cells [rows, cols, 246] float64 on the host: the number of
        finished envs with samples, the sums and the peak of their body columns and, per joint, the
        sums of columns 1..15 and the extremes of columns 3, 6, 7, 10 and 11. Synchronises. An env
        whose cell lies outside the grid is an error."""
        return self.record_cells("joint")

    def contact_buffers(self, rows=None, cols=None, cell_ids=None, edge_tol=0.05):
        """The contact record's tensors (include/lgx.h lgx_contact_buffers, ABI 14), allocated once
        per (rows, cols, cell_ids tensor, edge_tol) so a captured loop replays on fixed addresses:
        contact_body [N, 24, 12] and contact_env [N, 8] (each env's first episode since
        contact_begin), contact_status [N] (the eval_status rule) and the cells [rows, cols, 320].
        rows, cols and cell_ids as in gait_buffers; edge_tol: the terrain relief (m) above which a
        contact onset counts as on an edge. Every key asked for keeps its tensors, and the call makes
        that set the current one, which contact_begin / contact_record / contact_cells and the three
        attributes refer to."""
        return self._record_set("contact", rows, cols, cell_ids, edge_tol=float(edge_tol))

    def contact_begin(self):
        """lgx_contact_begin: reset the contact records and record every env's next (first) episode."""
        self.record_begin("contact")

    def contact_record(self):
        """lgx_contact_record for the step just run (call after every step(); stream-ordered, no host
        sync, capturable)."""
        self.record_step("contact")

    def contact_cells(self):
        """lgx_contact_reduce, then the cells [rows, cols, 320] float64 on the host: the number of
        finished envs, the sums and the peak of their env columns, the falls and, per body, the sums
        of columns 1, 2, 3, 5, 6, 8, 9, 11, the extremes of columns 4, 10 and 7 and the two fall
        histograms. Synchronises. An env whose cell lies outside the grid is an error."""
        return self.record_cells("contact")

    def _stream(self):
        """The HIP stream the env's launches are ordered on (0 for the host backend)."""
        return torch.cuda.current_stream(self.device).cuda_stream if self.sim_device_id >= 0 else 0

    @property
    def common_step_counter(self):
        return self._csc

    @common_step_counter.setter
    def common_step_counter(self, value):
        self._csc = int(value)
        if hasattr(self, "_step_dev"):
            self._step_dev.fill_(self._csc + 1)  # the number the next step reads

    def advance_step_counter(self, k):
        """Host mirror after a replayed capture that already advanced the device counter k times."""
        self._csc += int(k)

    # ------------------------------------------------------------------ setup
    def create_sim(self):
        """legged_robot.py:278-293: terrain (heightfield / trimesh) or plane, then envs."""
        self.up_axis_idx = 2
        mesh_type = self.cfg.terrain.mesh_type
        if mesh_type in ("heightfield", "trimesh"):
            self.terrain = Terrain(self.cfg.terrain, self.num_envs)
        if mesh_type == "plane":
            self._create_ground_plane()
        elif mesh_type == "heightfield":
            self._create_heightfield()
        elif mesh_type == "trimesh":
            self._create_trimesh()
        elif mesh_type is not None:
            raise ValueError("Terrain mesh type not recognised. Allowed types are [None, plane, heightfield, trimesh]")
        self._create_envs()

    def _create_ground_plane(self):
        """legged_robot.py:757-765: the kernel's contact against z = 0 (no buffers)."""
        self._terrain_mesh = None

    def _upload_terrain(self, slope_threshold):
        t = self.terrain
        self.height_samples = torch.tensor(t.heightsamples).view(t.tot_rows, t.tot_cols).to(self.device)
        mesh = terrain_utils.pack_mesh(t.heightsamples, t.cfg.horizontal_scale, t.cfg.vertical_scale, slope_threshold)
        self._terrain_mesh = torch.from_numpy(mesh.view(np.int32)).to(self.device)

    def _create_heightfield(self):
        """legged_robot.py:768-786: heightfield collision (no wall correction) + samples."""
        self._upload_terrain(None)

    def _create_trimesh(self):
        """legged_robot.py:788-802: the slope-corrected triangle mesh + samples. The kernel
        collides against it through the packed per-vertex words (no index buffer)."""
        self._upload_terrain(self.cfg.terrain.slope_treshold)

    def _create_envs(self):
        """legged_robot.py:805-894: model, body/dof names, index tables, domain randomisation."""
        asset_cfg = self.cfg.asset
        self.model_dict = mdl.load_model(asset_cfg.file, asset_cfg.foot_name, LEGGED_GYM_ROOT_DIR)
        self.body_names = list(self.model_dict["body_names"])
        self.dof_names = list(self.model_dict["dof_names"])
        self.num_bodies = len(self.body_names)
        self.num_dof = self.num_dofs = len(self.dof_names)
        base = list(self.cfg.init_state.pos) + list(self.cfg.init_state.rot) + list(self.cfg.init_state.lin_vel) + \
            list(self.cfg.init_state.ang_vel)
        self.base_init_state = torch.tensor(base, dtype=torch.float, device=self.device)
        self._get_env_origins()
        # Setup-time randomisation is drawn for ALL global envs (the single-GPU draw order)
        # and this shard's slice kept, so env k gets the same friction / mass / gains on any
        # number of ranks.
        n, total = self.num_envs, self.num_envs_total
        sl = slice(self.env_id_offset, self.env_id_offset + n)
        dr = self.cfg.domain_rand
        # _process_rigid_shape_props legged_robot.py:318-329 (64 friction buckets, CPU RNG)
        if dr.randomize_friction:
            bucket_ids = torch.randint(0, 64, (total, 1))
            lo, hi = dr.friction_range
            buckets = (hi - lo) * torch.rand(64, 1) + lo
            self.friction_coeffs = buckets[bucket_ids][sl]
        mass = np.zeros((total, 4), dtype=np.float32)
        for i in range(total):
            torch.rand(2, 1)  # start-pose xy jitter draw (legged_robot.py:867), kept for RNG order
            if dr.randomize_base_mass:
                mass[i, 0] = np.random.uniform(dr.added_mass_range[0], dr.added_mass_range[1], size=(1,))[0]
            if getattr(dr, "randomize_center_of_mass", False):
                mass[i, 1:4] = np.random.uniform(dr.added_com_range[0], dr.added_com_range[1], size=(3,))
        self.privileged_mass_params = torch.from_numpy(mass[sl].copy()).to(self.device)
        names = self.body_names
        feet = [s for s in names if self.cfg.asset.foot_name in s]
        pen, term = [], []
        for key in self.cfg.asset.penalize_contacts_on:
            pen.extend([s for s in names if key in s])
        for key in self.cfg.asset.terminate_after_contacts_on:
            term.extend([s for s in names if key in s])
        idx = lambda lst: torch.tensor([names.index(s) for s in lst], dtype=torch.long, device=self.device)  # noqa: E731
        self.feet_indices = idx(feet)
        self.penalised_contact_indices = idx(pen)
        self.termination_contact_indices = idx(term)
        links = self.model_dict["links"][1:]
        self.dof_pos_limits = torch.from_numpy(prm.soft_dof_limits(
            [l["lower"] for l in links], [l["upper"] for l in links], self.cfg.rewards.soft_dof_pos_limit)).to(self.device)
        self.dof_vel_limits = torch.tensor([l["velocity"] for l in links], dtype=torch.float, device=self.device)
        self.torque_limits = torch.tensor([l["effort"] for l in links], dtype=torch.float, device=self.device)

    def _get_env_origins(self):
        """legged_robot.py:897-930. Rough terrain: origins from the terrain tiles
        (level = random up to max_init_terrain_level, type = global env index / (N / cols));
        plane: a grid with env_spacing. Both use the GLOBAL env index, and the level draw is
        made for all envs and sliced, so shards reproduce the single-GPU layout."""
        total, sl = self.num_envs_total, slice(self.env_id_offset, self.env_id_offset + self.num_envs)
        self.env_origins = torch.zeros(self.num_envs, 3, device=self.device)
        if self.cfg.terrain.mesh_type in ("heightfield", "trimesh"):
            self.custom_origins = True
            t = self.cfg.terrain
            max_init_level = t.max_init_terrain_level if t.curriculum else t.num_rows - 1
            if max_init_level >= t.num_rows:
                # the reference indexes terrain_origins out of bounds here (a device fault);
                # refuse the configuration up front instead
                raise ValueError(f"terrain.max_init_terrain_level ({max_init_level}) must be < terrain.num_rows "
                                 f"({t.num_rows})")
            self.max_terrain_level = t.num_rows
            self.terrain_levels = torch.randint(0, max_init_level + 1, (total,), device=self.device)[sl].contiguous()
            self.terrain_types = torch.div(torch.arange(total, device=self.device), (total / t.num_cols),
                                           rounding_mode="floor").to(torch.long)[sl].contiguous()
            self.terrain_origins = torch.from_numpy(self.terrain.env_origins).to(self.device).to(torch.float)
            self.env_origins[:] = self.terrain_origins[self.terrain_levels, self.terrain_types]
            return
        self.custom_origins = False
        num_cols = np.floor(np.sqrt(total))
        num_rows = np.ceil(total / num_cols)
        xx, yy = torch.meshgrid(torch.arange(num_rows), torch.arange(num_cols), indexing="ij")
        spacing = self.cfg.env.env_spacing
        self.env_origins[:, 0] = spacing * xx.flatten()[sl].to(self.device)
        self.env_origins[:, 1] = spacing * yy.flatten()[sl].to(self.device)

    def _parse_cfg(self, cfg):
        """legged_robot.py:933-955."""
        self.dt = self.cfg.control.decimation * self.sim_params.dt
        self.obs_scales = self.cfg.normalization.obs_scales
        self.reward_scales = class_to_dict(self.cfg.rewards.scales)
        self.command_ranges = class_to_dict(self.cfg.commands.ranges)
        if self.cfg.terrain.mesh_type not in ("heightfield", "trimesh"):
            self.cfg.terrain.curriculum = False
        self.max_episode_length_s = self.cfg.env.episode_length_s
        self.max_episode_length = np.ceil(self.max_episode_length_s / self.dt)
        self.cfg.domain_rand.push_interval = np.ceil(self.cfg.domain_rand.push_interval_s / self.dt)

    def _init_buffers(self):
        """legged_robot.py:625-727 (+ go2.py:132-177): torch-owned, env-major buffers,
        bound once to the native env."""
        n, d, nb, na = self.num_envs, self.num_dof, self.num_bodies, self.num_actions
        dev = self.device
        z = self._zeros
        self.root_states = z(n, 13)
        self.root_states[:] = self.base_init_state
        self.root_states[:, :3] += self.env_origins
        self._dof_state3 = z(n, d, 2)
        self.dof_state = self._dof_state3.view(n * d, 2)
        self.dof_pos = self._dof_state3[..., 0]
        self.dof_vel = self._dof_state3[..., 1]
        self.base_quat = self.root_states[:, 3:7]
        self._contact3 = z(n, nb, 3)
        self.contact_forces = self._contact3
        self.rigid_body_states = z(n * nb, 13)
        self.rigid_body_states_view = self.rigid_body_states.view(n, nb, 13)
        self._step_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.common_step_counter = 0
        self._reset_calls = 0
        self.extras = {}
        self.noise_scale_vec = torch.from_numpy(prm.noise_vector(self.cfg, self.TASK_KIND == _abi.TASK_GO2)).to(dev)
        self.add_noise = self.cfg.noise.add_noise
        self.gravity_vec = torch.tensor([0.0, 0.0, -1.0], device=dev).repeat((n, 1))
        self.forward_vec = torch.tensor([1.0, 0.0, 0.0], device=dev).repeat((n, 1))
        self.actions_in = z(n, na)
        self.actions = z(n, na)
        self.torques = z(n, na)
        self.last_actions = z(n, na)
        self.last_dof_vel = z(n, d)
        self.last_root_vel = z(n, 6)
        self.last_torques = z(n, na)
        self.commands = z(n, self.cfg.commands.num_commands)
        sc = self.obs_scales
        self.commands_scale = torch.tensor([sc.lin_vel, sc.lin_vel, sc.ang_vel], device=dev)
        self.base_lin_vel = z(n, 3)
        self.base_ang_vel = z(n, 3)
        self.projected_gravity = z(n, 3)
        self.projected_gravity[:, 2] = -1.0
        self.last_base_lin_vel = z(n, 3)
        xs, ys = self.cfg.terrain.measured_points_x, self.cfg.terrain.measured_points_y
        self.num_height_points = len(xs) * len(ys)
        self.measured_heights = z(n, self.num_height_points)
        self.obs_history_buf = z(n, self.cfg.env.history_buffer_length, self.cfg.env.num_proprio)
        self.rpy_phase = z(n, 8)
        self.roll, self.pitch, self.yaw = self.rpy_phase[:, 0], self.rpy_phase[:, 1], self.rpy_phase[:, 2]
        self.phase_fl, self.phase_fr = self.rpy_phase[:, 3], self.rpy_phase[:, 4]
        self.phase_bl, self.phase_br = self.rpy_phase[:, 5], self.rpy_phase[:, 6]
        self.jump_flags = self.rpy_phase[:, 7:8]
        nf = len(self.feet_indices)
        self.last_contacts = z(n, nf, dtype=torch.bool)
        self.last_contact_heights = z(n, nf)
        self.feet_air_time = z(n, nf)
        dr = self.cfg.domain_rand
        if dr.randomize_friction:
            self._friction = self.friction_coeffs.to(dev).to(torch.float).reshape(n).contiguous()
        else:
            self._friction = torch.ones(n, device=dev) * self.cfg.terrain.dynamic_friction
        self.privileged_friction_coeffs = self._friction.view(n, 1)
        lo, hi = getattr(dr, "kp_kd_range", [1.0, 1.0])
        self.kp_kd_multipliers = ((hi - lo) * torch.rand(2, self.num_envs_total, na, device=dev) + lo)[
            :, self.env_id_offset:self.env_id_offset + n].contiguous()
        if not getattr(dr, "randomize_kp_kd", False):
            self.kp_kd_multipliers.fill_(1.0)
        self._init_actuator_randomisation()  # after every existing setup draw: those keep their values
        self._init_sensor_model()  # after the actuator draws
        self.push_step = self.push_dvel = None  # scheduled pushes (ABI 9): no draw, off unless allocated
        if prm.scheduled_pushes(self.cfg):
            self._alloc_push_schedule()
        self.cmd_step = self.cmd_val = None  # command schedule (ABI 10): no draw, off unless allocated
        if prm.scheduled_commands(self.cfg):
            self._alloc_command_schedule()
        self._init_external_force()  # after every existing setup draw: those keep their values
        self._init_scan_model()      # and so do these, after the force's
        self.default_dof_pos = torch.tensor([self.cfg.init_state.default_joint_angles[nm] for nm in self.dof_names],
                                            device=dev).unsqueeze(0)
        self._dof_state3[..., 0] = self.default_dof_pos
        p_gains, d_gains = [], []
        for nm in self.dof_names:
            kp = kd = 0.0
            for key in self.cfg.control.stiffness.keys():
                if key in nm:
                    kp, kd = self.cfg.control.stiffness[key], self.cfg.control.damping[key]
            p_gains.append(kp)
            d_gains.append(kd)
        self.p_gains = torch.tensor(p_gains, device=dev)
        self.d_gains = torch.tensor(d_gains, device=dev)
        # ---- native env
        model_struct = mdl.to_struct(self.model_dict)
        terrain = getattr(self, "terrain", None)
        self.task_params = prm.build_task_params(self.cfg, self.model_dict, n, self.num_envs_total, self.env_id_offset,
                                                 sim_dt=self.sim_params.dt, go2=self.TASK_KIND == _abi.TASK_GO2,
                                                 terrain_shape=(terrain.tot_rows, terrain.tot_cols) if terrain else None)
        self._sea_buffers = self._setup_actuator(self.task_params)
        names, _, _, term = prm.reward_terms(self.cfg, self.dt)
        self._episode_keys = names + (["termination"] if term is not None else [])
        ks = len(self._episode_keys)
        self.episode_sums_buf = z(n, ks)
        self.episode_sums = {k: self.episode_sums_buf[:, i] for i, k in enumerate(self._episode_keys)}
        self.episode_stats = z(ks + 1)
        # extras['episode'] values in key order in one buffer (the runner's native episode
        # tracking reads them as contiguous runs): rew_* means | terrain_level | command range log
        self._extras_vals = z(ks + 1 + 4)
        self._episode_means = self._extras_vals[:ks]
        self._terrain_level_mean = self._extras_vals[ks]
        self._command_range_log = self._extras_vals[ks + 1:]
        self._extras_time_outs = z(n, dtype=torch.bool)
        # command curriculum (go2.py:80-107 / legged_robot.py:580-591): the ranges are device
        # state (double, the reference's Python floats) updated by lgx_command_curriculum
        self._cmd_curriculum = bool(getattr(self.cfg.commands, "curriculum", False))
        self._command_ranges_buf = self._curriculum_vals = None
        if self._cmd_curriculum:
            r = self.cfg.commands.ranges
            self._command_ranges_buf = torch.tensor(list(r.lin_vel_x) + list(r.lin_vel_y) + list(r.ang_vel_yaw) +
                                                    list(r.heading), dtype=torch.float64, device=dev)
            self._curriculum_vals = z(n)
            go2 = self.TASK_KIND == _abi.TASK_GO2
            log = ([r.lin_vel_x[1], r.lin_vel_x[0], r.lin_vel_y[1], r.ang_vel_yaw[1]] if go2
                   else [r.lin_vel_x[1], r.lin_vel_y[1], r.ang_vel_yaw[1], 0.0])
            self._command_range_log.copy_(torch.tensor(log, dtype=torch.float32))
            self.command_ranges = _DeviceCommandRanges(self._command_ranges_buf)
        # NaN/Inf guard outputs (lgx_buffers.blew_up / blowup_count): per step, the envs whose
        # physics state went non-finite (given a finite stand-in state and reset); the count
        self.blew_up_buf = z(n, dtype=torch.bool)
        self._blowup_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self._native = _native.NativeEnv(model_struct, self.task_params, self.sim_device_id)
        self._bind()

    def _bind(self):
        self._native.bind({
            "root_states": self.root_states, "dof_state": self._dof_state3, "contact_forces": self._contact3,
            "rigid_body_states": self.rigid_body_states, "actions_in": self.actions_in, "actions": self.actions,
            "torques": self.torques, "last_actions": self.last_actions, "last_dof_vel": self.last_dof_vel,
            "last_root_vel": self.last_root_vel, "last_base_lin_vel": self.last_base_lin_vel,
            "last_torques": self.last_torques, "commands": self.commands,
            "episode_length": self._episode_length_buf, "episode_sums": self.episode_sums_buf,
            "obs_history": self.obs_history_buf, "last_contacts": self.last_contacts,
            "last_contact_heights": self.last_contact_heights, "feet_air_time": self.feet_air_time,
            "obs": self.obs_buf, "priv": self.privileged_obs_buf if self.num_privileged_obs else None,
            "critic": self.critic_obs_buf, "est": self.estimated_obs_buf if self.num_estimated_obs else None,
            "scan": self.scan_obs_buf if self.num_scan_obs else None, "rew": self.rew_buf, "reset": self.reset_buf,
            "time_out": self.time_out_buf, "base_lin_vel": self.base_lin_vel, "base_ang_vel": self.base_ang_vel,
            "projected_gravity": self.projected_gravity, "rpy_phase": self.rpy_phase,
            "measured_heights": self.measured_heights, "friction": self._friction,
            "mass_params": self.privileged_mass_params, "kp_kd": self.kp_kd_multipliers,
            "env_origins": self.env_origins, "episode_stats": self.episode_stats,
            "terrain_levels": getattr(self, "terrain_levels", None), "terrain_types": getattr(self, "terrain_types", None),
            "terrain_origins": getattr(self, "terrain_origins", None), "height_samples": self.height_samples,
            "terrain_mesh": self._terrain_mesh, "blew_up": self.blew_up_buf, "blowup_count": self._blowup_count,
            "command_ranges": self._command_ranges_buf, "curriculum_vals": self._curriculum_vals,
            "command_range_log": self._command_range_log if self._cmd_curriculum else None,
            "action_delay": self.action_delay_substeps, "action_history": self.action_history,
            "motor_strength": self.motor_strengths,
            "push_step": self.push_step, "push_dvel": self.push_dvel,
            "cmd_step": self.cmd_step, "cmd_val": self.cmd_val,
            "obs_noise_scale": self.obs_noise_scales, "obs_bias": self.obs_biases, "obs_delay": self.obs_delay_steps,
            "sensor_history": self.sensor_history, "sensor_count": self.sensor_count,
            "force_window": self.force_window, "force_vec": self.force_vec,
            "scan_noise": self.scan_noise_amps, "scan_dropout": self.scan_dropouts, "scan_offset": self.scan_offsets,
            "scan_delay": self.scan_delay_steps, "scan_history": self.scan_history,
            **self._sea_buffers,
        })

    # ------------------------------------------------------------------ actuator randomisation
    def _init_actuator_randomisation(self):
        """Actuation latency and motor strength (include/lgx.h ABI 8; domain_rand keys of
        params.actuator_randomisation). Buffers exist, and are bound, only when a feature is on or
        max_action_delay_s > 0; otherwise the three attributes are None and the step is the ideal
        actuator's. Draws only for an enabled feature, for all global envs and sliced as
        kp_kd_multipliers is, fixed per env: d_e = round(U(lo, hi) / sim_dt) physics substeps, one
        strength per env and joint."""
        n, na, d, dev = self.num_envs, self.num_actions, self.num_dof, self.device
        total, sl = self.num_envs_total, slice(self.env_id_offset, self.env_id_offset + self.num_envs)
        ar = prm.actuator_randomisation(self.cfg, self.sim_params.dt)
        self._action_history_len = H = ar["history_len"]
        self._action_delay_capacity = H * int(self.cfg.control.decimation)  # substeps
        self.action_delay_substeps = self.action_history = self.motor_strengths = None
        self._captured = False
        if H > 0:
            self.action_delay_substeps = torch.zeros(n, dtype=torch.int32, device=dev)
            self.action_history = torch.zeros(n, H, na, device=dev)
        if ar["delay_on"] and H > 0:  # (a range of [0, 0] s needs no history: nothing to draw)
            lo, hi = ar["delay_range_s"]
            delay_s = ((hi - lo) * torch.rand(total, device=dev) + lo)[sl]
            self.set_action_delay(delay_s)
        if ar["strength_on"]:
            lo, hi = ar["strength_range"]
            self.motor_strengths = ((hi - lo) * torch.rand(total, d, device=dev) + lo)[sl].contiguous()

    def set_action_delay(self, seconds):
        """Actuation latency of every env: a number of seconds or a tensor [num_envs] of seconds, rounded
        to physics substeps (round(s / sim_dt)). Written in place (a captured graph keeps replaying
        on the same address). ValueError when negative, or beyond the capacity the env was built
        with (domain_rand.max_action_delay_s)."""
        if self.action_delay_substeps is None:
            raise ValueError("this env was built without actuation latency support: set "
                             "domain_rand.max_action_delay_s (or randomize_action_delay) in its config")
        s = torch.as_tensor(seconds, dtype=torch.float64, device=self.device)
        if s.dim() not in (0, 1) or (s.dim() == 1 and s.shape[0] != self.num_envs):
            raise ValueError(f"action delay: a number or a tensor [{self.num_envs}], got shape {list(s.shape)}")
        sub = torch.round(s / float(self.sim_params.dt))
        lo, hi = float(sub.min()), float(sub.max())
        if not (lo >= 0.0 and hi <= self._action_delay_capacity):  # also refuses NaN
            raise ValueError(f"action delay of {lo:g}..{hi:g} physics substeps is outside 0..{self._action_delay_capacity} "
                             f"(capacity: {self._action_history_len} control steps, domain_rand.max_action_delay_s)")
        self.action_delay_substeps.copy_(sub.to(torch.int32).expand(self.num_envs))

    def set_motor_strength(self, value):
        """Motor strength factors: a number, or a tensor [num_envs] or [num_envs, num_dof]. Written
        in place once the buffer exists; the first call on an env built without
        randomize_motor_strength allocates it and re-binds, which a captured graph of this env's
        step would not see: RuntimeError once a step of this env has been captured (build the env
        with randomize_motor_strength, or set a strength before the capture).
        ValueError when negative or not finite."""
        v = torch.as_tensor(value, dtype=torch.float32, device=self.device)
        if v.dim() == 1 and v.shape[0] == self.num_envs:
            v = v.unsqueeze(1)
        if v.dim() not in (0, 2) or (v.dim() == 2 and tuple(v.shape) not in ((self.num_envs, 1), (self.num_envs, self.num_dof))):
            raise ValueError(f"motor strength: a number or a tensor [{self.num_envs}] or [{self.num_envs}, {self.num_dof}], "
                             f"got shape {list(v.shape)}")
        if not bool(torch.isfinite(v).all()) or float(v.min()) < 0.0:
            raise ValueError("motor strength factors must be finite and >= 0")
        if self.motor_strengths is None:
            if self._captured:
                raise RuntimeError("set_motor_strength: this env has no motor_strength buffer and its step has been captured "
                                   "in a graph, which would go on replaying the old binding; build the env with "
                                   "domain_rand.randomize_motor_strength or set a strength before the capture")
            self.motor_strengths = torch.ones(self.num_envs, self.num_dof, device=self.device)
            self._bind()
        self.motor_strengths.copy_(v.expand(self.num_envs, self.num_dof))

    # ------------------------------------------------------------------ sensor model
    def _init_sensor_model(self):
        """Per-env observation noise level, bias and sensing latency (include/lgx.h ABI 15;
        domain_rand keys of params.sensor_model). obs_delay_steps, sensor_history and sensor_count
        exist, and are bound, when max_obs_delay_s gives K > 0 control steps; obs_noise_scales and
        obs_biases when their randomisation or domain_rand.sensor_model is on (or after their
        setter's first call). Otherwise the attributes are None and the step is that of ABI 14.
        Draws only for an enabled feature, after the actuator draws, for all global envs and
        sliced by rank, fixed per env: one scale U(lo, hi), one offset per sensor channel uniform in
        +-level * sensor_amplitudes with level U(lo, hi) per env, one latency round(U(lo, hi) / dt)."""
        n, p, dev = self.num_envs, int(self.cfg.env.num_proprio), self.device
        total, sl = self.num_envs_total, slice(self.env_id_offset, self.env_id_offset + self.num_envs)
        sm = prm.sensor_model(self.cfg, self.dt)
        go2 = self.TASK_KIND == _abi.TASK_GO2
        self._sensor_history_len = K = sm["history_len"]
        self._obs_groups = prm.proprio_channel_groups(self.cfg, go2)
        self.sensor_amplitudes = torch.from_numpy(prm.sensor_amplitudes(self.cfg, go2)).to(dev)
        self.obs_noise_scales = self.obs_biases = self.obs_delay_steps = self.sensor_history = self.sensor_count = None
        if sm["on"] or sm["scale_on"]:
            self.obs_noise_scales = torch.ones(n, device=dev)
        if sm["on"] or sm["bias_on"]:
            self.obs_biases = torch.zeros(n, p, device=dev)
        if K > 0:  # (K covers the scan model's latency too: the proprio ring then exists beside the scan's)
            self.obs_delay_steps = torch.zeros(n, dtype=torch.int32, device=dev)
            self.sensor_history = torch.zeros(n, K, p, device=dev)
            self.sensor_count = torch.zeros(n, dtype=torch.int32, device=dev)
        if sm["scale_on"]:
            lo, hi = sm["scale_range"]
            self.set_obs_noise_scale(((hi - lo) * torch.rand(total, device=dev) + lo)[sl])
        if sm["bias_on"]:
            lo, hi = sm["bias_level_range"]
            level = (hi - lo) * torch.rand(total, 1, device=dev) + lo
            r = 2.0 * torch.rand(total, p, device=dev) - 1.0
            self.set_obs_bias((level * r * self.sensor_amplitudes)[sl])
        if sm["delay_on"] and K > 0:  # (a range of [0, 0] s needs no ring: nothing to draw)
            lo, hi = sm["delay_range_s"]
            self.set_obs_delay(((hi - lo) * torch.rand(total, device=dev) + lo)[sl])

    def _sensor_alloc(self, name, what, make, key="sensor_model"):
        """The first call of a sensor setter on an env built without its buffer: allocate, re-bind."""
        if self._captured:
            raise RuntimeError(f"{what}: this env has no {name} buffer and its step has been captured in a graph, "
                               "which would go on replaying the old binding; build the env with "
                               f"domain_rand.{key} or call {what} before the capture")
        setattr(self, name, make())
        self._bind()

    def set_obs_noise_scale(self, value):
        """Observation-noise level of every env: a number or a tensor [num_envs] that multiplies the
        config's noise amplitude (noise.add_noise decides whether there is noise at all). Written in
        place once the buffer exists; the first call on an env built without it allocates and
        re-binds: RuntimeError once a step of this env has been captured. ValueError when negative
        or not finite."""
        v = torch.as_tensor(value, dtype=torch.float32, device=self.device)
        if v.dim() not in (0, 1) or (v.dim() == 1 and v.shape[0] != self.num_envs):
            raise ValueError(f"obs noise scale: a number or a tensor [{self.num_envs}], got shape {list(v.shape)}")
        if not bool(torch.isfinite(v).all()) or float(v.min()) < 0.0:
            raise ValueError("obs noise scales must be finite and >= 0")
        if self.obs_noise_scales is None:
            self._sensor_alloc("obs_noise_scales", "set_obs_noise_scale", lambda: torch.ones(self.num_envs, device=self.device))
        self.obs_noise_scales.copy_(v.expand(self.num_envs))

    def set_obs_bias(self, bias):
        """Constant observation offsets in observation units: a tensor [num_proprio] or
        [num_envs, num_proprio] (obs_bias_from_physical builds one from physical units). Written in
        place once the buffer exists; the first call on an env built without it allocates and
        re-binds: RuntimeError once a step of this env has been captured. ValueError for a wrong
        shape or a non-finite entry."""
        n, p = self.num_envs, int(self.cfg.env.num_proprio)
        b = torch.as_tensor(bias, dtype=torch.float32, device=self.device)
        if tuple(b.shape) not in ((p,), (n, p)):
            raise ValueError(f"obs bias: a tensor [{p}] or [{n}, {p}], got shape {list(b.shape)}")
        if not bool(torch.isfinite(b).all()):
            raise ValueError("obs bias must be finite")
        if self.obs_biases is None:
            self._sensor_alloc("obs_biases", "set_obs_bias", lambda: torch.zeros(n, p, device=self.device))
        self.obs_biases.copy_(b.expand(n, p))

    def set_obs_delay(self, seconds):
        """Sensing latency of every env: a number of seconds or a tensor [num_envs] of seconds, rounded
        to control steps (round(s / dt)). Written in place (a captured graph keeps replaying on the
        same address). ValueError when negative, or beyond the capacity the env was built with
        (domain_rand.max_obs_delay_s)."""
        if self.obs_delay_steps is None:
            raise ValueError("this env was built without sensing latency support: set "
                             "domain_rand.max_obs_delay_s (or randomize_obs_delay) in its config")
        s = torch.as_tensor(seconds, dtype=torch.float64, device=self.device)
        if s.dim() not in (0, 1) or (s.dim() == 1 and s.shape[0] != self.num_envs):
            raise ValueError(f"obs delay: a number or a tensor [{self.num_envs}], got shape {list(s.shape)}")
        st = torch.round(s / float(self.dt))
        lo, hi = float(st.min()), float(st.max())
        if not (lo >= 0.0 and hi <= self._sensor_history_len):  # also refuses NaN
            raise ValueError(f"obs delay of {lo:g}..{hi:g} control steps is outside 0..{self._sensor_history_len} "
                             "(capacity: domain_rand.max_obs_delay_s)")
        self.obs_delay_steps.copy_(st.to(torch.int32).expand(self.num_envs))

    def obs_channel_groups(self):
        """name -> slice of the current-observation (proprio) row, from the task's layout
        (params.go2_proprio_layout / legged_proprio_layout)."""
        return dict(self._obs_groups)

    def obs_bias_from_physical(self, **groups):
        """[num_envs, num_proprio] in observation units from physical offsets per sensor group
        (ang_vel, roll_pitch, gravity, lin_vel, dof_pos, dof_vel, heights; those the task has): each a
        number, a tensor [width] or [num_envs, width], times the group's observation scale.
        ValueError for a group the task does not measure, a wrong shape or a non-finite entry."""
        n, p = self.num_envs, int(self.cfg.env.num_proprio)
        out = torch.zeros(n, p, device=self.device)
        for name, value in groups.items():
            if name not in prm.SENSOR_GROUPS or name not in self._obs_groups:
                known = [g for g in self._obs_groups if g in prm.SENSOR_GROUPS]
                raise ValueError(f"obs bias: '{name}' is not a sensor group of this task (it has {known})")
            sl = self._obs_groups[name]
            w = sl.stop - sl.start
            v = torch.as_tensor(value, dtype=torch.float32, device=self.device)
            if tuple(v.shape) not in ((), (w,), (n, w)):
                raise ValueError(f"obs bias {name}: a number or a tensor [{w}] or [{n}, {w}], got shape {list(v.shape)}")
            if not bool(torch.isfinite(v).all()):
                raise ValueError(f"obs bias {name} must be finite")
            out[:, sl] = v * prm.sensor_obs_scale(self.cfg, name)
        return out

    # ------------------------------------------------------------------ height-scan model
    def _init_scan_model(self):
        """Per-env height-scan model (include/lgx.h ABI 17; domain_rand keys of params.scan_model):
        noise, dropout, map offset and latency on the Go2 task kind's scan_obs_buf. scan_noise_amps
        [N], scan_dropouts [N, 2] (probability, value) and scan_offsets [N, 3] exist, and are bound,
        when their randomisation or domain_rand.scan_model is on (or after their setter's first
        call); scan_delay_steps [N] and scan_history [N, K, S] when max_scan_delay_s gives a
        capacity. Otherwise the attributes are None and the step is that of ABI 16. Draws only for
        an enabled feature, after every other setup draw, for all global envs and sliced by rank,
        fixed per env: an amplitude U(lo, hi) m, a probability U(lo, hi), a shift of length
        U(lo, hi) m in a direction uniform on the circle with dz U(lo, hi) m, a latency
        round(U(lo, hi) / dt)."""
        n, dev = self.num_envs, self.device
        total, sl = self.num_envs_total, slice(self.env_id_offset, self.env_id_offset + self.num_envs)
        sc = prm.scan_model(self.cfg, self.dt)
        S = int(self.num_scan_obs) if self.TASK_KIND == _abi.TASK_GO2 else 0
        self.scan_noise_amps = self.scan_dropouts = self.scan_offsets = self.scan_delay_steps = self.scan_history = None
        self._scan_points = S
        self._scan_dropout_value = sc["dropout_value"]
        self._scan_delay_cap = sc["delay_steps"] if S > 0 else 0
        if sc["any"] and S <= 0:
            raise ValueError("domain_rand: the scan model needs a task with a height scan (Go2 task kind, num_scan_obs > 0)")
        if S <= 0:
            return
        if sc["on"] or sc["noise_on"]:
            self.scan_noise_amps = torch.zeros(n, device=dev)
        if sc["on"] or sc["dropout_on"]:
            self.scan_dropouts = self._neutral_scan_dropout()
        if sc["on"] or sc["offset_on"]:
            self.scan_offsets = torch.zeros(n, 3, device=dev)
        if sc["delay_steps"] > 0:
            self.scan_delay_steps = torch.zeros(n, dtype=torch.int32, device=dev)
            self.scan_history = torch.zeros(n, self._sensor_history_len, S, device=dev)
        u = lambda r, *shape: (r[1] - r[0]) * torch.rand(total, *shape, device=dev) + r[0]  # noqa: E731
        if sc["noise_on"]:
            self.set_scan_noise(u(sc["noise_range"])[sl])
        if sc["dropout_on"]:
            self.set_scan_dropout(u(sc["dropout_range"])[sl], sc["dropout_value"])
        if sc["offset_on"]:
            r, th = u(sc["offset_xy_range"]), 2.0 * math.pi * torch.rand(total, device=dev)
            dz = u(sc["offset_z_range"])
            self.set_scan_offset((r * torch.cos(th))[sl], (r * torch.sin(th))[sl], dz[sl])
        if sc["delay_on"] and sc["delay_steps"] > 0:
            self.set_scan_delay(u(sc["delay_range_s"])[sl])

    def _neutral_scan_dropout(self):
        d = torch.zeros(self.num_envs, 2, device=self.device)
        d[:, 1] = self._scan_dropout_value
        return d

    def _scan_per_env(self, what, value, lo=None, hi=None):
        """A number or a tensor [num_envs] -> float32 [num_envs] on the device; ValueError otherwise."""
        if self._scan_points <= 0:
            raise ValueError(f"{what}: this task has no height scan (Go2 task kind, num_scan_obs > 0)")
        v = torch.as_tensor(value, dtype=torch.float32, device=self.device)
        if v.dim() not in (0, 1) or (v.dim() == 1 and v.shape[0] != self.num_envs):
            raise ValueError(f"{what}: a number or a tensor [{self.num_envs}], got shape {list(v.shape)}")
        if not bool(torch.isfinite(v).all()) or (lo is not None and float(v.min()) < lo) or \
                (hi is not None and float(v.max()) > hi):
            raise ValueError(f"{what}: finite values" + (f" in [{lo:g}, {hi if hi is not None else math.inf:g}]"
                                                          if lo is not None else ""))
        return v.expand(self.num_envs)

    def set_scan_noise(self, m):
        """Scan noise of every env: a number or a tensor [num_envs], the amplitude in m of uniform
        noise per scan point and step (0: none). Written in place once the buffer exists; the first
        call on an env built without it allocates and re-binds: RuntimeError once a step of this
        env has been captured. ValueError when negative or not finite."""
        v = self._scan_per_env("set_scan_noise", m, 0.0)
        if self.scan_noise_amps is None:
            self._sensor_alloc("scan_noise_amps", "set_scan_noise", lambda: torch.zeros(self.num_envs, device=self.device),
                               key="scan_model")
        self.scan_noise_amps.copy_(v)

    def set_scan_dropout(self, p, value=1.0):
        """Scan dropout of every env: p, a number or a tensor [num_envs], the probability that a
        scan point is lost in a step, and the value a lost point reads (a number or [num_envs],
        |value| <= 1; 1.0: no return, far). In place / first call as set_scan_noise."""
        pv = self._scan_per_env("set_scan_dropout", p, 0.0, 1.0)
        fv = self._scan_per_env("set_scan_dropout value", value, -1.0, 1.0)
        if self.scan_dropouts is None:
            self._sensor_alloc("scan_dropouts", "set_scan_dropout", self._neutral_scan_dropout, key="scan_model")
        self.scan_dropouts[:, 0].copy_(pv)
        self.scan_dropouts[:, 1].copy_(fv)

    def set_scan_offset(self, dx, dy, dz=0.0):
        """Map misregistration of every env: the scan is taken at the scan points shifted by (dx, dy)
        m in the robot's yaw frame, and dz m is added to every point. Each a number or a tensor
        [num_envs]. In place / first call as set_scan_noise."""
        vs = [self._scan_per_env("set_scan_offset", v) for v in (dx, dy, dz)]
        if self.scan_offsets is None:
            self._sensor_alloc("scan_offsets", "set_scan_offset", lambda: torch.zeros(self.num_envs, 3, device=self.device),
                               key="scan_model")
        for j, v in enumerate(vs):
            self.scan_offsets[:, j].copy_(v)

    def set_scan_delay(self, seconds):
        """Latency of every env's scan: a number of seconds or a tensor [num_envs], rounded to control
        steps. Written in place. ValueError when negative, or beyond the capacity the env was built
        with (domain_rand.max_scan_delay_s)."""
        if self.scan_delay_steps is None:
            raise ValueError("this env was built without scan latency support: set "
                             "domain_rand.max_scan_delay_s (or randomize_scan_delay) in its config")
        s = torch.as_tensor(seconds, dtype=torch.float64, device=self.device)
        if s.dim() not in (0, 1) or (s.dim() == 1 and s.shape[0] != self.num_envs):
            raise ValueError(f"scan delay: a number or a tensor [{self.num_envs}], got shape {list(s.shape)}")
        st = torch.round(s / float(self.dt))
        lo, hi = float(st.min()), float(st.max())
        if not (lo >= 0.0 and hi <= self._scan_delay_cap):  # also refuses NaN
            raise ValueError(f"scan delay of {lo:g}..{hi:g} control steps is outside 0..{self._scan_delay_cap} "
                             "(capacity: domain_rand.max_scan_delay_s)")
        self.scan_delay_steps.copy_(st.to(torch.int32).expand(self.num_envs))

    # ------------------------------------------------------------------ scheduled pushes
    def _alloc_push_schedule(self):
        self.push_step = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self.push_dvel = torch.zeros(self.num_envs, 3, device=self.device)

    def set_push_schedule(self, step, dvel):
        """Scheduled pushes (include/lgx.h ABI 9): env e gets the velocity impulse dvel[e] = (forward,
        left in m/s in its heading frame, yaw rate in rad/s) in the step in which its episode length
        becomes step[e]; a step <= 0 means never. step: an int or an int tensor [num_envs]; dvel: [3]
        or [num_envs, 3]. Written in place once the buffers exist; the first call on an env built
        without domain_rand.scheduled_pushes allocates them and re-binds, which a captured graph of
        this env's step would not see: RuntimeError once a step of this env has been captured.
        ValueError for wrong shapes, a non-finite dvel or a step beyond max_episode_length."""
        n = self.num_envs
        st = torch.as_tensor(step, device=self.device)
        if st.dtype.is_floating_point or st.dtype == torch.bool or st.dim() not in (0, 1) or \
                (st.dim() == 1 and st.shape[0] != n):
            raise ValueError(f"push step: an int or an int tensor [{n}], got {st.dtype} of shape {list(st.shape)}")
        dv = torch.as_tensor(dvel, dtype=torch.float32, device=self.device)
        if tuple(dv.shape) not in ((3,), (n, 3)):
            raise ValueError(f"push dvel: a tensor [3] or [{n}, 3], got shape {list(dv.shape)}")
        if not bool(torch.isfinite(dv).all()):
            raise ValueError("push dvel must be finite")
        if int(st.max()) > int(self.max_episode_length):
            raise ValueError(f"push step {int(st.max())} is beyond max_episode_length = {int(self.max_episode_length)}")
        if self.push_step is None:
            if self._captured:
                raise RuntimeError("set_push_schedule: this env has no push buffers and its step has been captured in "
                                   "a graph, which would go on replaying the old binding; build the env with "
                                   "domain_rand.scheduled_pushes or set a schedule before the capture")
            self._alloc_push_schedule()
            self._bind()
        self.push_step.copy_(st.to(torch.int32).expand(n))
        self.push_dvel.copy_(dv.expand(n, 3))

    def clear_push_schedule(self):
        """No env is pushed: push_step zeroed in place (a no-op on an env without the buffers)."""
        if self.push_step is not None:
            self.push_step.zero_()

    # ------------------------------------------------------------------ command schedule
    def _alloc_command_schedule(self):
        self.cmd_step = torch.full((self.num_envs, _abi.CMD_SEGMENTS), -1, dtype=torch.int32, device=self.device)
        self.cmd_val = torch.zeros(self.num_envs, _abi.CMD_SEGMENTS, 4, device=self.device)

    def set_command_schedule(self, steps, values):
        """Command schedule (include/lgx.h ABI 10): from the step in which its episode length
        reaches steps[e][k], and after every reset for a segment that starts at step 0, env e holds
        the command values[e][k] = (vx, vy, yaw rate, heading) exactly, until its next segment
        starts; no resample, heading rule or curriculum redraw changes it. steps: int [K'] or
        [num_envs, K'], non-decreasing along K', each in 0 <= step < max_episode_length; values:
        [K', 4] or [num_envs, K', 4]; K' <= 4, the unused entries are padded with -1. Written in
        place once the buffers exist; the first call on an env built without
        commands.scheduled_commands allocates them and re-binds, which a captured graph of this
        env's step would not see: RuntimeError once a step of this env has been captured.
        ValueError for wrong shapes, non-finite values, decreasing steps or a step out of range."""
        n, K = self.num_envs, _abi.CMD_SEGMENTS
        st = torch.as_tensor(steps, device=self.device)
        if st.dtype.is_floating_point or st.dtype == torch.bool or st.dim() not in (1, 2) or \
                not 1 <= st.shape[-1] <= K or (st.dim() == 2 and st.shape[0] != n):
            raise ValueError(f"command schedule steps: an int tensor [K'] or [{n}, K'] with 1 <= K' <= {K}, got "
                             f"{st.dtype} of shape {list(st.shape)}")
        kk = int(st.shape[-1])
        val = torch.as_tensor(values, dtype=torch.float32, device=self.device)
        if tuple(val.shape) not in ((kk, 4), (n, kk, 4)):
            raise ValueError(f"command schedule values: a tensor [{kk}, 4] or [{n}, {kk}, 4], got shape {list(val.shape)}")
        if not bool(torch.isfinite(val).all()):
            raise ValueError("command schedule values must be finite")
        if int(st.min()) < 0 or int(st.max()) >= int(self.max_episode_length):
            raise ValueError(f"command schedule steps must lie in 0 <= step < max_episode_length = "
                             f"{int(self.max_episode_length)} (got {int(st.min())}..{int(st.max())})")
        if kk > 1 and bool((st[..., 1:] < st[..., :-1]).any()):
            raise ValueError("command schedule steps must not decrease")
        if self.cmd_step is None:
            if self._captured:
                raise RuntimeError("set_command_schedule: this env has no command schedule buffers and its step has "
                                   "been captured in a graph, which would go on replaying the old binding; build the "
                                   "env with commands.scheduled_commands or set a schedule before the capture")
            self._alloc_command_schedule()
            self._bind()
        self.cmd_step[:, :kk].copy_(st.to(torch.int32).expand(n, kk))
        self.cmd_step[:, kk:].fill_(-1)
        self.cmd_val[:, :kk].copy_(val.expand(n, kk, 4))

    def clear_command_schedule(self):
        """No env is scheduled: cmd_step filled with -1 in place (a no-op on an env without the
        buffers). The commands an env holds stay until its next resample or reset."""
        if self.cmd_step is not None:
            self.cmd_step.fill_(-1)

    # ------------------------------------------------------------------ external force
    def _init_external_force(self):
        """Sustained external force on the base (include/lgx.h ABI 16; domain_rand keys of
        params.external_force). The buffers exist, and are bound, when scheduled_forces or
        randomize_external_force is on (or after set_force_schedule's first call); otherwise both
        attributes are None and the step is that of ABI 15. The randomisation draws after every
        other setup draw, for all global envs and sliced by rank, fixed per env: a horizontal
        direction uniform on the circle, a magnitude U(lo, hi) N at the base origin, lasting `steps`
        of every `period` control steps from the start 1 + floor(U * period), so the envs are out
        of phase."""
        dev = self.device
        total, sl = self.num_envs_total, slice(self.env_id_offset, self.env_id_offset + self.num_envs)
        ef = prm.external_force(self.cfg, self.dt)
        self.force_window = self.force_vec = None
        if ef["alloc"]:
            self._alloc_force_schedule()
        if ef["on"]:
            lo, hi = ef["range_n"]
            theta = 2.0 * math.pi * torch.rand(total, device=dev)
            mag = (hi - lo) * torch.rand(total, device=dev) + lo
            start = 1 + torch.floor(torch.rand(total, device=dev) * ef["period"]).to(torch.int64).clamp_(max=ef["period"] - 1)
            force = torch.stack([mag * torch.cos(theta), mag * torch.sin(theta), torch.zeros_like(mag)], dim=1)
            self.set_force_schedule(start[sl], force[sl], steps=ef["steps"], period=ef["period"])

    def _alloc_force_schedule(self):
        self.force_window = torch.zeros(self.num_envs, 3, dtype=torch.int32, device=self.device)
        self.force_vec = torch.zeros(self.num_envs, 6, device=self.device)

    def set_force_schedule(self, start, force, steps=None, period=0, point=(0.0, 0.0, 0.0)):
        """External force on the base (include/lgx.h ABI 16): from the step in which its episode
        length becomes start[e], env e's base link takes force[e] = (forward, left in its heading
        frame, up along world z) in N at point[e] (m, base link frame) in every substep of `steps`
        control steps (None: to the end of the episode); with period >= 1 the window repeats every
        `period` steps. A start <= 0 means never. start, steps, period: ints or int tensors
        [num_envs]; force, point: [3] or [num_envs, 3]. Written in place once the buffers exist; the
        first call on an env built without domain_rand.scheduled_forces allocates them and re-binds,
        which a captured graph of this env's step would not see: RuntimeError once a step of this
        env has been captured. ValueError for wrong shapes, non-finite values, steps < 1,
        period < 0 or a start beyond max_episode_length."""
        n, i32max = self.num_envs, 2 ** 31 - 1

        def ints(v, what):
            t = torch.as_tensor(v, device=self.device)
            if t.dtype.is_floating_point or t.dtype == torch.bool or t.dim() not in (0, 1) or \
                    (t.dim() == 1 and t.shape[0] != n):
                raise ValueError(f"force {what}: an int or an int tensor [{n}], got {t.dtype} of shape {list(t.shape)}")
            return t.to(torch.int64)

        def vec3(v, what):
            t = torch.as_tensor(v, dtype=torch.float32, device=self.device)
            if tuple(t.shape) not in ((3,), (n, 3)):
                raise ValueError(f"force {what}: a tensor [3] or [{n}, 3], got shape {list(t.shape)}")
            if not bool(torch.isfinite(t).all()):
                raise ValueError(f"force {what} must be finite")
            return t

        st, pe = ints(start, "start"), ints(period, "period")
        sp = ints(i32max if steps is None else steps, "steps")
        fv, pt = vec3(force, "vector"), vec3(point, "point")
        if int(sp.min()) < 1 or int(sp.max()) > i32max:
            raise ValueError(f"force steps must lie in 1..{i32max} (None: to the end of the episode)")
        if int(pe.min()) < 0 or int(pe.max()) > i32max:
            raise ValueError(f"force period must lie in 0..{i32max} (0: the window does not repeat)")
        if int(st.max()) > int(self.max_episode_length) or int(st.min()) < -i32max:
            raise ValueError(f"force start {int(st.max())} is beyond max_episode_length = {int(self.max_episode_length)}")
        if self.force_window is None:
            if self._captured:
                raise RuntimeError("set_force_schedule: this env has no force buffers and its step has been captured in "
                                   "a graph, which would go on replaying the old binding; build the env with "
                                   "domain_rand.scheduled_forces or set a schedule before the capture")
            self._alloc_force_schedule()
            self._bind()
        self.force_window[:, 0].copy_(st.to(torch.int32).expand(n))
        self.force_window[:, 1].copy_(sp.to(torch.int32).expand(n))
        self.force_window[:, 2].copy_(pe.to(torch.int32).expand(n))
        self.force_vec[:, :3].copy_(fv.expand(n, 3))
        self.force_vec[:, 3:].copy_(pt.expand(n, 3))

    def clear_force_schedule(self):
        """No env is forced: the starts zeroed in place (a no-op on an env without the buffers)."""
        if self.force_window is not None:
            self.force_window[:, 0].zero_()

    @property
    def physics_blowups(self):
        """Number of env steps whose physics went non-finite since creation (host sync)."""
        return int(self._blowup_count.item())

    def _setup_actuator(self, P):
        """PD control (legged_robot.py:440-478) lives in the kernel; subclasses with an
        actuator network fill P.sea_* and return its state buffers (anymal.py)."""
        return {}

    def _prepare_reward_function(self):
        """legged_robot.py:730-754: nonzero scales x dt, alphabetical; the terms run in
        the kernel (params.reward_terms validates that each one is implemented)."""
        for key in list(self.reward_scales.keys()):
            if self.reward_scales[key] == 0:
                self.reward_scales.pop(key)
            else:
                self.reward_scales[key] *= self.dt
        self.reward_names = [k for k in self.reward_scales if k != "termination"]


class _RangePair(list):
    """One [lo, hi] entry of _DeviceCommandRanges: item writes go through to the device ranges
    (the reference idiom `self.command_ranges["lin_vel_x"][1] = v`, go2.py:96-107)."""

    def __init__(self, owner, key, vals):
        super().__init__(vals)
        self._owner, self._key = owner, key

    def __setitem__(self, i, v):
        super().__setitem__(i, v)
        if len(self) != 2:
            raise ValueError("a command range is [lo, hi]")
        self._owner[self._key] = list(self)

    def __reduce__(self):  # a detached copy pickles as the plain [lo, hi] list
        return (list, (list(self),))


class _DeviceCommandRanges(dict):
    """self.command_ranges under the command curriculum: {'lin_vel_x': [lo, hi], ...} read
    from the device ranges the curriculum updates. Every read is a device-to-host copy (it
    synchronises with the stream); item writes, whole or per end, go to the device."""
    _KEYS = ("lin_vel_x", "lin_vel_y", "ang_vel_yaw", "heading")

    def __init__(self, buf):
        super().__init__()
        self._buf = buf
        for k in self._KEYS:
            dict.__setitem__(self, k, None)

    def __getitem__(self, key):
        i = self._KEYS.index(key)
        return _RangePair(self, key, [float(v) for v in self._buf[2 * i:2 * i + 2].tolist()])

    def __setitem__(self, key, value):
        i = self._KEYS.index(key)
        self._buf[2 * i:2 * i + 2] = torch.tensor([float(value[0]), float(value[1])], dtype=torch.float64)

    def values(self):
        return [self[k] for k in self._KEYS]

    def items(self):
        return [(k, self[k]) for k in self._KEYS]
