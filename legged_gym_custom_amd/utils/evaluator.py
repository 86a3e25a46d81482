"""PolicyEvaluator — batched policy evaluation on the device, with per-terrain metrics.

What share of the robots survive a full episode on each terrain level x type, how well do they
track the command and at what cost of transport: every env runs ONE episode (its first since
the start; later episodes of an env that fell are ignored, so falls are not over-counted as
they are in extras['episode']), the per-env records are kept by lgx_eval_accumulate after each
env step and folded per terrain cell by lgx_eval_reduce (include/lgx.h, ABI 7). The reference
has no counterpart (its play.py drives one robot and plots a few joint traces).

Policies:
  "student"  what a robot runs (deploy_base.py:244-250 with the exported modules):
             actor([obs | adaptation_encoder(history) | scan_encoder(scan) | estimator(obs)]),
             the mean action, no noise. The actor is fed the ESTIMATOR's output, not the env's
             true estimated observation (which play.py feeds).
  "teacher"  the same with the privileged encoder's latent.

On the GPU, when S8Act covers the networks (Go2), the act is its one-launch kernel writing the
mean straight into env.actions_in (the weights are packed once, at construction and by
refresh_weights()), and the loop body {act, env.step, eval_accumulate} is captured once as a
hipGraph and replayed. Otherwise (CPU, ANYmal) the torch modules run eagerly.

Push recovery (run_push_test): every env is shoved once, at the same episode step, by the step
kernel's scheduled push (lgx_buffers.push_step / push_dvel, ABI 9); the envs are spread over
speed x direction bins through the evaluation's free cell key (lgx_eval_buffers.cell_ids) and a
per-env recovery record (push_rec) is reduced per bin: one run gives the whole polar table.

Command response (run_command_test): every env holds a start command, switches once, at the same
episode step, to the command of its bin of a commanded vx x vy x yaw-rate grid through the step
kernel's command schedule (lgx_buffers.cmd_step / cmd_val, ABI 10), and a per-env step-response
record (cmd_rec) is reduced per bin: one run gives the tracking envelope and the step response.

Sensor model (run_sensor_test): every env gets the observation-noise level, the constant sensor
offset and the sensing latency of its bin of a noise x bias x latency grid through the step
kernel's sensor model (lgx_buffers.obs_noise_scale / obs_bias / obs_delay, ABI 15); the plain
record is reduced per bin: one run gives the whole table.

Height-scan model (run_scan_test): every env gets the scan noise, dropout, map shift and scan
latency of its bin of a four-way grid through the step kernel's height-scan model
(lgx_buffers.scan_noise / scan_dropout / scan_offset / scan_delay, ABI 17); the plain record is
reduced per bin.

Flight recorder (trace_depth= of the three runs, then traces()): a ring buffer on the device for every
env holds the last trace_depth control steps of the env's recorded episode (lgx_trace_record after
each step, include/lgx.h ABI 11: state, commands, joints, torques, actions, foot forces, reward and
the hardest-hit other body, TRACE_COLUMNS) and freezes when the episode ends; afterwards only the
chosen envs' traces (the falls, say) are unrolled on the device and copied to the host. Memory: the
ring takes num_envs x trace_depth x 304 B, 124 MB at 4096 envs and 100 steps.

Gait analysis (gait=True of the three runs): a per-foot contact state machine runs on the device after
each step (lgx_gait_record, include/lgx.h ABI 12) and is reduced per cell or bin of the run's mode:
stance and swing times, stride frequency, duty factor, foot clearance, slip, touchdown force, load
share, which feet move together, and a gait label (gait_cell_report); the per-env records:
gait_records().

Joint load (joints=True of the three runs): a per-joint record runs on the device after each step
(lgx_joint_record, include/lgx.h ABI 13) and is reduced per cell or bin of the run's mode: what the
policy asks of each motor: torque saturation, RMS and peak torque, positive and braking work, peak
speed, use of the joint range, action rate and clipping, and a list of flags (joint_cell_report);
the per-env records: joint_records().

Contacts (contacts=True of the three runs): a per-body record runs on the device after each step
(lgx_contact_record, include/lgx.h ABI 14) and is reduced per cell or bin of the run's mode: where
the robot touches the world: per body the contact share, onsets, force, hits on vertical faces, the
height above the terrain and the share of onsets on a terrain edge; per cell the collision share,
which body ended the falls and which was hit hardest (contact_cell_report); the per-env records:
contact_records().

Single process only: sharded evaluation (env shards over ranks) is out of scope.
"""
import math
import time
from collections import namedtuple

import numpy as np
import torch

from legged_gym_custom_amd import _abi

REPORT_KEYS = ("episodes", "running", "survival_rate", "fall_rate", "blowups", "mean_episode_s", "rms_lin_vel_err",
               "rms_yaw_err", "mean_forward_speed", "cost_of_transport", "mean_peak_foot_force")

# the 76 columns of a flight-recorder row (include/lgx.h lgx_trace_record)
TRACE_COLUMNS = tuple(
    ["episode_length", "pos_x", "pos_y", "pos_z", "quat_x", "quat_y", "quat_z", "quat_w"]
    + [f"{k}_{a}" for k in ("base_lin_vel", "base_ang_vel", "projected_gravity") for a in "xyz"]
    + ["command_vx", "command_vy", "command_yaw", "command_heading"]
    + [f"{k}_{j}" for k in ("dof_pos", "dof_vel", "torque", "action") for j in range(_abi.MAX_DOF)]
    + [f"foot_force_{f}" for f in range(_abi.MAX_FEET)]
    + ["reward", "peak_body_force", "peak_body_index"])
assert len(TRACE_COLUMNS) == _abi.TRACE_COLS


def cell_report(cell, dt, weight):
    """The report entries of one cell row [12] (n_envs, n_timeout, n_fall, n_blowup, sums of the
    8 record columns); weight = m * g of the cost of transport. Ratios without data are None."""
    n, n_to, n_fall, n_blow = (int(round(float(v))) for v in cell[:4])
    s = [float(v) for v in cell[4:]]
    ep = n_to + n_fall + n_blow
    div = lambda a, b: a / b if b > 0 else None  # noqa: E731
    rms = lambda a: math.sqrt(a / s[0]) if s[0] > 0 else None  # noqa: E731
    return {"episodes": ep, "running": n - ep, "survival_rate": div(n_to, ep), "fall_rate": div(n_fall, ep),
            "blowups": n_blow, "mean_episode_s": div(s[0] * dt, ep), "rms_lin_vel_err": rms(s[1]),
            "rms_yaw_err": rms(s[2]), "mean_forward_speed": div(s[3], s[0] * dt),
            "cost_of_transport": div(s[5], weight * s[4]), "mean_peak_foot_force": div(s[7], ep)}


def push_cell_report(pcell, dt):
    """The recovery entries of one push cell row [5] (n, sum of peak tilt, sum of peak tracking
    error, survivors, sum of the survivors' settle steps). Means without data are None."""
    n, surv = int(round(float(pcell[0]))), int(round(float(pcell[3])))
    div = lambda a, b: a / b if b > 0 else None  # noqa: E731
    return {"pushed": n, "mean_peak_tilt_rad": div(float(pcell[1]), n), "mean_peak_lin_vel_err": div(float(pcell[2]), n),
            "survivors": surv, "mean_settle_s": div(float(pcell[4]) * dt, surv)}


def command_cell_report(ccell, dt, command):
    """The step-response entries of one command cell row [9] (n, survivors, the survivors' sums of
    linear and yaw settle steps, sum of peak tilt, the survivors' sums of steady samples and of
    achieved vx, vy, yaw rate) for the bin's command (vx, vy, yaw). Means without data are None."""
    c = [float(v) for v in ccell]
    n, surv = int(round(c[0])), int(round(c[1]))
    div = lambda a, b: a / b if b > 0 else None  # noqa: E731
    achieved = [c[6] / c[5], c[7] / c[5], c[8] / c[5]] if c[5] > 0 else None
    norm2 = command[0] * command[0] + command[1] * command[1]
    gain = (achieved[0] * command[0] + achieved[1] * command[1]) / norm2 if achieved is not None and norm2 > 0 else None
    return {"switched": n, "survivors": surv, "mean_settle_s": div(c[2] * dt, surv),
            "mean_yaw_settle_s": div(c[3] * dt, surv), "mean_peak_tilt_rad": div(c[4], n), "achieved": achieved,
            "gain": gain}


# lgx_gait_record's body pairs (columns 6..11), in order
def force_cell_report(ccell, dt, command, force_n, theta, steady):
    """The force-test entries of one command cell row [9] (command_cell_report's columns; the
    onset is the record's switch step) for the bin's force (force_n newtons at angle theta from
    forward towards left) under the held command (vx, vy, yaw). steady: the force lasts to the end
    of the episode, so the steady window holds forced samples only; otherwise achieved, deflection
    and compliance are None. Means without data are None."""
    r = command_cell_report(ccell, dt, command)
    achieved = r["achieved"] if steady else None
    deflection = [a - c for a, c in zip(achieved, command)] if achieved is not None else None
    compliance = ((deflection[0] * math.cos(theta) + deflection[1] * math.sin(theta)) / force_n
                  if deflection is not None and force_n > 0 else None)
    return {"forced": r["switched"], "survivors": r["survivors"], "mean_peak_tilt_rad": r["mean_peak_tilt_rad"],
            "mean_settle_s": r["mean_settle_s"], "achieved": achieved, "deflection": deflection,
            "compliance_m_per_s_per_n": compliance}


GAIT_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
_FOOT_PLACES = {"FL": (0, 0), "FR": (0, 1), "RL": (1, 0), "RR": (1, 1),   # (front 0 / hind 1, left 0 / right 1)
                "LF": (0, 0), "RF": (0, 1), "LH": (1, 0), "RH": (1, 1)}


def _foot_places(foot_names):
    """(front / hind, left / right) of each foot from its body name (FL/FR/RL/RR or LF/RF/LH/RH as
    a token of the name); None unless they are four feet on four different corners."""
    places = []
    for name in foot_names:
        hit = [_FOOT_PLACES[t] for t in str(name).upper().replace("-", "_").split("_") if t in _FOOT_PLACES]
        if len(hit) != 1:
            return None
        places.append(hit[0])
    return places if len(places) == 4 and len(set(places)) == 4 else None


def gait_label(mean_duty, pair_sync, foot_names):
    """The gait label, a rule and not a measurement: diag, lat and fore are the means of the two
    diagonal, same-side and front/hind pair synchronies (the share of samples in which both feet of
    the pair had the same contact state). "stand" if the mean duty factor exceeds 0.95; else "pronk"
    if all three exceed 0.8; else "trot" / "pace" / "bound" for the largest of diag / lat / fore when
    it leads the other two by at least 0.1; else "mixed". None without data or when the feet cannot
    be placed from their names."""
    places = _foot_places(foot_names)
    if places is None or mean_duty is None or pair_sync is None or any(v is None for v in pair_sync):
        return None
    kinds = {"diag": [], "lat": [], "fore": []}
    for (a, b), v in zip(GAIT_PAIRS, pair_sync):
        (ea, sa), (eb, sb) = places[a], places[b]
        kinds["fore" if ea == eb else ("lat" if sa == sb else "diag")].append(v)
    diag, lat, fore = (sum(kinds[k]) / len(kinds[k]) for k in ("diag", "lat", "fore"))
    if mean_duty > 0.95:
        return "stand"
    if min(diag, lat, fore) > 0.8:
        return "pronk"
    ranked = sorted(((diag, "trot"), (lat, "pace"), (fore, "bound")), reverse=True)
    return ranked[0][1] if ranked[0][0] - ranked[1][0] >= 0.1 else "mixed"


def gait_cell_report(row, dt, foot_names):
    """The gait entries of one gait cell row [61] (lgx_gait_reduce: the number of finished envs with
    samples, sums of the 12 body columns, sums of columns 4..15 of each foot) for the feet
    foot_names (their body names, in feet_idx order). JSON-serialisable; None where there is no
    data, never NaN.

    Per foot ("feet"[name]): duty_factor (stance samples / samples), stride_hz (touchdowns per
    second), mean_stance_s / mean_swing_s (over the stances / swings whose both ends were seen),
    mean_clearance_m (the highest point of a completed swing over its lift-off height),
    slip_m_per_stance_s (horizontal foot travel while in contact, per second of stance), load_share
    (the foot's share of the summed vertical stance force), mean_touchdown_force (the envs' mean of
    their hardest touchdown, N), mean_step_length_m (horizontal foot travel per completed swing:
    the swing path over the completed swings) and stumble_share (samples with a horizontal force
    above 5 x the vertical one). Per body: flight_share (no foot in contact), mean_feet_in_contact,
    pair_sync (GAIT_PAIRS order), mean_duty_factor, mean_stride_hz, mean_slip_m_per_stance_s (means
    over the feet that have data) and gait (gait_label)."""
    c = [float(v) for v in row]
    assert len(c) == _abi.GAIT_CELL_COLS
    div = lambda a, b: a / b if b > 0 else None  # noqa: E731
    def mean(v):  # over the feet that have data
        v = [x for x in v if x is not None]
        return sum(v) / len(v) if v else None
    n, samples, hist, pairs = int(round(c[0])), c[1], c[2:7], c[7:13]
    names = [str(x) for x in foot_names][:_abi.MAX_FEET]
    per = 1 + _abi.GAIT_BODY_COLS
    blocks = [c[per + 12 * f: per + 12 * (f + 1)] for f in range(len(names))]
    load = sum(b[8] for b in blocks)
    feet = {}
    for name, b in zip(names, blocks):
        feet[name] = {"duty_factor": div(b[0], samples), "stride_hz": div(b[1], samples * dt),
                      "mean_stance_s": div(b[3] * dt, b[2]), "mean_swing_s": div(b[5] * dt, b[4]),
                      "mean_clearance_m": div(b[6], b[4]), "slip_m_per_stance_s": div(b[7], b[0] * dt),
                      "load_share": div(b[8], load), "mean_touchdown_force": div(b[9], n),
                      "mean_step_length_m": div(b[10], b[4]), "stumble_share": div(b[11], samples)}
    sync = [div(pairs[i], samples) if max(GAIT_PAIRS[i]) < len(names) else None for i in range(6)]
    duty = mean([f["duty_factor"] for f in feet.values()])
    return {"envs": n, "samples": int(round(samples)), "gait": gait_label(duty, sync, names),
            "flight_share": div(hist[0], samples),
            "mean_feet_in_contact": div(sum(m * h for m, h in enumerate(hist)), samples), "pair_sync": sync,
            "mean_duty_factor": duty, "mean_stride_hz": mean([f["stride_hz"] for f in feet.values()]),
            "mean_slip_m_per_stance_s": mean([f["slip_m_per_stance_s"] for f in feet.values()]), "feet": feet}


# joint_cell_report's flags: the shares of a joint's samples above which it is named
JOINT_FLAG_SATURATION = 0.05  # torque at or above the limit
JOINT_FLAG_RANGE = 0.01       # angle outside the soft position limits
JOINT_FLAG_CLIP = 0.01        # action at or above clip_actions
_JOINT_PER = _abi.JOINT_COLS + 4  # columns of a joint in a cell row: 15 sums, 5 extremes
_JOINT_BASE = 2 + _abi.JOINT_BODY_COLS
assert _JOINT_BASE + _abi.MAX_DOF * _JOINT_PER == _abi.JOINT_CELL_COLS


def _joint_extremes():
    """The cell columns that are maxima and those that are minima (lgx_joint_reduce)."""
    hi, lo = [1 + _abi.JOINT_BODY_COLS], []
    for j in range(_abi.MAX_DOF):
        b = _JOINT_BASE + _JOINT_PER * j
        hi += [b + 15, b + 16, b + 17, b + 19]
        lo.append(b + 18)
    return hi, lo


def joint_total_row(cells):
    """The joint cell row [246] of all cells [..., 246] together: the sums added, the maxima / minima
    taken over the cells that have an env (an empty cell's zeros are no angle or torque anyone
    used); all zero when every cell is empty."""
    flat = torch.as_tensor(cells, dtype=torch.float64).reshape(-1, _abi.JOINT_CELL_COLS)
    total = flat.sum(0)
    full = flat[flat[:, 0] > 0]
    hi, lo = _joint_extremes()
    total[hi] = full[:, hi].max(0).values if len(full) else 0.0
    total[lo] = full[:, lo].min(0).values if len(full) else 0.0
    return total


def joint_cell_report(row, dt, joint_names, params):
    """The joint-load entries of one joint cell row [246] (lgx_joint_reduce) for the joints
    joint_names (env.dof_names); params: the limits, an object with torque_limits [j], dof_vel_limits
    [j], dof_pos_limits [j][2] and clip_actions (the env's lgx_task_params). JSON-serialisable; None
    where there is no data, never NaN.

    Per joint ("joints"[name]): torque_saturation_share (samples with |torque| at the limit),
    rms_torque and rms_torque_over_limit (heat), mean_peak_torque (the envs' mean of their peak),
    max_peak_torque and max_peak_torque_over_limit, mean_positive_power_w / mean_negative_power_w
    (positive / braking work per second of recorded time), work_share (the joint's share of the
    positive work), max_peak_power_w, max_peak_speed, max_peak_speed_over_limit, over_speed_share,
    out_of_range_share (outside the soft position limits), range_used [min q, max q],
    range_margin_rad (min(min q - lo, hi - max q): negative when the range was left),
    action_rate_rms (over the samples that have a predecessor: samples - envs), action_clip_share,
    braking_share (samples with negative power) and mean_speed. Per body: envs, samples,
    mean_peak_power_w (the envs' mean of their peak total power), max_peak_power_w,
    any_saturation_share / any_out_of_range_share (samples in which any joint was) and flags.

    flags is a rule and not a measurement: one string per joint and crossing, for a torque
    saturation share above JOINT_FLAG_SATURATION, any sample above the speed limit, an out-of-range
    share above JOINT_FLAG_RANGE and an action clip share above JOINT_FLAG_CLIP."""
    c = [float(v) for v in row]
    assert len(c) == _abi.JOINT_CELL_COLS
    div = lambda a, b: a / b if b > 0 else None  # noqa: E731
    root = lambda v: None if v is None else math.sqrt(v)  # noqa: E731
    n, samples = int(round(c[0])), c[1]
    have = lambda v: v if n > 0 else None  # noqa: E731  (an extreme of no env is no value)
    names = [str(x) for x in joint_names][:_abi.MAX_DOF]
    blocks = [c[_JOINT_BASE + _JOINT_PER * j: _JOINT_BASE + _JOINT_PER * (j + 1)] for j in range(len(names))]
    work = sum(b[3] for b in blocks)
    joints, flags = {}, []
    for j, (name, b) in enumerate(zip(names, blocks)):
        L, V = float(params.torque_limits[j]), float(params.dof_vel_limits[j])
        lo, hi = float(params.dof_pos_limits[j][0]), float(params.dof_pos_limits[j][1])
        rms = root(div(b[1], samples))
        e = {"torque_saturation_share": div(b[0], samples), "rms_torque": rms,
             "rms_torque_over_limit": None if rms is None else div(rms, L), "mean_peak_torque": div(b[2], n),
             "max_peak_torque": have(b[15]), "max_peak_torque_over_limit": have(div(b[15], L)),
             "mean_positive_power_w": div(b[3], samples * dt), "mean_negative_power_w": div(b[4], samples * dt),
             "work_share": have(div(b[3], work)), "max_peak_power_w": have(b[16]), "max_peak_speed": have(b[17]),
             "max_peak_speed_over_limit": have(div(b[17], V)), "over_speed_share": div(b[7], samples),
             "out_of_range_share": div(b[8], samples), "range_used": have([b[18], b[19]]),
             "range_margin_rad": have(min(b[18] - lo, hi - b[19])), "action_rate_rms": root(div(b[11], samples - n)),
             "action_clip_share": div(b[12], samples), "braking_share": div(b[13], samples),
             "mean_speed": div(b[14], samples)}
        joints[name] = e
        if n > 0:
            if e["torque_saturation_share"] > JOINT_FLAG_SATURATION:
                flags.append(f"{name}: torque at its limit in {e['torque_saturation_share']:.1%} of the samples")
            if b[7] > 0:
                flags.append(f"{name}: above the speed limit in {int(round(b[7]))} samples "
                             f"({e['over_speed_share']:.2%})")
            if e["out_of_range_share"] > JOINT_FLAG_RANGE:
                flags.append(f"{name}: outside the soft position limits in {e['out_of_range_share']:.1%} of the samples")
            if e["action_clip_share"] > JOINT_FLAG_CLIP:
                flags.append(f"{name}: action at its clip in {e['action_clip_share']:.1%} of the samples")
    return {"envs": n, "samples": int(round(samples)), "mean_peak_power_w": div(c[2], n), "max_peak_power_w": have(c[5]),
            "any_saturation_share": div(c[3], samples), "any_out_of_range_share": div(c[4], samples),
            "flags": flags if n > 0 else None, "joints": joints}


# The terrain relief (m) under a body above which a contact onset counts as "on an edge" (the
# record's edge_tol): a rule, not a measurement.
EDGE_RELIEF_M = 0.05
_CONTACT_PER = 13   # columns of a body in a contact cell row: 8 sums, 3 extremes, 2 fall histograms
_CONTACT_BASE = 8
assert _CONTACT_BASE + _abi.MAX_BODIES * _CONTACT_PER == _abi.CONTACT_CELL_COLS


def contact_total_row(cells):
    """The contact cell row [320] of all cells [..., 320] together: the sums added, the maxima taken
    over the cells that have an env and the minima (column 7's) over the cells that have samples;
    all zero when every cell is empty."""
    flat = torch.as_tensor(cells, dtype=torch.float64).reshape(-1, _abi.CONTACT_CELL_COLS)
    total = flat.sum(0)
    full, sampled = flat[flat[:, 0] > 0], flat[flat[:, 1] > 0]
    hi = [4] + [_CONTACT_BASE + _CONTACT_PER * b + k for b in range(_abi.MAX_BODIES) for k in (8, 9)]
    lo = [_CONTACT_BASE + _CONTACT_PER * b + 10 for b in range(_abi.MAX_BODIES)]
    total[hi] = full[:, hi].max(0).values if len(full) else 0.0
    total[lo] = sampled[:, lo].min(0).values if len(sampled) else 0.0
    return total


def contact_cell_report(row, dt, body_names, feet, termination, penalised):
    """The contact entries of one contact cell row [320] (lgx_contact_reduce) for the bodies
    body_names (env.body_names); feet, termination, penalised: the body indices of feet_idx,
    termination_idx and penalised_idx. JSON-serialisable; None where there is no data, never NaN.

    Per body ("bodies"[name]): contact_share (samples with a contact force over 0.1 N, the collision
    reward's rule), onsets_per_s, mean_force_in_contact (impulse / contact time), peak_force,
    face_hit_share (the share of its contact samples with a force more horizontal than 5 : 1, the
    feet_stumble rule), hard_share (samples over the 1 N termination threshold),
    mean_height_above_terrain_m, min_height_above_terrain_m, edge_onset_share (the share of its
    onsets over a terrain relief above the record's edge_tol), mean_onset_relief_m,
    max_onset_relief_m and roles (of "foot", "termination", "penalised").
    Per cell: envs, samples, collision_share (samples with any non-foot body in contact),
    mean_penalised_in_contact (the collision reward's raw value per sample), peak_nonfoot_force,
    falls, mean_termination_bodies_at_fall, fall_causes ({name: share of the falls which that
    termination body ended, "no_contact": the share ended by orientation or by falling out}; the
    shares sum to 1), hardest_hit_at_fall (the same over the non-foot bodies: which one carried the
    largest force at the step that ended the episode) and foot_edge_onset_share (the feet's onsets
    together: the share of touchdowns on an edge)."""
    c = [float(v) for v in row]
    assert len(c) == _abi.CONTACT_CELL_COLS
    div = lambda a, b: a / b if b > 0 else None  # noqa: E731
    n, samples, falls = int(round(c[0])), c[1], c[5]
    names = [str(x) for x in body_names][:_abi.MAX_BODIES]
    feet, termination, penalised = ([int(i) for i in lst] for lst in (feet, termination, penalised))
    blocks = [c[_CONTACT_BASE + _CONTACT_PER * b: _CONTACT_BASE + _CONTACT_PER * (b + 1)] for b in range(len(names))]
    bodies = {}
    for i, (name, b) in enumerate(zip(names, blocks)):
        roles = [r for r, lst in (("foot", feet), ("termination", termination), ("penalised", penalised)) if i in lst]
        bodies[name] = {
            "contact_share": div(b[0], samples), "onsets_per_s": div(b[1], samples * dt),
            "mean_force_in_contact": div(b[2], b[0] * dt), "peak_force": b[8] if n > 0 else None,
            "face_hit_share": div(b[3], b[0]), "hard_share": div(b[7], samples),
            "mean_height_above_terrain_m": div(b[4], samples),
            "min_height_above_terrain_m": b[10] if samples > 0 else None,
            "edge_onset_share": div(b[5], b[1]), "mean_onset_relief_m": div(b[6], b[1]),
            "max_onset_relief_m": b[9] if b[1] > 0 else None, "roles": roles}
    causes = hardest = None
    if falls > 0:
        causes = {names[i]: blocks[i][11] / falls for i in sorted(set(termination)) if i < len(names)}
        causes["no_contact"] = c[6] / falls
        nonfoot = [i for i in range(len(names)) if i not in feet]
        hardest = {names[i]: blocks[i][12] / falls for i in nonfoot}
        hardest["no_contact"] = (falls - sum(blocks[i][12] for i in nonfoot)) / falls
    foot = [blocks[i] for i in feet if i < len(names)]
    return {"envs": n, "samples": int(round(samples)), "collision_share": div(c[3], samples),
            "mean_penalised_in_contact": div(c[2], samples), "peak_nonfoot_force": c[4] if n > 0 else None,
            "falls": int(round(falls)), "mean_termination_bodies_at_fall": div(c[7], falls),
            "fall_causes": causes, "hardest_hit_at_fall": hardest,
            "foot_edge_onset_share": div(sum(b[5] for b in foot), sum(b[1] for b in foot)), "bodies": bodies}


# The record families a run can keep, in the order the loop body records them. kind: the env's
# <kind>_buffers / record_begin / record_step / record_cells; flag: the keyword of run, run_push_test
# and run_command_test; key: the report entry; last: the evaluator attribute that holds the finished
# run's cells ([rows, cols, 61 / 246 / 320] float64, None without the record); total: all cells'
# rows [n, cols] -> the total's row; report(row, *args(env)): the entry of one cell row;
# buffers: extra keywords of <kind>_buffers.
Record = namedtuple("Record", "kind flag key last total report args buffers")
RECORDS = (
    Record("gait", "gait", "gait", "last_gait_cells", lambda flat: flat.sum(0), gait_cell_report,
           lambda env: (float(env.dt), [env.body_names[i] for i in env.feet_indices.tolist()]), {}),
    Record("joint", "joints", "joints", "last_joint_cells", joint_total_row, joint_cell_report,
           lambda env: (float(env.dt), env.dof_names, env._native.params), {}),
    Record("contact", "contacts", "contacts", "last_contact_cells", contact_total_row, contact_cell_report,
           lambda env: (float(env.dt), env.body_names, env.feet_indices.tolist(),
                        env.termination_contact_indices.tolist(), env.penalised_contact_indices.tolist()),
           {"edge_tol": EDGE_RELIEF_M}),
)


def _min_max(t, kind):
    return None if t is None else [kind(t.min()), kind(t.max())]


class PolicyEvaluator:
    def __init__(self, env, runner, policy="student"):
        if policy not in ("student", "teacher"):
            raise ValueError(f"policy must be 'student' or 'teacher' (got {policy!r})")
        if getattr(env, "num_envs_total", env.num_envs) != env.num_envs:
            raise RuntimeError("PolicyEvaluator is single-process: the env is sharded over ranks")
        self.env, self.runner, self.alg = env, runner, runner.alg
        self.policy = policy
        self.adaptation_mode = policy == "student"
        self.device = str(runner.device)
        if torch.device(self.device) != torch.device(env.device):
            raise RuntimeError(f"the evaluator runs the policy on the env's device ({env.device}), not {self.device}")
        self.on_gpu = self.device.startswith("cuda")
        self._graph = self._graph_key = None            # run's captured loop (key: the trace depth, gait, joints)
        self._push_graph = self._push_graph_key = None  # run_push_test's own captured loop
        self._cmd_graph = self._cmd_graph_key = None    # run_command_test's own captured loop
        self._sensor_graph = self._sensor_graph_key = None  # run_sensor_test's own captured loop
        self._scan_graph = self._scan_graph_key = None      # run_scan_test's own captured loop
        self.last_scan_bins = None
        self._force_graph = self._force_graph_key = None  # run_force_test's own captured loop
        self.last_force_cells = self.last_force_bins = None
        self.last_sensor_bins = None
        self._fused = None
        self.last_cells = None
        self.last_push_cells = self.last_push_bins = None
        self.last_cmd_cells = self.last_cmd_bins = None
        self._trace_depth = None     # the flight recorder's depth in the run under way (None: off)
        self.last_trace_depth = None  # the depth of the last finished run, None when it was not traced
        self._records = ()           # the RECORDS the run under way keeps
        for r in RECORDS:
            setattr(self, r.last, None)  # last_gait_cells, last_joint_cells, last_contact_cells
        if self.on_gpu:
            from legged_gym_custom_amd.rsl_rl.algorithms.s8_act import S8Act
            if S8Act.supported(self.alg):
                f = S8Act(self.alg, env.num_envs)
                dst = env.actions_in
                if dst.shape == f.mu.shape and dst.is_contiguous() and dst.dtype == torch.float32:
                    # the kernel writes the mean into the env's action input: env.step copies nothing
                    f.mu = dst
                    f.args.mu, f.args.ld_mu = dst.data_ptr(), dst.stride(0)
                self._fused = f
                self.refresh_weights()
        # m * g of the cost of transport: the model's nominal total mass (the per-env added base
        # mass of the mass randomisation is ignored)
        self.mass = float(sum(l["mass"] for l in env.model_dict["links"]))
        self.gravity = abs(float(env.sim_params.gravity[2]))

    def refresh_weights(self):
        """Re-pack the fused act kernel's weights (after the runner loaded or trained them)."""
        if self._fused is not None:
            self._fused.refresh_weights()
            self._graph = self._push_graph = self._cmd_graph = self._sensor_graph = self._force_graph = self._scan_graph = None

    # ------------------------------------------------------------------ one iteration
    def act(self):
        """The policy's mean action on the env's current observations."""
        env, ac = self.env, self.alg.actor_critic
        obs, priv, scan = env.obs_buf, env.privileged_obs_buf, env.scan_obs_buf
        if self._fused is not None:
            mu, _ = self._fused.run(obs, priv, env.critic_obs_buf, scan, rows=None, head=None,
                                    adaptation_mode=self.adaptation_mode)
            return mu
        return ac.act_inference(obs, priv, self.alg.estimator(obs), scan, adaptation_mode=self.adaptation_mode)

    def step(self, ev=None):
        """One eager iteration: act, env.step, eval_accumulate (ev: the eval buffers to record
        into; default: the plain evaluation's), gait_record in a gait run, joint_record in a joints
        run, contact_record in a contacts run and trace_record in a traced run."""
        with torch.no_grad():
            self._body(ev)

    def _body(self, ev):
        """The loop body, written once for the eager loop (step) and the capture (_capture)."""
        env = self.env
        env.step(self.act())
        env.eval_accumulate(ev)
        for r in self._records:
            env.record_step(r.kind)
        if self._trace_depth is not None:
            env.trace_record()

    def begin(self, ev=None):
        """Reset every env and start recording. The env's step and reset-call counters (the keys
        of its random streams) are rewound, so an evaluation depends only on the weights, the
        seed and the config, and repeats exactly; do not interleave it with training on the same
        env. reset() ends with the reference's zero-action step (base_task.py:131-135), which
        yields the first observations; the episode lengths are then set to 0 (no random initial
        lengths)."""
        env = self.env
        env.common_step_counter = 0
        env._reset_calls = 0
        with torch.no_grad():
            env.reset()
            env.episode_length_buf = torch.zeros_like(env.episode_length_buf)
            env.eval_begin(ev)
            for r in self._records:
                env.record_begin(r.kind)
            if self._trace_depth is not None:
                env.trace_begin()

    def _set_trace(self, trace_depth, gait=False, joints=False, contacts=False):
        """Start a run: the flight recorder's depth for it (None: off; else the env's rings of that
        depth, allocated once per depth) and whether it keeps the gait record, the joint-load record
        and the contact record (the mode picks the env's gait / joint / contact buffers: their cell
        key is the mode's)."""
        flags = {"gait": gait, "joints": joints, "contacts": contacts}
        self.last_trace_depth = None
        for r in RECORDS:
            setattr(self, r.last, None)
        self._records = tuple(r for r in RECORDS if flags[r.flag])
        self._trace_depth = None if trace_depth is None else int(trace_depth)
        if self._trace_depth is not None:
            self.env.trace_buffers(self._trace_depth)

    def _record_buffers(self, *grid):
        """Make the env's buffers of the run's records current: grid = (rows, cols, cell_ids) for a
        mode whose bin is the cell key, nothing for the terrain grid."""
        for r in self._records:
            getattr(self.env, r.kind + "_buffers")(*grid, **r.buffers)

    def _capture(self, ev=None):
        """The loop body as one hipGraph (the runner's _capture_rollout is the model): one eager
        iteration warms every kernel, then the capture records without executing. Returns the
        graph (it records into ev; default: the plain evaluation's buffers)."""
        env = self.env
        self.step(ev)
        torch.cuda.synchronize(self.device)
        csc = env.common_step_counter
        g = torch.cuda.CUDAGraph()
        with torch.inference_mode(False), torch.no_grad(), \
                torch.cuda.graph(g, capture_error_mode=self.alg.capture_mode()):
            self._body(ev)
        env.common_step_counter = csc  # host mirror (capture advanced it, the device did not)
        return g

    # ------------------------------------------------------------------ run
    def run(self, num_steps=None, graph=True, action_delay_s=None, motor_strength=None, trace_depth=None,
            gait=False, joints=False, contacts=False):
        """Evaluate: reset, num_steps x {act, step, accumulate}, reduce, one host read; returns the
        report (JSON-serialisable): per-cell and total entries REPORT_KEYS, None where a cell has
        no data (never NaN).

        action_delay_s / motor_strength: a constant actuation latency (seconds) / motor strength
        factor for all envs for this run only, set through env.set_action_delay / set_motor_strength
        (in place: the captured loop keeps replaying); the env's own per-env values are put back, in
        place, when the run ends. None leaves the env's values. The env must have been built with
        the capacity (domain_rand.max_action_delay_s). The report's action_delay_substeps /
        motor_strength are the [min, max] over the envs during the run, None when the env has no
        such buffer.

        num_steps defaults to max_episode_length + 1: the step kernel's rule is time_out =
        episode_length > max_episode_length (lgx_env.hip env_step_kernel, go2.py:186-204), the
        length counting from 0, so by then every env has finished once and `running` is 0.
        graph: replay the captured loop body where the env allows it (GPU, env.graph_capturable);
        False forces the eager loop. Both give bit-identical cells.
        trace_depth: record the last trace_depth steps of every env's episode in the flight recorder
        (the loop body gains lgx_trace_record, in a captured loop of its own per depth; the cells are
        bit-identical to an untraced run's); read them with traces(). None: no recorder, the loop
        and its graph are the untraced ones.
        gait: keep the gait record (the loop body gains lgx_gait_record, in a captured loop of its
        own; the cells are bit-identical to a run's without it): the report gains a "gait" entry
        (gait_cell_report) in every cell and in total; the per-env records: gait_records(). False:
        nothing changes.
        joints: keep the joint-load record (the loop body gains lgx_joint_record, in a captured loop
        of its own; the cells are bit-identical to a run's without it): the report gains a "joints"
        entry (joint_cell_report) in every cell and in total; the per-env records: joint_records().
        False: nothing changes.
        contacts: keep the contact record (the loop body gains lgx_contact_record, in a captured loop
        of its own; the cells are bit-identical to a run's without it): the report gains a "contacts"
        entry (contact_cell_report) in every cell and in total; the per-env records:
        contact_records(). False: nothing changes."""
        env = self.env
        self._set_trace(trace_depth, gait, joints, contacts)
        self._record_buffers()  # the terrain grid is the cell key
        saved = []  # (buffer, its values before this run)
        try:
            if action_delay_s is not None:
                if env.action_delay_substeps is not None:
                    saved.append((env.action_delay_substeps, env.action_delay_substeps.clone()))
                env.set_action_delay(action_delay_s)
            if motor_strength is not None:
                had = env.motor_strengths is not None
                if had:
                    saved.append((env.motor_strengths, env.motor_strengths.clone()))
                env.set_motor_strength(motor_strength)  # (the first one allocates: refused once a loop is captured)
                if not had:
                    saved.append((env.motor_strengths, torch.ones_like(env.motor_strengths)))
            cells, head, rates = self._drive("_graph", (), num_steps, graph, env.eval_cells)
            out = self.report(cells, head["num_steps"], rates["wall_s"], head["graph"])
            self._attach_records(out["total"], [cell for row in out["cells"] for cell in row])
            return out
        finally:
            for buf, old in saved:
                buf.copy_(old)

    def _drive(self, slot, key, num_steps, graph, read_cells, prepare=None, started=None, cleanup=None):
        """The run of all five modes. slot / key: the mode's graph attribute ("_graph", "_push_graph",
        "_cmd_graph", "_sensor_graph", "_force_graph", "_scan_graph"; its key lives in slot + "_key") and the mode's part of the graph key, to which
        the trace depth and the gait, joints and contacts flags are added: the loop is captured when
        there is no graph or the key changed. prepare(): the mode's setup before the capture and begin, returns the eval
        buffers to record into (None: the plain evaluation's); started(): after begin; cleanup():
        always, when the run ends or fails. read_cells(): the mode's reduce and host read
        (synchronises), one tensor or a tuple with the [rows, cols, 12] cells first.
        Returns (what read_cells returned, the report's common head, its wall_s / env_steps_per_s
        tail) and sets last_cells, last_trace_depth and the RECORDS' last_*_cells (the cells of the
        records the run kept)."""
        env = self.env
        steps = int(env.max_episode_length) + 1 if num_steps is None else int(num_steps)
        use_graph = bool(graph) and self.on_gpu and getattr(env, "graph_capturable", False)
        gkey = key + (self._trace_depth,) + tuple(r in self._records for r in RECORDS)
        try:
            ev = prepare() if prepare else None
            if use_graph and (getattr(self, slot) is None or getattr(self, slot + "_key") != gkey):
                setattr(self, slot, self._capture(ev))
                setattr(self, slot + "_key", gkey)
            self.begin(ev)
            if started:
                started()
            t0 = self._loop(steps, getattr(self, slot) if use_graph else None, ev)
            cells = read_cells()
            rcells = [env.record_cells(r.kind) for r in self._records]
            wall = time.perf_counter() - t0
        finally:
            if cleanup:
                cleanup()
        self.last_cells = cells[0] if isinstance(cells, tuple) else cells  # as lgx_eval_reduce wrote them
        self.last_trace_depth = self._trace_depth
        for r, c in zip(self._records, rcells):
            setattr(self, r.last, c)
        return cells, self._head(steps, use_graph), self._rates(steps, wall)

    def _head(self, steps, graph):
        return {"policy": self.policy, "num_envs": int(self.env.num_envs), "num_steps": steps, "dt": float(self.env.dt),
                "nominal_mass": self.mass, "graph": graph}

    def _rates(self, steps, wall):
        return {"wall_s": wall, "env_steps_per_s": steps * self.env.num_envs / wall if wall > 0 else None}

    def _attach_records(self, total, bins):
        """The report entry (Record.key, by Record.report) of every record the finished run kept, in
        the total and in every bin, from its last_*_cells; bins: the report's cells or bins flat, in
        the order of the record's cells. Nothing without a record."""
        for r in RECORDS:
            rcells = getattr(self, r.last)
            if rcells is None:
                continue
            args = r.args(self.env)
            flat = rcells.reshape(-1, rcells.shape[2])
            total[r.key] = r.report(r.total(flat), *args)
            for row, b in zip(flat, bins):
                b[r.key] = r.report(row, *args)

    def _switch_step(self, at_s, test):
        """at_s (seconds into the episode) as an episode step of the push / command test."""
        at, last = float(at_s), int(self.env.max_episode_length)
        step = int(round(at / float(self.env.dt))) if math.isfinite(at) else -1
        if not 0 < step < last:
            raise ValueError(f"{test}: at_s = {at_s} s is step {step}, outside 0 < step < max_episode_length = {last}")
        return step

    def _cmd_eval(self, key, other):
        """env.cmd_eval_buffers(*key), which the command test and the force test share: the env
        allocates them anew when the key changes, so the captured loop of the other mode (slot
        `other`), which records into the old ones, is dropped then."""
        if getattr(self.env, "_cmd_eval_key", None) != key:
            setattr(self, other, None)
        return self.env.cmd_eval_buffers(*key)

    def _bins(self, count):
        """Each env's bin of `count`: randperm(num_envs, seeded with env.seed) % count."""
        return torch.randperm(self.env.num_envs, generator=torch.Generator().manual_seed(int(self.env.seed))) % count

    def _records_of(self, r):
        """The per-env records of RECORDS entry r of the last run, numpy arrays on the host under
        their lgx_<kind>_buffers member names, and the status."""
        if getattr(self, r.last) is None:
            raise RuntimeError(f"{r.kind}_records(): the last run kept no {r.kind} record (pass {r.flag}=True to run, "
                               "run_push_test or run_command_test first)")
        names = [name for name, _ in _abi.RECORD_KINDS[r.kind][1]] + ["status"]
        return {name: getattr(self.env, attr).cpu().numpy() for name, attr in zip(names, self.env._RECORD_ATTRS[r.kind])}

    def gait_records(self):
        """The per-env gait records of the last run (it must have been one with gait=True), numpy
        arrays on the host: foot [N, 4, 16], body [N, 12] and status [N] (lgx_gait_buffers)."""
        return self._records_of(RECORDS[0])

    def joint_records(self):
        """The per-env joint-load records of the last run (it must have been one with joints=True),
        numpy arrays on the host: joint [N, 12, 16], body [N, 4] and status [N] (lgx_joint_buffers)."""
        return self._records_of(RECORDS[1])

    def contact_records(self):
        """The per-env contact records of the last run (it must have been one with contacts=True),
        numpy arrays on the host: body [N, 24, 12], env [N, 8] and status [N] (lgx_contact_buffers)."""
        return self._records_of(RECORDS[2])

    def _loop(self, steps, g, ev):
        """steps x the loop body (g: its captured graph, or None for the eager loop) recording
        into ev; returns the start time."""
        env = self.env
        if self.on_gpu:
            torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        if g is not None:
            for _ in range(steps):
                g.replay()
                env.advance_step_counter(1)
        else:
            for _ in range(steps):
                self.step(ev)
        return t0

    # ------------------------------------------------------------------ push recovery
    def run_push_test(self, speeds, directions=8, at_s=2.0, settle_tol=0.3, num_steps=None, graph=True,
                      trace_depth=None, gait=False, joints=False, contacts=False):
        """How hard a shove does the policy survive, from which side, and how quickly does it
        settle: one run in which every env is pushed once, at episode step round(at_s / dt), by a
        velocity impulse of its bin (speed index s, direction index d): dvel = speeds[s] *
        (cos t, sin t, 0) with t = 2 pi d / directions measured from the robot's forward axis
        towards its left. Envs get bins by randperm(num_envs, seeded with env.seed) % (S * D): bin
        sizes differ by at most one and do not follow the terrain columns. Speed 0 gives the
        control row.

        The records go to a second set of eval buffers (env.push_eval_buffers: the bin is the cell
        key, plus the per-env recovery record of include/lgx.h), and this mode's captured loop is a
        graph of its own, never the plain run's. The env needs the push buffers before any of its
        steps is captured (domain_rand.scheduled_pushes = True, or call this before run()).
        The schedule is cleared in place when the run ends, so a following run() is the plain one.

        trace_depth: the flight recorder, as in run(). gait: the gait record, as in run(), per bin.
        joints: the joint-load record, as in run(), per bin. contacts: the contact record, as in run(),
        per bin.

        Returns the report: "bins"[s][d] with the REPORT_KEYS entries and pushed (finished envs
        with post-push samples), mean_peak_tilt_rad, mean_peak_lin_vel_err (m/s), survivors (timed
        out among them) and mean_settle_s (the survivors' mean time from the push to the last step
        whose tracking error exceeded settle_tol); "total" likewise; speeds, directions_deg,
        push_step, settle_tol. None where there is no data, never NaN.
        ValueError: no speeds or directions, a negative or non-finite speed, a push step outside
        0 < step < max_episode_length."""
        env = self.env
        self._set_trace(trace_depth, gait, joints, contacts)
        speeds = [float(v) for v in speeds]
        S, D = len(speeds), int(directions)
        if S < 1 or D < 1 or not all(math.isfinite(v) and v >= 0.0 for v in speeds):
            raise ValueError(f"push test: need at least one finite speed >= 0 and one direction (got {speeds}, {directions})")
        if not (math.isfinite(float(settle_tol)) and float(settle_tol) >= 0.0):
            raise ValueError(f"push test: settle_tol must be finite and >= 0 (got {settle_tol})")
        step = self._switch_step(at_s, "push test")
        bins = self._bins(S * D)
        theta = 2.0 * math.pi * (bins % D).double() / D
        v = torch.tensor(speeds, dtype=torch.float64)[bins // D]
        dvel = torch.stack([v * torch.cos(theta), v * torch.sin(theta), torch.zeros_like(v)], 1).float()
        key = (S, D, float(settle_tol))

        def prepare():
            env.set_push_schedule(0, dvel)  # (the first one allocates: refused once a loop is captured)
            ev = env.push_eval_buffers(*key)
            env.push_cell_ids.copy_(bins.to(torch.int32))
            self._record_buffers(S, D, env.push_cell_ids)  # the bin is the cell key
            return ev

        (cells, pcells), head, rates = self._drive(
            "_push_graph", key, num_steps, graph, env.eval_push_cells, prepare,
            lambda: env.set_push_schedule(step, dvel),  # after begin: its reset ends with an env step of its own
            env.clear_push_schedule)
        self.last_push_cells, self.last_push_bins = pcells, bins
        dt, w = head["dt"], self.mass * self.gravity
        both = lambda c, p: {**cell_report(c, dt, w), **push_cell_report(p, dt)}  # noqa: E731
        out = {**head, "speeds": speeds, "directions_deg": [360.0 * d / D for d in range(D)],
               "push_step": step, "push_at_s": step * dt, "settle_tol": float(settle_tol),
               "total": both(cells.reshape(-1, cells.shape[2]).sum(0), pcells.reshape(-1, pcells.shape[2]).sum(0)),
               "bins": [[both(cells[s, d], pcells[s, d]) for d in range(D)] for s in range(S)], **rates}
        self._attach_records(out["total"], [b for row in out["bins"] for b in row])
        return out

    # ------------------------------------------------------------------ command response
    def run_command_test(self, vx, vy=(0.0,), yaw=(0.0,), at_s=2.0, start=(0.0, 0.0, 0.0), steady_after_s=1.0,
                         settle_tol=0.3, yaw_tol=0.3, num_steps=None, graph=True, trace_depth=None, gait=False,
                         joints=False, contacts=False):
        """What does the robot do when commanded, how fast does it get there, and does it stay up:
        one run in which every env holds the command `start` = (vx, vy, yaw rate), switches at
        episode step round(at_s / dt) to the command of its bin (vx[ix], vy[iy], yaw[iw]) and is
        recorded from the switch on. Bin index (ix * |vy| + iy) * |yaw| + iw; envs get bins by
        randperm(num_envs, seeded with env.seed) % bins. The commands are literal (no small-command
        zeroing, no heading controller: yaw is a yaw rate) and come back after a reset: a reset env
        holds `start` again and switches again, but only an env's first episode is recorded.

        The records go to eval buffers of their own (env.cmd_eval_buffers: the bin is the cell key,
        plus the per-env step-response record of include/lgx.h), and this mode's captured loop is a
        graph of its own. The env needs the schedule buffers before any of its steps is captured
        (commands.scheduled_commands = True, or call this before run()). The schedule is written
        before the run's reset and cleared in place when the run ends, so a following run() is the
        plain one.

        trace_depth: the flight recorder, as in run(). gait: the gait record, as in run(), per bin
        (how the gait changes with the commanded speed). joints: the joint-load record, as in run(),
        per bin (what each commanded speed asks of the motors). contacts: the contact record, as in
        run(), per bin.

        Returns the report: "bins"[ix][iy][iw] with the REPORT_KEYS entries and switched (finished
        envs with post-switch samples), survivors (timed out among them), mean_settle_s /
        mean_yaw_settle_s (the survivors' mean time from the switch until the linear velocity / yaw
        rate error stays within settle_tol / yaw_tol; 0: never off), mean_peak_tilt_rad, achieved
        [vx, vy, yaw] (the survivors' mean velocities over the samples from steady_after_s after the
        switch on) and gain (achieved velocity projected on the commanded (vx, vy) direction over its
        norm; None for a zero linear command); "total" likewise without achieved / gain; vx, vy,
        yaw, start, switch_step, steady_after, the tolerances. None where there is no data, never NaN.
        ValueError: an empty list, a non-finite entry, a switch step outside 0 < step <
        max_episode_length, a negative or non-finite tolerance or steady_after_s."""
        env = self.env
        self._set_trace(trace_depth, gait, joints, contacts)
        vx, vy, yaw, start = ([float(v) for v in lst] for lst in (vx, vy, yaw, start))
        if min(len(vx), len(vy), len(yaw)) < 1 or len(start) != 3 or \
                not all(math.isfinite(v) for v in vx + vy + yaw + start):
            raise ValueError(f"command test: vx, vy and yaw need at least one finite entry each and start three "
                             f"(got {vx}, {vy}, {yaw}, {start})")
        for name, tol in (("settle_tol", settle_tol), ("yaw_tol", yaw_tol), ("steady_after_s", steady_after_s)):
            if not (math.isfinite(float(tol)) and float(tol) >= 0.0):
                raise ValueError(f"command test: {name} must be finite and >= 0 (got {tol})")
        dt, step = float(env.dt), self._switch_step(at_s, "command test")
        steady = int(round(float(steady_after_s) / dt))
        n, nx, ny, nw = env.num_envs, len(vx), len(vy), len(yaw)
        bins = self._bins(nx * ny * nw)
        grid = torch.tensor([[a, b, c, 0.0] for a in vx for b in vy for c in yaw], dtype=torch.float32)
        values = torch.stack([torch.tensor(start + [0.0], dtype=torch.float32).expand(n, 4), grid[bins]], 1)
        key = (nx, ny * nw, float(settle_tol), float(yaw_tol), steady)

        def prepare():
            # before begin: its reset sees segment 0 (the first call allocates: refused once a loop is captured)
            env.set_command_schedule([0, step], values)
            ev = self._cmd_eval(key, "_force_graph")
            env.cmd_cell_ids.copy_(bins.to(torch.int32))
            env.cmd_switch_step.fill_(step)
            self._record_buffers(nx, ny * nw, env.cmd_cell_ids)  # the bin is the cell key
            return ev

        (cells, ccells), head, rates = self._drive("_cmd_graph", key, num_steps, graph, env.eval_command_cells,
                                                   prepare, cleanup=env.clear_command_schedule)
        self.last_cmd_cells, self.last_cmd_bins = ccells, bins
        w = self.mass * self.gravity
        both = lambda c, p, cmd: {**cell_report(c, dt, w), **command_cell_report(p, dt, cmd)}  # noqa: E731
        total = both(cells.reshape(-1, cells.shape[2]).sum(0), ccells.reshape(-1, ccells.shape[2]).sum(0), (0.0, 0.0, 0.0))
        del total["achieved"], total["gain"]  # (means over different commands say nothing)
        out = {**head, "vx": vx, "vy": vy, "yaw": yaw, "start": start, "switch_step": step,
               "switch_at_s": step * dt, "steady_after": steady, "settle_tol": float(settle_tol),
               "yaw_tol": float(yaw_tol), "total": total,
               "bins": [[[both(cells[ix, iy * nw + iw], ccells[ix, iy * nw + iw], (vx[ix], vy[iy], yaw[iw]))
                          for iw in range(nw)] for iy in range(ny)] for ix in range(nx)], **rates}
        self._attach_records(total, [b for plane in out["bins"] for row in plane for b in row])
        return out

    # ------------------------------------------------------------------ external force
    def run_force_test(self, forces, directions=8, at_s=2.0, for_s=None, point=(0.0, 0.0, 0.0), command=(0.5, 0.0, 0.0),
                       steady_after_s=1.0, settle_tol=0.3, yaw_tol=0.3, num_steps=None, graph=True, trace_depth=None,
                       gait=False, joints=False, contacts=False):
        """How many newtons from which side does the policy hold its course against, and how far
        does it get deflected: one run in which every env holds `command` = (vx, vy, yaw rate)
        through the command schedule (one segment from step 0, so a reset env holds it again) and,
        from episode step round(at_s / dt) on, takes the sustained external force of its bin on its
        base (include/lgx.h ABI 16; force index f, direction index d): forces[f] * (cos t, sin t, 0)
        N with t = 2 pi d / directions from the robot's forward axis towards its left, at `point`
        (m, base link frame), for round(for_s / dt) steps (None: to the end of the episode). Envs
        get bins by randperm(num_envs, seeded with env.seed) % (F * D). Force 0 gives the control
        row.

        The per-env record is the step-response record of the command test with the onset as its
        switch step (env.cmd_eval_buffers: the bin is the cell key; no record kernel of its own),
        and this mode's captured loop is a graph of its own. The env needs the command schedule and
        the force buffers before any of its steps is captured (commands.scheduled_commands and
        domain_rand.scheduled_forces = True, or call this before run()). Both schedules are cleared
        in place when the run ends, so a following run() is the plain one.

        trace_depth, gait, joints, contacts: as in run(), the records per bin.

        Returns the report: "bins"[f][d] with the REPORT_KEYS entries and forced (finished envs
        with samples after the onset), survivors (timed out among them), mean_peak_tilt_rad,
        mean_settle_s (the survivors' mean time from the onset until the tracking error stays within
        settle_tol; 0: never off), achieved [vx, vy, yaw] (the survivors' mean velocities over the
        samples from steady_after_s after the onset on), deflection (achieved minus command) and
        compliance_m_per_s_per_n (the deflection projected on the force direction, over the force;
        None at force 0); achieved, deflection and compliance are None when for_s is given (the
        steady window would mix forced and free samples). "total" likewise without deflection and
        compliance; forces_n, directions_deg, onset_step, force_steps (None: to the end), point,
        command, steady_after, the tolerances. None where there is no data, never NaN.
        ValueError: no forces or directions, a negative or non-finite force, a non-finite point or
        command, an onset outside 0 < step < max_episode_length, a for_s shorter than one step, a
        negative or non-finite tolerance or steady_after_s."""
        env = self.env
        self._set_trace(trace_depth, gait, joints, contacts)
        forces, point, command = ([float(v) for v in lst] for lst in (forces, point, command))
        F, D = len(forces), int(directions)
        if F < 1 or D < 1 or not all(math.isfinite(v) and v >= 0.0 for v in forces):
            raise ValueError(f"force test: need at least one finite force >= 0 and one direction (got {forces}, {directions})")
        if len(point) != 3 or len(command) != 3 or not all(math.isfinite(v) for v in point + command):
            raise ValueError(f"force test: point and command need three finite entries each (got {point}, {command})")
        for name, tol in (("settle_tol", settle_tol), ("yaw_tol", yaw_tol), ("steady_after_s", steady_after_s)):
            if not (math.isfinite(float(tol)) and float(tol) >= 0.0):
                raise ValueError(f"force test: {name} must be finite and >= 0 (got {tol})")
        dt, step = float(env.dt), self._switch_step(at_s, "force test")
        fsteps = None
        if for_s is not None:
            fsteps = int(round(float(for_s) / dt)) if math.isfinite(float(for_s)) else 0
            if fsteps < 1:
                raise ValueError(f"force test: for_s = {for_s} s is shorter than one control step")
        steady = int(round(float(steady_after_s) / dt))
        n = env.num_envs
        bins = self._bins(F * D)
        theta = 2.0 * math.pi * (bins % D).double() / D
        mag = torch.tensor(forces, dtype=torch.float64)[bins // D]
        fvec = torch.stack([mag * torch.cos(theta), mag * torch.sin(theta), torch.zeros_like(mag)], 1).float()
        values = torch.tensor(command + [0.0], dtype=torch.float32).expand(n, 1, 4)
        key = (F, D, float(settle_tol), float(yaw_tol), steady)

        def prepare():
            # before begin: its reset sees the command segment; the force starts after begin, whose
            # reset ends with an env step of its own (the first calls allocate: refused once a loop is captured)
            env.set_command_schedule([0], values)
            env.set_force_schedule(0, fvec, steps=fsteps, point=point)
            ev = self._cmd_eval(key, "_cmd_graph")
            env.cmd_cell_ids.copy_(bins.to(torch.int32))
            env.cmd_switch_step.fill_(step)
            self._record_buffers(F, D, env.cmd_cell_ids)  # the bin is the cell key
            return ev

        def cleanup():
            env.clear_command_schedule()
            env.clear_force_schedule()

        (cells, ccells), head, rates = self._drive(
            "_force_graph", key, num_steps, graph, env.eval_command_cells, prepare,
            lambda: env.set_force_schedule(step, fvec, steps=fsteps, point=point), cleanup)
        self.last_force_cells, self.last_force_bins = ccells, bins
        w = self.mass * self.gravity
        both = lambda c, p, f, t: {**cell_report(c, dt, w), **force_cell_report(p, dt, command, f, t, fsteps is None)}  # noqa: E731
        total = both(cells.reshape(-1, cells.shape[2]).sum(0), ccells.reshape(-1, ccells.shape[2]).sum(0), 0.0, 0.0)
        del total["deflection"], total["compliance_m_per_s_per_n"]  # (means over different forces say nothing)
        out = {**head, "forces_n": forces, "directions_deg": [360.0 * d / D for d in range(D)], "onset_step": step,
               "onset_at_s": step * dt, "force_steps": fsteps, "point": point, "command": command,
               "steady_after": steady, "settle_tol": float(settle_tol), "yaw_tol": float(yaw_tol), "total": total,
               "bins": [[both(cells[f, d], ccells[f, d], forces[f], 2.0 * math.pi * d / D) for d in range(D)]
                        for f in range(F)], **rates}
        self._attach_records(total, [b for row in out["bins"] for b in row])
        return out

    # ------------------------------------------------------------------ sensor model
    def run_sensor_test(self, noise=(1.0,), bias=(0.0,), delay_s=(0.0,), num_steps=None, graph=True, trace_depth=None,
                        gait=False, joints=False, contacts=False):
        """How much observation noise, sensor offset and stale proprioception does the policy
        survive: one run over a noise x bias x latency grid through the step kernel's sensor model
        (lgx_buffers.obs_noise_scale / obs_bias / obs_delay, include/lgx.h ABI 15). Bin index
        (in * |bias| + ib) * |delay_s| + id; envs get bins by randperm(num_envs, seeded with
        env.seed) % bins. Env e of a bin gets the noise scale noise[in] (a multiple of the config's
        own noise amplitude), the constant offset bias[ib] * env.sensor_amplitudes[i] * r[e, i] on
        every sensor channel i (r uniform in [-1, 1], drawn once on the CPU from
        torch.Generator().manual_seed(env.seed): the same for every level and on both backends) and
        the sensing latency round(delay_s[id] / dt) control steps.

        The records go to eval buffers of their own (env.sensor_eval_buffers: the bin is the cell
        key), and this mode's captured loop is a graph of its own, captured once per grid shape and
        flags: the three buffers are written in place, so other level values of the same shape
        replay it. The env needs the buffers before any of its steps is captured
        (domain_rand.sensor_model = True, or call this before run()) and, for a latency, the
        capacity (domain_rand.max_obs_delay_s). The env's own per-env values are put back in place
        when the run ends or fails.

        trace_depth, gait, joints, contacts: as in run(), the records per bin.

        Returns the report: "bins"[in][ib][id] with the REPORT_KEYS entries, "total", noise, bias,
        delay_s, delay_steps. None where there is no data, never NaN.
        ValueError: an empty list, a negative or non-finite entry, a latency beyond the capacity,
        more than one noise level on an env whose config has noise.add_noise off (the levels could
        not differ)."""
        env = self.env
        self._set_trace(trace_depth, gait, joints, contacts)
        noise, bias, delay_s = ([float(v) for v in lst] for lst in (noise, bias, delay_s))
        if min(len(noise), len(bias), len(delay_s)) < 1 or \
                not all(math.isfinite(v) and v >= 0.0 for v in noise + bias + delay_s):
            raise ValueError(f"sensor test: noise, bias and delay_s need at least one finite entry >= 0 each "
                             f"(got {noise}, {bias}, {delay_s})")
        dt = float(env.dt)
        dsteps = [int(round(d / dt)) for d in delay_s]
        cap = int(env._sensor_history_len) if env.obs_delay_steps is not None else 0
        if max(dsteps) > cap:
            raise ValueError(f"sensor test: a latency of {max(dsteps)} control steps is beyond the env's capacity of {cap} "
                             "(domain_rand.max_obs_delay_s)")
        if len(noise) > 1 and not env.cfg.noise.add_noise:
            raise ValueError("sensor test: more than one noise level on an env whose config has noise.add_noise off "
                             "(the levels could not differ)")
        nn, nb, nd = len(noise), len(bias), len(delay_s)
        n, p = env.num_envs, int(env.cfg.env.num_proprio)
        bins = self._bins(nn * nb * nd)
        r = 2.0 * torch.rand(n, p, generator=torch.Generator().manual_seed(int(env.seed))) - 1.0
        scale = torch.tensor(noise, dtype=torch.float32)[bins // (nb * nd)]
        level = torch.tensor(bias, dtype=torch.float32)[(bins // nd) % nb]
        offsets = level.view(n, 1) * env.sensor_amplitudes.cpu().view(1, p) * r
        steps = torch.tensor(dsteps, dtype=torch.float64)[bins % nd]
        saved = []  # (buffer, its values before this run; neutral ones for a buffer this run allocates)

        def prepare():
            had_scale, had_bias = env.obs_noise_scales is not None, env.obs_biases is not None
            for t in (env.obs_noise_scales, env.obs_biases, env.obs_delay_steps):
                if t is not None:
                    saved.append((t, t.clone()))
            env.set_obs_noise_scale(scale.to(env.device))  # (a first call allocates: refused once a loop is captured)
            if not had_scale:
                saved.append((env.obs_noise_scales, torch.ones_like(env.obs_noise_scales)))
            env.set_obs_bias(offsets.to(env.device))
            if not had_bias:
                saved.append((env.obs_biases, torch.zeros_like(env.obs_biases)))
            if env.obs_delay_steps is not None:
                env.set_obs_delay(steps.to(env.device) * dt)
            ev = env.sensor_eval_buffers(nn, nb * nd)
            env.sensor_cell_ids.copy_(bins.to(torch.int32))
            self._record_buffers(nn, nb * nd, env.sensor_cell_ids)  # the bin is the cell key
            return ev

        def restore():
            for buf, old in saved:
                buf.copy_(old)

        cells, head, rates = self._drive("_sensor_graph", (nn, nb, nd), num_steps, graph, env.eval_sensor_cells,
                                         prepare, cleanup=restore)
        self.last_sensor_bins = bins
        w = self.mass * self.gravity
        out = {**head, "noise": noise, "bias": bias, "delay_s": delay_s, "delay_steps": dsteps,
               "total": cell_report(cells.reshape(-1, cells.shape[2]).sum(0), dt, w),
               "bins": [[[cell_report(cells[i, j * nd + k], dt, w) for k in range(nd)] for j in range(nb)]
                        for i in range(nn)], **rates}
        self._attach_records(out["total"], [b for plane in out["bins"] for row in plane for b in row])
        return out

    # ------------------------------------------------------------------ height-scan model
    def run_scan_test(self, noise_m=(0.0,), dropout=(0.0,), offset_x_m=(0.0,), delay_s=(0.0,), num_steps=None, graph=True,
                      trace_depth=None, gait=False, joints=False, contacts=False, dropout_value=1.0):
        """How much scan noise, how many lost points, how much map drift and how stale a map does
        the policy survive: one run over a noise x dropout x offset x latency grid through the step
        kernel's height-scan model (lgx_buffers.scan_noise / scan_dropout / scan_offset / scan_delay,
        include/lgx.h ABI 17). Bin index ((in * |dropout| + ip) * |offset_x_m| + io) * |delay_s| +
        id; envs get bins by randperm(num_envs, seeded with env.seed) % bins. Env e of a bin gets
        the noise amplitude noise_m[in] (m), the dropout probability dropout[ip] (a lost point reads
        dropout_value), the map shift offset_x_m[io] m along its heading (negative: the map lags
        behind) and the scan latency round(delay_s[id] / dt) control steps.

        The records go to eval buffers of their own (env.scan_eval_buffers: the bin is the cell
        key), and this mode's captured loop is a graph of its own, captured once per grid shape and
        flags: the buffers are written in place, so other level values of the same shape replay it.
        The env needs the buffers before any of its steps is captured (domain_rand.scan_model =
        True, or call this before run()) and, for a latency, the capacity
        (domain_rand.max_scan_delay_s). The env's own per-env values are put back in place when the
        run ends or fails. No evaluation kernel of its own: the plain record, reduced per bin.

        trace_depth, gait, joints, contacts: as in run(), the records per bin.

        Returns the report: "bins"[in][ip][io][id] with the REPORT_KEYS entries, "total", noise_m,
        dropout, offset_x_m, delay_s, delay_steps. None where there is no data, never NaN.
        ValueError: an empty list, a non-finite entry, a negative noise, dropout or latency, a
        dropout above 1, a latency beyond the capacity, a task without a height scan."""
        env = self.env
        self._set_trace(trace_depth, gait, joints, contacts)
        noise_m, dropout, offset_x_m, delay_s = ([float(v) for v in lst] for lst in (noise_m, dropout, offset_x_m, delay_s))
        if min(len(noise_m), len(dropout), len(offset_x_m), len(delay_s)) < 1 or \
                not all(math.isfinite(v) for v in noise_m + dropout + offset_x_m + delay_s) or \
                not all(v >= 0.0 for v in noise_m + dropout + delay_s) or max(dropout) > 1.0:
            raise ValueError("scan test: noise_m, dropout, offset_x_m and delay_s need at least one finite entry each, "
                             f"noise_m and delay_s >= 0, dropout in [0, 1] (got {noise_m}, {dropout}, {offset_x_m}, {delay_s})")
        if getattr(env, "_scan_points", 0) <= 0:
            raise ValueError("scan test: this task has no height scan (Go2 task kind, num_scan_obs > 0)")
        dt = float(env.dt)
        dsteps = [int(round(d / dt)) for d in delay_s]
        cap = int(env._scan_delay_cap) if env.scan_delay_steps is not None else 0
        if max(dsteps) > cap:
            raise ValueError(f"scan test: a latency of {max(dsteps)} control steps is beyond the env's capacity of {cap} "
                             "(domain_rand.max_scan_delay_s)")
        nn, np_, no, nd = len(noise_m), len(dropout), len(offset_x_m), len(delay_s)
        bins = self._bins(nn * np_ * no * nd)
        pick = lambda lst, idx: torch.tensor(lst, dtype=torch.float32)[idx]  # noqa: E731
        amp = pick(noise_m, bins // (np_ * no * nd))
        prob = pick(dropout, (bins // (no * nd)) % np_)
        shift = pick(offset_x_m, (bins // nd) % no)
        steps = torch.tensor(dsteps, dtype=torch.float64)[bins % nd]
        saved = []  # (buffer, its values before this run; neutral ones for a buffer this run allocates)

        def prepare():
            had = [t is not None for t in (env.scan_noise_amps, env.scan_dropouts, env.scan_offsets)]
            for t in (env.scan_noise_amps, env.scan_dropouts, env.scan_offsets, env.scan_delay_steps):
                if t is not None:
                    saved.append((t, t.clone()))
            dev = env.device
            env.set_scan_noise(amp.to(dev))  # (a first call allocates: refused once a loop is captured)
            if not had[0]:
                saved.append((env.scan_noise_amps, torch.zeros_like(env.scan_noise_amps)))
            env.set_scan_dropout(prob.to(dev), dropout_value)
            if not had[1]:
                saved.append((env.scan_dropouts, env._neutral_scan_dropout()))
            env.set_scan_offset(shift.to(dev), 0.0, 0.0)
            if not had[2]:
                saved.append((env.scan_offsets, torch.zeros_like(env.scan_offsets)))
            if env.scan_delay_steps is not None:
                env.set_scan_delay(steps.to(dev) * dt)
            ev = env.scan_eval_buffers(nn * np_, no * nd)
            env.scan_cell_ids.copy_(bins.to(torch.int32))
            self._record_buffers(nn * np_, no * nd, env.scan_cell_ids)  # the bin is the cell key
            return ev

        def restore():
            for buf, old in saved:
                buf.copy_(old)

        cells, head, rates = self._drive("_scan_graph", (nn, np_, no, nd), num_steps, graph, env.eval_scan_cells,
                                         prepare, cleanup=restore)
        self.last_scan_bins = bins
        w = self.mass * self.gravity
        flat = cells.reshape(-1, cells.shape[2])
        out = {**head, "noise_m": noise_m, "dropout": dropout, "dropout_value": float(dropout_value),
               "offset_x_m": offset_x_m, "delay_s": delay_s, "delay_steps": dsteps,
               "total": cell_report(flat.sum(0), dt, w),
               "bins": [[[[cell_report(flat[((i * np_ + j) * no + k) * nd + m], dt, w) for m in range(nd)]
                          for k in range(no)] for j in range(np_)] for i in range(nn)], **rates}
        self._attach_records(out["total"], [b for a in out["bins"] for p_ in a for row in p_ for b in row])
        return out

    # ------------------------------------------------------------------ flight recorder
    def traces(self, which="falls", max_envs=16):
        """The recorded traces of chosen envs of the last run (it must have been traced: trace_depth).
        which: "falls" = the envs whose recorded episode ended in a fall or a blow-up (status 2 or
        3), the shortest recorded episode first, ties by env id, the first max_envs of them; or a
        sequence of env ids (max_envs is then ignored). The selection is made and the traces are
        unrolled on the device (lgx_trace_gather); only the selection crosses to the host.

        Returns a dict of numpy arrays: trace [M, K, 76] (oldest row first, newest last, zero rows in
        front of an episode shorter than K), length [M] (rows of trace that hold data), env_id [M],
        status [M] (0 still recording, 1 timed out, 2 fell, 3 blew up), terrain_level / terrain_type
        [M] (-1 without a terrain grid), columns (TRACE_COLUMNS) and dt (seconds per row)."""
        env = self.env
        if self.last_trace_depth is None:
            raise RuntimeError("traces(): the last run was not traced (pass trace_depth= to run, run_push_test or "
                               "run_command_test first)")
        if isinstance(which, str):
            if which != "falls":
                raise ValueError(f"traces(): which must be 'falls' or a sequence of env ids (got {which!r})")
            ids = (env.trace_status >= 2).nonzero().reshape(-1)  # (ascending: the stable sort keeps ties by id)
            ids = ids[torch.sort(env.trace_count[ids], stable=True).indices][:max(int(max_envs), 0)]
        else:
            ids = torch.as_tensor(which).reshape(-1)
        out, out_len = env.trace_gather(ids)
        ids = ids.to(env.device).long()
        grid = getattr(env, "terrain_levels", None) is not None
        none = torch.full_like(ids, -1)
        host = lambda t: t.cpu().numpy()  # noqa: E731
        return {"trace": host(out), "length": host(out_len), "env_id": host(ids), "status": host(env.trace_status[ids]),
                "terrain_level": host(env.terrain_levels[ids] if grid else none),
                "terrain_type": host(env.terrain_types[ids] if grid else none),
                "columns": np.array(TRACE_COLUMNS), "dt": np.float64(env.dt)}

    def sweep_action_delay(self, delays_s, **run_kwargs):
        """One report per actuation latency (seconds) of delays_s, each a full run() with that
        constant latency for all envs. The latency is written in place, so the loop is captured
        once (at the first run) and replayed for every entry; the env's own latencies are back in
        place afterwards."""
        return [self.run(action_delay_s=float(d), **run_kwargs) for d in delays_s]

    def report(self, cells, steps=None, wall=None, graph=None):
        env = self.env
        dt, w = float(env.dt), self.mass * self.gravity
        rows, cols = int(cells.shape[0]), int(cells.shape[1])
        assert cells.shape[2] == _abi.EVAL_CELL_COLS
        total = cells.reshape(-1, _abi.EVAL_CELL_COLS).sum(0)
        out = {**self._head(steps, graph), "terrain_levels": rows, "terrain_types": cols,
               "action_delay_substeps": _min_max(getattr(env, "action_delay_substeps", None), int),
               "motor_strength": _min_max(getattr(env, "motor_strengths", None), float),
               "total": cell_report(total, dt, w),
               "cells": [[cell_report(cells[r, c], dt, w) for c in range(cols)] for r in range(rows)]}
        if wall is not None and steps:
            out.update(self._rates(steps, wall))
        return out
