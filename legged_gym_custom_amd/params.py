"""Config object -> lgx_task_params (the constants the HIP step and the oracle read).

Every derived constant is computed exactly as the reference derives it, in the same
precision (Python double, then rounded to fp32 where torch would store it):
  dt, max_episode_length, push_interval        legged_robot.py:946-955
  reward scale filtering and *dt, order          legged_robot.py:730-754 (alphabetical)
  soft dof limits (fp32 tensor ops)              legged_robot.py:344-357
  PD gains by joint-name substring               legged_robot.py:704-727
  noise vector                                   go2.py:110-129 / legged_robot.py:594-622
  height points meshgrid(x, y)                   legged_robot.py:980-994
  command resampling interval                    go2.py:393
"""
import math

import numpy as np

from . import _abi
from .utils.helpers import class_to_dict

F32 = np.float32


def reward_terms(cfg, dt):
    """(names, ids, scales_f32, termination_scale or None) in the reference's order."""
    scales = class_to_dict(cfg.rewards.scales)
    names, ids, vals = [], [], []
    term = None
    for key in list(scales.keys()):
        s = scales[key]
        if s == 0:
            continue
        s = s * dt
        if key == "termination":
            term = s
            continue
        if key not in _abi.REWARD_IDS:
            raise NotImplementedError(f"reward term '{key}' has no _reward_{key} implementation")
        names.append(key)
        ids.append(_abi.REWARD_IDS[key])
        vals.append(s)
    return names, ids, vals, term


def go2_proprio_layout(num_dof=12):
    """The Go2 current-observation vector (go2.py:506-515) as ordered (field, width) slots:
    the order the env kernel writes (lgx_env.hip compute_observations) and the deploy
    observation builder fills (deploy/base/deploy_base.py). Phase = sin/cos of the FR, FL,
    BL, BR gait phases (go2.py:497-504)."""
    return (("ang_vel", 3), ("roll_pitch", 2), ("command", 3), ("dof_pos", num_dof), ("dof_vel", num_dof),
            ("actions", num_dof), ("phase", 8))


GO2_PHASE_LEGS = ("fr", "fl", "bl", "br")


def legged_proprio_layout(num_dof=12, num_actions=12, num_heights=0):
    """The LEGGED current-observation vector (legged_robot.py:240-273) as ordered (field, width)
    slots, the order the env kernel writes; heights: the measured-height channels (0 without them)."""
    return (("lin_vel", 3), ("ang_vel", 3), ("gravity", 3), ("command", 3), ("dof_pos", num_dof),
            ("dof_vel", num_dof), ("actions", num_actions), ("heights", num_heights))


# The measured groups of a proprio row (the sensor channels of include/lgx.h, ABI 15) -> the
# noise_scales key and the obs_scales key (None: scale 1) of the group.
SENSOR_GROUPS = {"lin_vel": ("lin_vel", "lin_vel"), "ang_vel": ("ang_vel", "ang_vel"), "roll_pitch": ("imu", None),
                 "gravity": ("gravity", None), "dof_pos": ("dof_pos", "dof_pos"), "dof_vel": ("dof_vel", "dof_vel"),
                 "heights": ("height_measurements", "height_measurements")}


def proprio_layout(cfg, go2):
    """The task's layout function applied to its config."""
    D, A = cfg.env.num_actions, cfg.env.num_actions
    if go2:
        return go2_proprio_layout(D)
    return legged_proprio_layout(D, A, max(int(cfg.env.num_proprio) - (12 + 2 * D + A), 0))


def proprio_channel_groups(cfg, go2):
    """name -> slice of the proprio row, from the layout (not from noise_vector: the Go2 noise
    slots are shifted by one, go2.py:120-127)."""
    out, at = {}, 0
    for name, width in proprio_layout(cfg, go2):
        if width > 0:
            out[name] = slice(at, at + width)
        at += width
    return out


def sensor_obs_scale(cfg, group):
    """The observation scale of a sensor group (physical unit -> observation unit)."""
    key = SENSOR_GROUPS[group][1]
    return 1.0 if key is None else float(getattr(cfg.normalization.obs_scales, key))


def sensor_amplitudes(cfg, go2):
    """[num_proprio] float32: on each sensor channel the amplitude the config's own noise has for
    its group, noise_level * noise_scales.<group> * obs scale, placed by the layout; 0 elsewhere."""
    v = np.zeros(cfg.env.num_proprio, dtype=np.float32)
    ns, lvl = cfg.noise.noise_scales, cfg.noise.noise_level
    for name, sl in proprio_channel_groups(cfg, go2).items():
        if name in SENSOR_GROUPS:
            v[sl] = float(getattr(ns, SENSOR_GROUPS[name][0])) * lvl * sensor_obs_scale(cfg, name)
    return v


def sensor_model(cfg, dt):
    """The sensor-model keys of cfg.domain_rand (all optional, read with getattr: the shipped config
    classes do not carry them) -> dict:
      on             sensor_model: allocate and bind all five buffers up front, with neutral values
      scale_on / scale_range   randomize_obs_noise_scale, obs_noise_scale_range
      bias_on / bias_level_range   randomize_obs_bias, obs_bias_level_range (multiples of sensor_amplitudes)
      delay_on / delay_range_s / max_delay_s   randomize_obs_delay, obs_delay_range_s, max_obs_delay_s
                                               (default: the range's upper end)
      history_len    K = round(max(max_obs_delay_s, max_scan_delay_s) / dt) control steps
                     (lgx_task_params.sensor_history_len; the scan model's ring shares it)
    A ValueError when K exceeds LGX_MAX_SENSOR_HISTORY or a range is not 0 <= lo <= hi."""
    dr = cfg.domain_rand
    delay_on = bool(getattr(dr, "randomize_obs_delay", False))
    lo, hi = (float(v) for v in getattr(dr, "obs_delay_range_s", [0.0, 0.0]))
    max_s = float(getattr(dr, "max_obs_delay_s", hi if delay_on else 0.0))
    if not (0.0 <= lo <= hi) or not max_s >= 0.0:
        raise ValueError(f"domain_rand.obs_delay_range_s {[lo, hi]} / max_obs_delay_s {max_s}: need 0 <= lo <= hi")
    if delay_on and int(round(hi / dt)) > int(round(max_s / dt)):
        raise ValueError(f"domain_rand.obs_delay_range_s upper end {hi} s exceeds max_obs_delay_s {max_s} s")
    # the scan model's ring (ABI 17) has the same K rows: the capacity is the larger of the two
    K = int(round(max(max_s, scan_delay_capacity(cfg, dt)[0]) / dt))
    if K > _abi.MAX_SENSOR_HISTORY:
        raise ValueError(f"domain_rand.max_obs_delay_s / max_scan_delay_s = {max(max_s, scan_delay_capacity(cfg, dt)[0])} s "
                         f"is {K} control steps of sensor history; at most {_abi.MAX_SENSOR_HISTORY} (LGX_MAX_SENSOR_HISTORY)")
    scale_on = bool(getattr(dr, "randomize_obs_noise_scale", False))
    slo, shi = (float(v) for v in getattr(dr, "obs_noise_scale_range", [1.0, 1.0]))
    if scale_on and not (0.0 <= slo <= shi):
        raise ValueError(f"domain_rand.obs_noise_scale_range {[slo, shi]}: need 0 <= lo <= hi")
    bias_on = bool(getattr(dr, "randomize_obs_bias", False))
    blo, bhi = (float(v) for v in getattr(dr, "obs_bias_level_range", [0.0, 0.0]))
    if bias_on and not (0.0 <= blo <= bhi):
        raise ValueError(f"domain_rand.obs_bias_level_range {[blo, bhi]}: need 0 <= lo <= hi")
    return dict(on=bool(getattr(dr, "sensor_model", False)), scale_on=scale_on, scale_range=[slo, shi],
                bias_on=bias_on, bias_level_range=[blo, bhi], delay_on=delay_on, delay_range_s=[lo, hi],
                max_delay_s=max_s, history_len=K)


def scan_delay_capacity(cfg, dt):
    """(max_scan_delay_s, delay_on, [lo, hi]) of cfg.domain_rand: the scan model's latency keys
    randomize_scan_delay, scan_delay_range_s, max_scan_delay_s (default: the range's upper end when
    the randomisation is on). ValueError when the range is not 0 <= lo <= hi or exceeds the capacity."""
    dr = cfg.domain_rand
    delay_on = bool(getattr(dr, "randomize_scan_delay", False))
    lo, hi = (float(v) for v in getattr(dr, "scan_delay_range_s", [0.0, 0.0]))
    max_s = float(getattr(dr, "max_scan_delay_s", hi if delay_on else 0.0))
    if not (0.0 <= lo <= hi) or not max_s >= 0.0:
        raise ValueError(f"domain_rand.scan_delay_range_s {[lo, hi]} / max_scan_delay_s {max_s}: need 0 <= lo <= hi")
    if delay_on and int(round(hi / dt)) > int(round(max_s / dt)):
        raise ValueError(f"domain_rand.scan_delay_range_s upper end {hi} s exceeds max_scan_delay_s {max_s} s")
    return max_s, delay_on, [lo, hi]


def scan_model(cfg, dt):
    """The height-scan model's keys of cfg.domain_rand (include/lgx.h ABI 17; all optional, read with
    getattr: the shipped config classes do not carry them) -> dict:
      on             scan_model: allocate and bind the buffers up front, with neutral values
      noise_on / noise_range       randomize_scan_noise, scan_noise_range (m)
      dropout_on / dropout_range / dropout_value
                                   randomize_scan_dropout, scan_dropout_range (probability),
                                   scan_dropout_value (what a lost point reads, default 1.0)
      offset_on / offset_xy_range / offset_z_range
                                   randomize_scan_offset, scan_offset_xy_range (m, the length of a
                                   shift in a random direction), scan_offset_z_range (m, lo <= hi)
      delay_on / delay_range_s / max_delay_s
                                   randomize_scan_delay, scan_delay_range_s, max_scan_delay_s
      delay_steps    round(max_scan_delay_s / dt): > 0 = the scan ring exists (its K rows are
                     sensor_model's history_len, the larger of the two capacities)
      any            one of the above asks for a buffer
    A ValueError for a bad range: 0 <= lo <= hi (dropout: hi <= 1; z: lo <= hi), |dropout value| <= 1."""
    dr = cfg.domain_rand
    max_s, delay_on, delay_range = scan_delay_capacity(cfg, dt)

    def rng(key, default, lo_min=0.0, hi_max=math.inf):
        lo, hi = (float(v) for v in getattr(dr, key, default))
        if not (lo_min <= lo <= hi <= hi_max):
            raise ValueError(f"domain_rand.{key} {[lo, hi]}: need {lo_min:g} <= lo <= hi <= {hi_max:g}")
        return [lo, hi]

    noise_range = rng("scan_noise_range", [0.0, 0.0])
    dropout_range = rng("scan_dropout_range", [0.0, 0.0], hi_max=1.0)
    xy_range = rng("scan_offset_xy_range", [0.0, 0.0])
    z_range = rng("scan_offset_z_range", [0.0, 0.0], lo_min=-math.inf)
    value = float(getattr(dr, "scan_dropout_value", 1.0))
    if not abs(value) <= 1.0:
        raise ValueError(f"domain_rand.scan_dropout_value {value}: a scan value, |value| <= 1")
    out = dict(on=bool(getattr(dr, "scan_model", False)),
               noise_on=bool(getattr(dr, "randomize_scan_noise", False)), noise_range=noise_range,
               dropout_on=bool(getattr(dr, "randomize_scan_dropout", False)), dropout_range=dropout_range,
               dropout_value=value,
               offset_on=bool(getattr(dr, "randomize_scan_offset", False)), offset_xy_range=xy_range,
               offset_z_range=z_range, delay_on=delay_on, delay_range_s=delay_range, max_delay_s=max_s,
               delay_steps=int(round(max_s / dt)))
    out["any"] = out["on"] or out["noise_on"] or out["dropout_on"] or out["offset_on"] or out["delay_steps"] > 0
    return out


def noise_vector(cfg, go2):
    p = cfg.env.num_proprio
    v = np.zeros(p, dtype=np.float32)
    ns, lvl, sc = cfg.noise.noise_scales, cfg.noise.noise_level, cfg.normalization.obs_scales
    if go2:  # go2.py:120-127 — note the slot offsets (Appendix B Q1)
        v[0:3] = ns.ang_vel * lvl * sc.ang_vel
        v[3:5] = ns.imu * lvl
        v[5:8] = 0.0
        v[8:9] = 0.0
        v[9:21] = ns.dof_pos * lvl * sc.dof_pos
        v[21:33] = ns.dof_vel * lvl * sc.dof_vel
        v[33:45] = 0.0
        v[45:53] = 0.0
    else:  # legged_robot.py:611-621
        v[:3] = ns.lin_vel * lvl * sc.lin_vel
        v[3:6] = ns.ang_vel * lvl * sc.ang_vel
        v[6:9] = ns.gravity * lvl
        v[9:12] = 0.0
        v[12:24] = ns.dof_pos * lvl * sc.dof_pos
        v[24:36] = ns.dof_vel * lvl * sc.dof_vel
        v[36:48] = 0.0
        if cfg.terrain.measure_heights:
            v[48:235] = ns.height_measurements * lvl * sc.height_measurements
    return v


def soft_dof_limits(lower, upper, soft):
    lo = np.asarray(lower, dtype=F32)
    hi = np.asarray(upper, dtype=F32)
    m = (lo + hi) / F32(2)
    r = hi - lo
    return np.stack([m - (F32(0.5) * r) * F32(soft), m + (F32(0.5) * r) * F32(soft)], 1).astype(F32)


def actuator_randomisation(cfg, sim_dt):
    """The actuator keys of cfg.domain_rand (all optional, read with getattr: the shipped config
    classes do not carry them) -> dict:
      delay_on / delay_range_s [lo, hi] / max_delay_s   randomize_action_delay, action_delay_range_s,
                                                        max_action_delay_s (default: the range's upper end)
      strength_on / strength_range                      randomize_motor_strength, motor_strength_range
      history_len   H = ceil(round(max_action_delay_s / sim_dt) / decimation): the control steps of
                    action history the largest latency needs (lgx_task_params.action_history_len)
    A ValueError when H exceeds LGX_MAX_ACTION_HISTORY or a range is not 0 <= lo <= hi."""
    dr = cfg.domain_rand
    delay_on = bool(getattr(dr, "randomize_action_delay", False))
    lo, hi = (float(v) for v in getattr(dr, "action_delay_range_s", [0.0, 0.0]))
    max_s = float(getattr(dr, "max_action_delay_s", hi))
    if not (0.0 <= lo <= hi) or max_s < 0.0:
        raise ValueError(f"domain_rand.action_delay_range_s {[lo, hi]} / max_action_delay_s {max_s}: need 0 <= lo <= hi")
    if delay_on and hi > max_s:
        raise ValueError(f"domain_rand.action_delay_range_s upper end {hi} s exceeds max_action_delay_s {max_s} s")
    n = int(cfg.control.decimation)
    max_sub = int(round(max_s / sim_dt))
    H = -(-max_sub // n)
    if H > _abi.MAX_ACTION_HISTORY:
        raise ValueError(f"domain_rand.max_action_delay_s = {max_s} s is {max_sub} physics substeps = {H} control steps "
                         f"of action history; at most {_abi.MAX_ACTION_HISTORY} (LGX_MAX_ACTION_HISTORY)")
    slo, shi = (float(v) for v in getattr(dr, "motor_strength_range", [0.9, 1.1]))
    strength_on = bool(getattr(dr, "randomize_motor_strength", False))
    if strength_on and not (0.0 <= slo <= shi):
        raise ValueError(f"domain_rand.motor_strength_range {[slo, shi]}: need 0 <= lo <= hi")
    return dict(delay_on=delay_on, delay_range_s=[lo, hi], max_delay_s=max_s, history_len=H,
                strength_on=strength_on, strength_range=[slo, shi])


def scheduled_pushes(cfg):
    """cfg.domain_rand.scheduled_pushes (optional, read with getattr: the shipped config classes do
    not carry it; set it on a config instance): allocate and bind the scheduled-push buffers
    (lgx_buffers.push_step / push_dvel, include/lgx.h ABI 9) when the env is built, so that
    env.set_push_schedule never has to re-bind (which a captured graph would not see)."""
    return bool(getattr(cfg.domain_rand, "scheduled_pushes", False))


def external_force(cfg, dt):
    """The external-force keys of cfg.domain_rand (all optional, read with getattr: the shipped
    config classes do not carry them; set them on a config instance) -> dict:
      alloc      scheduled_forces or randomize_external_force: allocate and bind the force buffers
                 (lgx_buffers.force_window / force_vec, include/lgx.h ABI 16) when the env is built,
                 so that env.set_force_schedule never has to re-bind
      on / range_n [lo, hi]   randomize_external_force, external_force_range (N, the magnitude)
      steps      round(external_force_duration_s / dt) control steps the force lasts, at least 1
      period     round(external_force_interval_s / dt) control steps from one onset to the next
    A ValueError when the randomisation is on and the range is not 0 <= lo <= hi, the duration is
    not positive or the interval is shorter than one control step."""
    dr = cfg.domain_rand
    on = bool(getattr(dr, "randomize_external_force", False))
    lo, hi = (float(v) for v in getattr(dr, "external_force_range", [0.0, 0.0]))
    dur = float(getattr(dr, "external_force_duration_s", 1.0))
    itv = float(getattr(dr, "external_force_interval_s", 5.0))
    steps, period = max(int(round(dur / dt)), 1), int(round(itv / dt))
    if on and (not (0.0 <= lo <= hi) or not dur > 0.0 or period < 1):
        raise ValueError(f"domain_rand.external_force_range {[lo, hi]} N / external_force_duration_s {dur} / "
                         f"external_force_interval_s {itv}: need 0 <= lo <= hi, a positive duration and an interval "
                         "of at least one control step")
    return {"alloc": on or bool(getattr(dr, "scheduled_forces", False)), "on": on, "range_n": (lo, hi),
            "steps": steps, "period": period}


def scheduled_commands(cfg):
    """cfg.commands.scheduled_commands (optional, read with getattr as scheduled_pushes is): allocate
    and bind the command schedule buffers (lgx_buffers.cmd_step / cmd_val, include/lgx.h ABI 10) when
    the env is built, so that env.set_command_schedule never has to re-bind."""
    return bool(getattr(cfg.commands, "scheduled_commands", False))


def build_task_params(cfg, model, num_envs, num_envs_total=None, env_id_offset=0, sim_dt=None, go2=True,
                      terrain_shape=None):
    P = _abi.TaskParams()
    P.abi_version = _abi.ABI_VERSION
    P.task_kind = _abi.TASK_GO2 if go2 else _abi.TASK_LEGGED
    P.num_envs = num_envs
    P.num_envs_total = num_envs_total or num_envs
    P.env_id_offset = env_id_offset
    D = len(model["dof_names"])
    names = model["body_names"]
    P.num_dof = D
    P.num_bodies = len(names)
    P.num_actions = cfg.env.num_actions
    P.num_proprio = cfg.env.num_proprio
    P.history_len = cfg.env.history_buffer_length
    P.num_obs = cfg.env.num_observations
    P.num_priv = cfg.env.num_privileged_obs
    P.num_est = cfg.env.num_estimated_obs
    P.num_scan = cfg.env.num_scan_obs
    P.num_critic = cfg.env.num_critic_obs
    P.decimation = cfg.control.decimation
    sdt = sim_dt if sim_dt is not None else cfg.sim.dt
    dt = cfg.control.decimation * sdt
    P.sim_dt = sdt
    P.dt = dt
    P.action_scale = cfg.control.action_scale
    P.clip_actions = cfg.normalization.clip_actions
    P.clip_obs = cfg.normalization.clip_observations
    P.control_type = _abi.CONTROL[cfg.control.control_type]
    dr = cfg.domain_rand
    P.randomize_kp_kd = int(getattr(dr, "randomize_kp_kd", False))
    P.action_history_len = actuator_randomisation(cfg, sdt)["history_len"]
    P.sensor_history_len = sensor_model(cfg, dt)["history_len"]
    links = model["links"][1:]
    for i, dn in enumerate(model["dof_names"]):
        P.default_dof_pos[i] = cfg.init_state.default_joint_angles[dn]
        kp = kd = 0.0
        for key in cfg.control.stiffness.keys():
            if key in dn:
                kp, kd = cfg.control.stiffness[key], cfg.control.damping[key]
        P.p_gains[i], P.d_gains[i] = kp, kd
        P.torque_limits[i] = links[i]["effort"]
        P.dof_vel_limits[i] = links[i]["velocity"]
    lim = soft_dof_limits([l["lower"] for l in links], [l["upper"] for l in links], cfg.rewards.soft_dof_pos_limit)
    for i in range(D):
        P.dof_pos_limits[i][0], P.dof_pos_limits[i][1] = float(lim[i, 0]), float(lim[i, 1])
    P.soft_dof_vel_limit = getattr(cfg.rewards, "soft_dof_vel_limit", 1.0)
    P.soft_torque_limit = getattr(cfg.rewards, "soft_torque_limit", 1.0)
    sc = cfg.normalization.obs_scales
    P.obs_scale_lin_vel, P.obs_scale_ang_vel = sc.lin_vel, sc.ang_vel
    P.obs_scale_dof_pos, P.obs_scale_dof_vel, P.obs_scale_height = sc.dof_pos, sc.dof_vel, sc.height_measurements
    P.add_noise = int(cfg.noise.add_noise)
    nv = noise_vector(cfg, go2)
    for i in range(len(nv)):
        P.noise_vec[i] = float(nv[i])
    P.measure_heights = int(cfg.terrain.measure_heights)
    xs, ys = cfg.terrain.measured_points_x, cfg.terrain.measured_points_y
    P.num_height_points = len(xs) * len(ys)
    for i, x in enumerate(xs):
        for j, y in enumerate(ys):
            P.height_points[i * len(ys) + j][0] = x
            P.height_points[i * len(ys) + j][1] = y
    # commands
    c = cfg.commands
    P.heading_command = int(c.heading_command)
    P.zero_command = int(getattr(c, "zero_command", False))
    P.zero_command_prob = getattr(c, "zero_command_prob", 0.0)
    P.resample_interval = int(c.resampling_time / dt)
    P.has_user_command = int(len(getattr(c, "user_command", [])) > 0)
    for i, v in enumerate(getattr(c, "user_command", [])[:4]):
        P.user_command[i] = v
    P.cmd_lin_vel_x[:] = c.ranges.lin_vel_x
    P.cmd_lin_vel_y[:] = c.ranges.lin_vel_y
    P.cmd_ang_vel_yaw[:] = c.ranges.ang_vel_yaw
    P.cmd_heading[:] = c.ranges.heading
    P.heading_error_gain = getattr(c, "heading_error_gain", 0.5)
    P.commands_scale[:] = [sc.lin_vel, sc.lin_vel, sc.ang_vel]
    e = cfg.env
    P.period = getattr(e, "period", 1.0)
    P.offset_fl, P.offset_fr = getattr(e, "fl_offset", 0.0), getattr(e, "fr_offset", 0.0)
    P.offset_bl, P.offset_br = getattr(e, "bl_offset", 0.0), getattr(e, "br_offset", 0.0)
    P.max_episode_length_s = e.episode_length_s
    P.max_episode_length = int(np.ceil(e.episode_length_s / dt))
    P.parkour = int(getattr(cfg.terrain, "parkour", False))
    # body index tables (legged_robot.py:846-894, go2.py:40-77)
    feet = [i for i, n in enumerate(names) if cfg.asset.foot_name in n]
    pen, term = [], []
    for key in cfg.asset.penalize_contacts_on:
        pen.extend([i for i, n in enumerate(names) if key in n])
    for key in cfg.asset.terminate_after_contacts_on:
        term.extend([i for i, n in enumerate(names) if key in n])
    P.num_feet = len(feet)
    P.n_termination, P.n_penalised = len(term), len(pen)
    for i, v in enumerate(term):
        P.termination_idx[i] = v
    for i, v in enumerate(pen):
        P.penalised_idx[i] = v
    for i, v in enumerate(feet[: _abi.MAX_FEET]):
        P.feet_idx[i] = v
    calves = [i for i, n in enumerate(names) if "calf" in n]
    for i, v in enumerate(calves[:4]):
        P.calf_idx[i] = v
    dn = model["dof_names"]
    for i, leg in enumerate(("FL", "FR", "RL", "RR")):
        for arr, j in ((P.hip_joint_idx, "hip"), (P.thigh_joint_idx, "thigh"), (P.calf_joint_idx, "calf")):
            name = f"{leg}_{j}_joint"
            arr[i] = dn.index(name) if name in dn else 0
    # rewards
    rn, rid, rs, term_scale = reward_terms(cfg, dt)
    P.num_reward_terms = len(rid)
    for i, (a, b) in enumerate(zip(rid, rs)):
        P.reward_ids[i] = a
        P.reward_scales[i] = b
    # command curriculum (go2.py:80-107 / legged_robot.py:580-591; lgx.h command_curriculum)
    c = cfg.commands
    if getattr(c, "curriculum", False):
        if "tracking_lin_vel" not in rn:
            # the reference indexes episode_sums['tracking_lin_vel'] (KeyError without the term)
            raise KeyError("commands.curriculum needs the tracking_lin_vel reward term")
        P.curriculum_term = rn.index("tracking_lin_vel")
        P.curriculum_threshold = float(np.float32(0.8 * rs[P.curriculum_term]))
        if go2:
            P.command_curriculum = 1
            P.curriculum_delta = float(c.vel_increment)
            P.curriculum_lo_min = float(c.max_reverse_vel)
            P.curriculum_lo_max = 0.0
            P.curriculum_lo_free = int(c.max_reverse_vel >= 0.0)
            P.curriculum_hi_max = float(c.max_forward_vel)
        else:
            P.command_curriculum = 2
            P.curriculum_delta = 0.05
            P.curriculum_lo_min = -float(c.max_curriculum)
            P.curriculum_lo_max = 0.0
            P.curriculum_hi_max = float(c.max_curriculum)
    P.only_positive_rewards = int(cfg.rewards.only_positive_rewards)
    P.has_termination_reward = int(term_scale is not None)
    P.termination_scale = term_scale or 0.0
    r = cfg.rewards
    P.tracking_sigma = r.tracking_sigma
    P.base_height_target = r.base_height_target
    P.max_foot_height = getattr(r, "max_foot_height", 0.0)
    P.percent_time_on_ground = getattr(r, "percent_time_on_ground", 0.5)
    P.max_contact_force = r.max_contact_force
    P.pitch_deg_target = getattr(r, "pitch_deg_target", 0.0)
    P.roll_deg_target = getattr(r, "roll_deg_target", 0.0)
    # events
    P.push_robots = int(getattr(dr, "push_robots", False))
    P.push_interval = int(np.ceil(getattr(dr, "push_interval_s", 15) / dt))
    P.max_push_vel_xy = getattr(dr, "max_push_vel_xy", 0.0)
    ist = cfg.init_state
    P.base_init_state[:] = list(ist.pos) + list(ist.rot) + list(ist.lin_vel) + list(ist.ang_vel)
    t = cfg.terrain
    P.mesh_type = {"plane": _abi.MESH_PLANE, "heightfield": _abi.MESH_HEIGHTFIELD,
                   "trimesh": _abi.MESH_TRIMESH}.get(t.mesh_type, _abi.MESH_PLANE)
    P.custom_origins = int(t.mesh_type in ("heightfield", "trimesh"))
    P.horizontal_scale, P.vertical_scale, P.border_size = t.horizontal_scale, t.vertical_scale, t.border_size
    P.curriculum = int(t.curriculum and t.mesh_type in ("heightfield", "trimesh"))
    P.terrain_length = t.terrain_length
    P.promote_threshold, P.demote_threshold = t.promote_threshold, t.demote_threshold
    P.num_terrain_rows, P.num_terrain_cols = t.num_rows, t.num_cols
    P.max_terrain_level = t.num_rows
    if terrain_shape is not None:  # Terrain.tot_rows, tot_cols (terrain.py:29-31)
        P.hf_rows, P.hf_cols = int(terrain_shape[0]), int(terrain_shape[1])
    # physics
    P.gravity[:] = cfg.sim.gravity
    P.ground_friction = t.static_friction
    P.solver_iterations = max(4, int(cfg.sim.physx.num_position_iterations) * 2)
    P.baumgarte = 0.2
    P.slop = 0.001
    P.max_depenetration_vel = cfg.sim.physx.max_depenetration_velocity
    P.contact_margin = cfg.sim.physx.contact_offset
    P.limit_margin = 0.01
    return P
