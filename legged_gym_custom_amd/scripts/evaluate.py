"""evaluate.py — how good is the trained policy: the latest checkpoint of the task's experiment
(loaded as play.py loads it) is run for one episode in every env, on the device, and survival,
command tracking and cost of transport are reported per terrain level x type
(legged_gym_custom_amd/utils/evaluator.py). The terrain and command curricula are switched off
(every env keeps its tile; the command ranges are the configured ones); the rest of the config
stays as trained: observation noise, pushes, friction / mass / gain randomisation.

  python legged_gym/scripts/evaluate.py --task=go2_parkour --num_envs=4096 [--policy student|teacher]
         [--eval_steps N] [--action_delay_ms a[,b,...]] [--motor_strength x]
         [--push_vel v[,v,...] [--push_dirs 8] [--push_at_s 2.0]]
         [--cmd_vx a[,b,...] [--cmd_vy ...] [--cmd_yaw ...] [--cmd_at_s 2.0] [--cmd_start vx,vy,yaw]]
         [--obs_noise a[,b,...]] [--obs_bias a[,b,...]] [--obs_delay_ms a[,b,...]]
         [--scan_noise_m a[,b,...]] [--scan_dropout a[,b,...]] [--scan_offset_m=a[,b,...]] [--scan_delay_ms a[,b,...]]
         [--force_n a[,b,...] [--force_dirs 8] [--force_at_s 2.0] [--force_for_s S] [--force_point x,y,z]
          [--force_cmd vx,vy,yaw]]
         [--trace_falls M [--trace_s 2.0]] [--gait] [--joints] [--contacts]

--action_delay_ms: a constant actuation latency for all envs (the env is built with the action
history the largest one needs); several values give one report each under "sweep", on one captured
loop. --motor_strength: a constant motor strength factor. Without them the config's own actuator
randomisation applies, as trained.

--push_vel: the push-recovery test (PolicyEvaluator.run_push_test): every env is shoved once, --push_at_s
seconds into its episode, by a velocity impulse of one of the given speeds (m/s; 0 gives the control row)
from one of --push_dirs directions in the robot's heading frame; one run fills the speeds x directions
table. The config's own random pushes (domain_rand.push_robots) are switched off for this mode, so the
scheduled push is the only disturbance.

--cmd_vx: the command-response test (PolicyEvaluator.run_command_test): every env holds --cmd_start, switches
--cmd_at_s seconds into its episode to one command of the --cmd_vx x --cmd_vy x --cmd_yaw grid (m/s, m/s, rad/s;
literal commands, the yaw entry is a yaw rate) and is recorded from the switch on: settle times, peak tilt,
achieved velocities and gain per bin. The config's random pushes are switched off for this mode; not with --push_vel.

--obs_noise / --obs_bias / --obs_delay_ms: the sensor test (PolicyEvaluator.run_sensor_test); any of the three
selects it. Every env gets one cell of the noise x bias x latency grid through the step kernel's sensor model:
--obs_noise in multiples of the config's own observation-noise amplitude (needs noise.add_noise for more than one
level), --obs_bias in multiples of the same amplitudes as a constant random offset per env and sensor channel,
--obs_delay_ms as a sensing latency in ms, rounded to control steps. A list that is not given is the neutral one
(1 / 0 / 0). The env is built with domain_rand.sensor_model = True and the sensor history the largest latency needs;
the rest of the config stays as trained. Not with --push_vel, --cmd_vx, --action_delay_ms or --motor_strength.

--scan_noise_m / --scan_dropout / --scan_offset_m / --scan_delay_ms: the scan test (PolicyEvaluator.run_scan_test);
any of the four selects it. Every env gets one cell of the noise x dropout x offset x latency grid through the step
kernel's height-scan model: --scan_noise_m as the amplitude in m of uniform noise per scan point and step,
--scan_dropout as the probability that a point is lost in a step (it then reads --scan_dropout_value, default 1.0:
no return, far), --scan_offset_m as a shift of the whole map along the robot's heading in m (write the list with
"=" when it begins with a minus sign), --scan_delay_ms as the scan's latency in ms, rounded to control steps. A
list that is not given is the neutral one (0). The env is built with domain_rand.scan_model = True and the scan
history the largest latency needs; the rest of the config stays as trained. One line per bin with its survival
rate is printed before the JSON. Tasks with a height scan only (Go2 task kind). Not with the other tests.

--force_n: the force test (PolicyEvaluator.run_force_test): every env holds --force_cmd (default 0.5,0,0) and,
from --force_at_s seconds into its episode on, takes a sustained external force of one of the given magnitudes (N;
0 gives the control row) from one of --force_dirs directions in the robot's heading frame on its base, at
--force_point (m, base link frame), for --force_for_s seconds (default: to the end of the episode); one run fills
the forces x directions table with survival, settle time, peak tilt, the achieved velocity, the deflection and the
compliance (m/s per N) per bin. The config's random pushes are switched off for this mode. Not with --push_vel,
--cmd_vx, the sensor test, --action_delay_ms or --motor_strength.

--trace_falls M: the flight recorder (PolicyEvaluator.traces), valid in every mode: the last --trace_s seconds
of every env's episode are kept in a ring buffer on the device (depth = round(trace_s / dt) steps, clipped to
[1, max_episode_length]; the rings take num_envs x depth x 304 B), and the traces of the M shortest falls are
written to <the JSON's name without .json>_traces.npz (trace [M, depth, 76], length, env_id, status,
terrain_level, terrain_type, columns, dt); the JSON gains "traces": {"file", "envs", "depth"}. With a latency
sweep the traces are those of its last entry.

--gait: gait analysis (PolicyEvaluator.run(gait=True), gait_cell_report), valid in every mode, alone or with
--trace_falls: a per-foot contact state machine runs on the device after every step; every cell (plain run), bin
(push and command tests) and "total" of the JSON gains a "gait" entry: per foot duty factor, stride frequency,
stance / swing time, clearance, slip, load share, touchdown force, step length and stumble share; per body the
flight share, the mean number of feet in contact, the six pair synchronies and a gait label (stand / pronk / trot /
pace / bound / mixed). One summary line per cell or bin with data is printed before the JSON ("gait <where>:
<label>, stride Hz, mean duty factor, slip").

--joints: the joint load (PolicyEvaluator.run(joints=True), joint_cell_report), valid in every mode, alone or with
--gait and --trace_falls: a per-joint record runs on the device after every step; every cell, bin and "total" of
the JSON gains a "joints" entry: per joint the torque saturation share, RMS and peak torque (also over the limit),
positive and braking power, work share, peak power, peak and mean speed, over-speed and out-of-range shares, the
range used and its margin to the soft limits, action rate, clip share and braking share; per body the peak total
power, the shares of samples with any joint saturated / out of range, and flags. For the total one line per joint
is printed before the JSON ("joint total <name>: saturation share, RMS torque / limit, peak speed / limit, range
margin, action rate, flags").

--contacts: where the robot touches the world (PolicyEvaluator.run(contacts=True), contact_cell_report), valid in
every mode, alone or with --gait, --joints and --trace_falls: a per-body record runs on the device after every
step; every cell, bin and "total" of the JSON gains a "contacts" entry: per body the contact share, onsets per
second, mean and peak force, the share of hits on vertical faces, the height above the terrain and the share of
contact onsets on a terrain edge (relief above evaluator.EDGE_RELIEF_M); per cell the collision share, the falls,
which termination body ended them ("fall_causes") and which body was hit hardest at that step. One line per cell
or bin with data is printed before the JSON ("contacts <where>: falls 37: base 62 %, FR_thigh 22 %, no contact
16 %; foot touchdowns on an edge 9 %").

One JSON document is printed and written next to the checkpoint (eval_<policy>.json; a sweep:
eval_<policy>_latency.json; the push test: eval_<policy>_push.json; the command test:
eval_<policy>_command.json; the sensor test: eval_<policy>_sensors.json; the force test:
eval_<policy>_force.json; the scan test: eval_<policy>_scan.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import isaacgym  # noqa: E402,F401  (placeholder, as in play.py)
import torch  # noqa: E402

from legged_gym_custom_amd import LEGGED_GYM_ROOT_DIR  # noqa: E402
from legged_gym.envs import *  # noqa: E402,F401,F403
from legged_gym.utils import get_args, get_load_path, task_registry  # noqa: E402
from legged_gym_custom_amd.utils.evaluator import PolicyEvaluator  # noqa: E402


def evaluate(args, policy="student", eval_steps=None, root=None, graph=True, action_delay_ms=None, motor_strength=None,
             push_vel=None, push_dirs=8, push_at_s=2.0, cmd_vx=None, cmd_vy=None, cmd_yaw=None, cmd_at_s=2.0,
             cmd_start=None, trace_falls=None, trace_s=2.0, gait=False, joints=False, contacts=False, obs_noise=None,
             obs_bias=None, obs_delay_ms=None, force_n=None, force_dirs=8, force_at_s=2.0, force_for_s=None,
             force_point=None, force_cmd=None, scan_noise_m=None, scan_dropout=None, scan_offset_m=None, scan_delay_ms=None,
             scan_dropout_value=1.0):
    env_cfg, train_cfg = task_registry.get_cfgs(name=args.task)
    env_cfg.terrain.curriculum = False
    env_cfg.commands.curriculum = False
    delays_s = [float(ms) / 1000.0 for ms in (action_delay_ms or [])]
    if delays_s:  # the capacity the largest delay needs (never less than the config's own)
        dr = env_cfg.domain_rand
        own = getattr(dr, "max_action_delay_s", getattr(dr, "action_delay_range_s", [0.0, 0.0])[1])
        dr.max_action_delay_s = max(float(own), max(delays_s))
    if push_vel:
        if delays_s or motor_strength is not None:
            raise ValueError("--push_vel is a mode of its own: not with --action_delay_ms / --motor_strength")
        env_cfg.domain_rand.scheduled_pushes = True  # the push buffers exist before any capture
        env_cfg.domain_rand.push_robots = False      # the scheduled push is the only disturbance
    if cmd_vx:
        if push_vel or delays_s or motor_strength is not None:
            raise ValueError("--cmd_vx is a mode of its own: not with --push_vel / --action_delay_ms / --motor_strength")
        env_cfg.commands.scheduled_commands = True  # the schedule buffers exist before any capture
        env_cfg.domain_rand.push_robots = False     # the command switch is the only disturbance
    sensors = any(v is not None for v in (obs_noise, obs_bias, obs_delay_ms))
    if sensors:
        if push_vel or cmd_vx or delays_s or motor_strength is not None:
            raise ValueError("--obs_noise / --obs_bias / --obs_delay_ms are a mode of their own: not with --push_vel / "
                             "--cmd_vx / --action_delay_ms / --motor_strength")
        obs_delay_s = [float(ms) / 1000.0 for ms in (obs_delay_ms or [0.0])]
        dr = env_cfg.domain_rand
        dr.sensor_model = True  # the three buffers exist before any capture
        from legged_gym_custom_amd import params as prm
        # the config's own capacity by the env's rule (a range counts only with its randomisation on)
        own = prm.sensor_model(env_cfg, env_cfg.control.decimation * env_cfg.sim.dt)["max_delay_s"]
        dr.max_obs_delay_s = max([own] + obs_delay_s)  # the capacity the largest latency needs
    if force_n:
        if push_vel or cmd_vx or sensors or delays_s or motor_strength is not None:
            raise ValueError("--force_n is a mode of its own: not with --push_vel / --cmd_vx / --obs_noise / --obs_bias / "
                             "--obs_delay_ms / --action_delay_ms / --motor_strength")
        env_cfg.commands.scheduled_commands = True   # the schedule and the force buffers exist
        env_cfg.domain_rand.scheduled_forces = True  # before any capture
        env_cfg.domain_rand.push_robots = False      # the force is the only disturbance
    scan = any(v is not None for v in (scan_noise_m, scan_dropout, scan_offset_m, scan_delay_ms))
    if scan:
        if push_vel or cmd_vx or sensors or force_n or delays_s or motor_strength is not None:
            raise ValueError("--scan_noise_m / --scan_dropout / --scan_offset_m / --scan_delay_ms are a mode of their own: "
                             "not with --push_vel / --cmd_vx / --obs_* / --force_n / --action_delay_ms / --motor_strength")
        scan_delay_s = [float(ms) / 1000.0 for ms in (scan_delay_ms or [0.0])]
        dr = env_cfg.domain_rand
        dr.scan_model = True  # the buffers exist before any capture
        from legged_gym_custom_amd import params as prm
        own = prm.scan_delay_capacity(env_cfg, env_cfg.control.decimation * env_cfg.sim.dt)[0]
        dr.max_scan_delay_s = max([own] + scan_delay_s)  # the capacity the largest latency needs
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)

    train_cfg.runner.resume = True
    log_root = os.path.join(os.environ.get("LGX_LOG_ROOT") or os.path.join(root or LEGGED_GYM_ROOT_DIR, "logs"),
                            train_cfg.runner.experiment_name)
    runner, train_cfg = task_registry.make_alg_runner(env=env, name=args.task, args=args, train_cfg=train_cfg,
                                                      log_root=log_root)
    checkpoint = get_load_path(log_root, load_run=train_cfg.runner.load_run, checkpoint=train_cfg.runner.checkpoint)
    ev = PolicyEvaluator(env, runner, policy=policy)
    head = dict(task=args.task, checkpoint=checkpoint, iteration=int(runner.current_learning_iteration))
    depth = None
    if trace_falls is not None:
        if int(trace_falls) < 1 or not float(trace_s) > 0.0:
            raise ValueError(f"--trace_falls needs M >= 1 and --trace_s > 0 (got {trace_falls}, {trace_s})")
        depth = min(max(int(round(float(trace_s) / float(env.dt))), 1), int(env.max_episode_length))
    if push_vel:
        report = dict(**head, **ev.run_push_test(push_vel, directions=push_dirs, at_s=push_at_s, num_steps=eval_steps,
                                                 graph=graph, trace_depth=depth, gait=gait, joints=joints, contacts=contacts))
        out = os.path.join(os.path.dirname(checkpoint), f"eval_{policy}_push.json")
    elif cmd_vx:
        report = dict(**head, **ev.run_command_test(cmd_vx, vy=cmd_vy or (0.0,), yaw=cmd_yaw or (0.0,), at_s=cmd_at_s,
                                                    start=cmd_start or (0.0, 0.0, 0.0), num_steps=eval_steps,
                                                    graph=graph, trace_depth=depth, gait=gait, joints=joints, contacts=contacts))
        out = os.path.join(os.path.dirname(checkpoint), f"eval_{policy}_command.json")
    elif sensors:
        report = dict(**head, **ev.run_sensor_test(obs_noise or (1.0,), obs_bias or (0.0,), obs_delay_s, num_steps=eval_steps,
                                                   graph=graph, trace_depth=depth, gait=gait, joints=joints, contacts=contacts))
        out = os.path.join(os.path.dirname(checkpoint), f"eval_{policy}_sensors.json")
    elif force_n:
        report = dict(**head, **ev.run_force_test(force_n, directions=force_dirs, at_s=force_at_s, for_s=force_for_s,
                                                  point=force_point or (0.0, 0.0, 0.0), command=force_cmd or (0.5, 0.0, 0.0),
                                                  num_steps=eval_steps, graph=graph, trace_depth=depth, gait=gait,
                                                  joints=joints, contacts=contacts))
        out = os.path.join(os.path.dirname(checkpoint), f"eval_{policy}_force.json")
    elif scan:
        report = dict(**head, **ev.run_scan_test(scan_noise_m or (0.0,), scan_dropout or (0.0,), scan_offset_m or (0.0,),
                                                 scan_delay_s, num_steps=eval_steps, graph=graph, trace_depth=depth,
                                                 gait=gait, joints=joints, contacts=contacts,
                                                 dropout_value=scan_dropout_value))
        out = os.path.join(os.path.dirname(checkpoint), f"eval_{policy}_scan.json")
    elif len(delays_s) > 1:
        sweep = ev.sweep_action_delay(delays_s, num_steps=eval_steps, graph=graph, motor_strength=motor_strength,
                                      trace_depth=depth, gait=gait, joints=joints, contacts=contacts)
        report = dict(**head, policy=policy, action_delay_ms=[1000.0 * d for d in delays_s], sweep=sweep)
        out = os.path.join(os.path.dirname(checkpoint), f"eval_{policy}_latency.json")
    else:
        report = dict(**head, **ev.run(eval_steps, graph=graph, action_delay_s=delays_s[0] if delays_s else None,
                                       motor_strength=motor_strength, trace_depth=depth, gait=gait, joints=joints, contacts=contacts))
        out = os.path.join(os.path.dirname(checkpoint), f"eval_{policy}.json")
    if depth is not None:
        import numpy as np
        tr = ev.traces("falls", max_envs=int(trace_falls))
        npz = out[:-len(".json")] + "_traces.npz"
        np.savez(npz, **tr)
        report["traces"] = {"file": npz, "envs": int(tr["env_id"].shape[0]), "depth": depth}
    with open(out, "w") as f:
        json.dump(report, f, indent=1)
    return report, out


def scan_summary(report):
    """The survival table of a scan test: one line per bin, then the total."""
    fmt = lambda v, spec: "-" if v is None else format(v, spec)  # noqa: E731
    lines = []

    def line(where, entry, always=False):
        lines.append(f"{where}: survival {fmt(entry['survival_rate'], '.3f')}, fall rate {fmt(entry['fall_rate'], '.3f')}, "
                     f"{entry['episodes']} episodes")

    _each_place(report, line)
    return lines


def gait_summary(report):
    """The human-readable lines of a --gait report: one per cell or bin with data, and the total
    ("-" where it has none)."""
    fmt = lambda v, spec: "-" if v is None else format(v, spec)  # noqa: E731
    lines = []

    def line(where, entry, always=False):
        g = entry.get("gait")
        if g and (always or g["samples"] > 0):
            lines.append(f"gait {where}: {g['gait'] or '-'}, stride {fmt(g['mean_stride_hz'], '.2f')} Hz, duty "
                         f"{fmt(g['mean_duty_factor'], '.2f')}, slip {fmt(g['mean_slip_m_per_stance_s'], '.3f')} m/s, "
                         f"{g['envs']} envs")

    _each_place(report, line)
    return lines


def _each_place(report, line):
    """line(where, entry, always=False) for every cell or bin of a report (of every entry of a
    latency sweep), then for its total with always=True."""
    for i, rep in enumerate(report.get("sweep", [report])):
        tag = f"delay {report['action_delay_ms'][i]:g} ms " if "sweep" in report else ""
        if "speeds" in rep:  # the push test
            for s, row in enumerate(rep["bins"]):
                for d, cell in enumerate(row):
                    line(f"{tag}push {rep['speeds'][s]:g} m/s from {rep['directions_deg'][d]:g} deg", cell)
        elif "forces_n" in rep:  # the force test
            for f, row in enumerate(rep["bins"]):
                for d, cell in enumerate(row):
                    line(f"{tag}force {rep['forces_n'][f]:g} N from {rep['directions_deg'][d]:g} deg", cell)
        elif "offset_x_m" in rep:  # the scan test
            for i, a in enumerate(rep["bins"]):
                for j, b in enumerate(a):
                    for k, c in enumerate(b):
                        for m, cell in enumerate(c):
                            line(f"{tag}scan noise {rep['noise_m'][i]:g} m dropout {rep['dropout'][j]:g} offset "
                                 f"{rep['offset_x_m'][k]:g} m delay {1000.0 * rep['delay_s'][m]:g} ms", cell)
        elif "delay_steps" in rep:  # the sensor test
            for i, a in enumerate(rep["bins"]):
                for j, b in enumerate(a):
                    for k, cell in enumerate(b):
                        line(f"{tag}sensors noise {rep['noise'][i]:g} bias {rep['bias'][j]:g} delay "
                             f"{1000.0 * rep['delay_s'][k]:g} ms", cell)
        elif "vx" in rep:  # the command test
            for ix, a in enumerate(rep["bins"]):
                for iy, b in enumerate(a):
                    for iw, cell in enumerate(b):
                        line(f"{tag}command vx {rep['vx'][ix]:g} vy {rep['vy'][iy]:g} yaw {rep['yaw'][iw]:g}", cell)
        else:
            for r, row in enumerate(rep["cells"]):
                for c, cell in enumerate(row):
                    line(f"{tag}level {r} type {c}", cell)
        line(f"{tag}total", rep["total"], always=True)


def joint_summary(report):
    """The human-readable lines of a --joints report: one per joint of the total (of every entry of
    a latency sweep; "-" where it has no data)."""
    fmt = lambda v, spec: "-" if v is None else format(v, spec)  # noqa: E731
    lines = []
    for i, rep in enumerate(report.get("sweep", [report])):
        tag = f"delay {report['action_delay_ms'][i]:g} ms " if "sweep" in report else ""
        total = rep["total"].get("joints")
        for name, j in (total["joints"] if total else {}).items():
            flags = [f.split(": ", 1)[1] for f in total["flags"] or () if f.startswith(name + ": ")]
            lines.append(f"joint {tag}total {name}: saturated {fmt(j['torque_saturation_share'], '.1%')}, RMS torque "
                         f"{fmt(j['rms_torque_over_limit'], '.2f')} of the limit, peak speed "
                         f"{fmt(j['max_peak_speed_over_limit'], '.2f')} of the limit, range margin "
                         f"{fmt(j['range_margin_rad'], '.3f')} rad, action rate {fmt(j['action_rate_rms'], '.3f')}, "
                         f"flags: {'; '.join(flags) or 'none'}")
    return lines


def contact_summary(report):
    """The human-readable lines of a --contacts report: one per cell or bin with data, and the total:
    which body ended the falls (the largest shares first) and how often the feet land on an edge."""
    lines = []

    def line(where, entry, always=False):
        c = entry.get("contacts")
        if not c or not (always or c["envs"] > 0):
            return
        causes = sorted((c["fall_causes"] or {}).items(), key=lambda kv: (kv[0] == "no_contact", -kv[1]))
        who = ", ".join(f"{'no contact' if k == 'no_contact' else k} {100 * v:.0f} %" for k, v in causes if v > 0)
        edge = c["foot_edge_onset_share"]
        lines.append(f"contacts {where}: falls {c['falls']}{': ' + who if who else ''}; foot touchdowns on an edge "
                     f"{'-' if edge is None else format(100 * edge, '.0f') + ' %'}")

    _each_place(report, line)
    return lines


def main(argv=None):
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--policy", choices=("student", "teacher"), default="student")
    p.add_argument("--eval_steps", type=int, default=None)
    p.add_argument("--action_delay_ms", type=lambda s: [float(v) for v in s.split(",")], default=None)
    p.add_argument("--motor_strength", type=float, default=None)
    p.add_argument("--push_vel", type=lambda s: [float(v) for v in s.split(",")], default=None)
    p.add_argument("--push_dirs", type=int, default=8)
    p.add_argument("--push_at_s", type=float, default=2.0)
    floats = lambda s: [float(v) for v in s.split(",")]  # noqa: E731
    p.add_argument("--cmd_vx", type=floats, default=None)
    p.add_argument("--cmd_vy", type=floats, default=None)
    p.add_argument("--cmd_yaw", type=floats, default=None)
    p.add_argument("--cmd_at_s", type=float, default=2.0)
    p.add_argument("--cmd_start", type=floats, default=None)
    p.add_argument("--obs_noise", type=floats, default=None)
    p.add_argument("--obs_bias", type=floats, default=None)
    p.add_argument("--obs_delay_ms", type=floats, default=None)
    p.add_argument("--scan_noise_m", type=floats, default=None)
    p.add_argument("--scan_dropout", type=floats, default=None)
    p.add_argument("--scan_dropout_value", type=float, default=1.0)
    p.add_argument("--scan_offset_m", type=floats, default=None)
    p.add_argument("--scan_delay_ms", type=floats, default=None)
    p.add_argument("--force_n", type=floats, default=None)
    p.add_argument("--force_dirs", type=int, default=8)
    p.add_argument("--force_at_s", type=float, default=2.0)
    p.add_argument("--force_for_s", type=float, default=None)
    p.add_argument("--force_point", type=floats, default=None)
    p.add_argument("--force_cmd", type=floats, default=None)
    p.add_argument("--trace_falls", type=int, default=None)
    p.add_argument("--trace_s", type=float, default=2.0)
    p.add_argument("--gait", action="store_true")
    p.add_argument("--joints", action="store_true")
    p.add_argument("--contacts", action="store_true")
    own, rest = p.parse_known_args(sys.argv[1:] if argv is None else argv)
    torch.set_float32_matmul_precision("high")
    report, _ = evaluate(get_args(rest), policy=own.policy, eval_steps=own.eval_steps,
                         action_delay_ms=own.action_delay_ms, motor_strength=own.motor_strength,
                         push_vel=own.push_vel, push_dirs=own.push_dirs, push_at_s=own.push_at_s,
                         cmd_vx=own.cmd_vx, cmd_vy=own.cmd_vy, cmd_yaw=own.cmd_yaw, cmd_at_s=own.cmd_at_s,
                         cmd_start=own.cmd_start, trace_falls=own.trace_falls, trace_s=own.trace_s,
                         gait=own.gait, joints=own.joints, contacts=own.contacts, obs_noise=own.obs_noise,
                         obs_bias=own.obs_bias, obs_delay_ms=own.obs_delay_ms, force_n=own.force_n,
                         force_dirs=own.force_dirs, force_at_s=own.force_at_s, force_for_s=own.force_for_s,
                         force_point=own.force_point, force_cmd=own.force_cmd, scan_noise_m=own.scan_noise_m,
                         scan_dropout=own.scan_dropout, scan_offset_m=own.scan_offset_m, scan_delay_ms=own.scan_delay_ms,
                         scan_dropout_value=own.scan_dropout_value)
    for ln in (scan_summary(report) if "offset_x_m" in report else []) + (gait_summary(report) if own.gait else []) + (joint_summary(report) if own.joints else []) + \
            (contact_summary(report) if own.contacts else []):
        print(ln)
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
