"""Policy evaluation throughput (dev tool): PolicyEvaluator on a task with randomly initialised
networks (the timing does not depend on the weights), graph replay and the eager loop alternated.

  python tools/eval_bench.py [--task go2] [--num_envs 4096] [--steps N] [--repeats 3] [--out FILE]
  python tools/eval_bench.py --push_vel 0,0.5,1.0,1.5 [--push_dirs 8] ...   # + the push test (run_push_test)
  python tools/eval_bench.py --force_n 0,20,40,80 [--force_dirs 8] ...   # + the force test (run_force_test)
  python tools/eval_bench.py --scan_offset_m=-0.1,0,0.1 [--scan_noise_m ..] [--scan_dropout ..] [--scan_delay_ms 0,40,80] ...
                                                     # + the scan test (run_scan_test; --task go2 or go2_parkour)
  python tools/eval_bench.py --trace_depth 100 ...   # + the plain run with the flight recorder on, and traces()
  python tools/eval_bench.py --gait ...   # + the plain run with the gait record on (run(gait=True))
  python tools/eval_bench.py --joints ...   # + the plain run with the joint-load record on (run(joints=True))
  python tools/eval_bench.py --contacts ...   # + the plain run with the contact record on (run(contacts=True))
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/eval_bench.py --profile
  python tools/eval_bench.py --stats DIR/..._kernel_stats.csv --merge FILE   # kernel times into FILE

Times are host clocks around runs that end in the evaluator's host read (a device synchronise);
--profile runs one short eager evaluation only, and one short eager command test with --cmd_vx (kernel
times come from the trace, not from here)."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {"eval_accumulate_kernel": "eval_accumulate_us", "eval_reduce_kernel": "eval_reduce_us",
           "eval_cmd_reduce_kernel": "eval_cmd_reduce_us",
           "env_step_kernel": "env_step_us", "act_kernel(lgx_s8_act_args": "act_us",
           "trace_record_kernel": "trace_record_us", "trace_gather_kernel": "trace_gather_us",
           "gait_record_kernel": "gait_record_us", "gait_reduce_kernel": "gait_reduce_us",
           "joint_record_kernel": "joint_record_us", "joint_reduce_kernel": "joint_reduce_us",
           "contact_record_kernel": "contact_record_us", "contact_reduce_kernel": "contact_reduce_us",
           "contact_begin_kernel": "contact_begin_us"}


def merge_stats(stats_csv, out):
    """Average kernel times (us) of the evaluation's kernels from a rocprofv3 --stats CSV."""
    doc = json.load(open(out)) if os.path.exists(out) else {}
    k = doc.setdefault("kernel_trace", {"source": "rocprofv3 --kernel-trace --stats, eager evaluation"})
    for row in csv.DictReader(open(stats_csv)):
        for pat, key in KERNELS.items():
            if pat in row["Name"]:
                k[key] = round(float(row["AverageNs"]) / 1e3, 2)
                k[key.replace("_us", "_calls")] = int(row["Calls"])
    json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps(k))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--task", default="go2")
    p.add_argument("--num_envs", type=int, default=4096)
    p.add_argument("--steps", type=int, default=None)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--device", default="cuda:0", help="cpu: a rehearsal of the tool, not a measurement")
    p.add_argument("--push_vel", type=lambda s: [float(v) for v in s.split(",")], default=None,
                   help="also time run_push_test with these speeds (the env is built with scheduled_pushes)")
    p.add_argument("--push_dirs", type=int, default=8)
    p.add_argument("--cmd_vx", type=lambda s: [float(v) for v in s.split(",")], default=None,
                   help="also time run_command_test with these forward commands (the env is built with "
                        "scheduled_commands; not with --push_vel)")
    p.add_argument("--cmd_vy", type=lambda s: [float(v) for v in s.split(",")], default=[0.0])
    p.add_argument("--cmd_yaw", type=lambda s: [float(v) for v in s.split(",")], default=[0.0])
    p.add_argument("--force_n", type=lambda s: [float(v) for v in s.split(",")], default=None,
                   help="also time run_force_test with these forces (the env is built with scheduled_commands and "
                        "scheduled_forces; not with --push_vel or --cmd_vx)")
    p.add_argument("--force_dirs", type=int, default=8)
    floats = lambda s: [float(v) for v in s.split(",")]  # noqa: E731
    p.add_argument("--scan_noise_m", type=floats, default=None,
                   help="also time run_scan_test over this grid (any of the four --scan_* lists; the env is built with "
                        "domain_rand.scan_model and the scan history the largest latency needs; not with the other tests)")
    p.add_argument("--scan_dropout", type=floats, default=None)
    p.add_argument("--scan_offset_m", type=floats, default=None)
    p.add_argument("--scan_delay_ms", type=floats, default=None)
    p.add_argument("--trace_depth", type=int, default=None,
                   help="also time run(trace_depth=K), the flight recorder, and traces('falls', 16) after it")
    p.add_argument("--gait", action="store_true", help="also time run(gait=True), the gait record")
    p.add_argument("--joints", action="store_true", help="also time run(joints=True), the joint-load record")
    p.add_argument("--contacts", action="store_true", help="also time run(contacts=True), the contact record")
    p.add_argument("--profile", action="store_true")
    p.add_argument("--stats")
    p.add_argument("--merge")
    p.add_argument("--out")
    a = p.parse_args()
    scan = any(v is not None for v in (a.scan_noise_m, a.scan_dropout, a.scan_offset_m, a.scan_delay_ms))
    assert sum(bool(v) for v in (a.push_vel, a.cmd_vx, a.force_n, scan)) <= 1, \
        "--push_vel, --cmd_vx, --force_n or --scan_*, one at a time"
    if a.stats:
        return merge_stats(a.stats, a.merge)
    import torch
    from legged_gym_custom_amd.envs import task_registry, task_registry_configs
    from legged_gym_custom_amd.utils.evaluator import PolicyEvaluator
    from legged_gym_custom_amd.utils.helpers import get_args
    assert a.device == "cpu" or torch.cuda.is_available(), "eval_bench needs an MI355X"
    cfg, tcfg = task_registry_configs(a.task)
    cfg.seed = tcfg.seed = 1
    cfg.terrain.curriculum = cfg.commands.curriculum = False
    if a.push_vel:
        cfg.domain_rand.scheduled_pushes = True  # buffers bound with no env scheduled: the plain run's step is unchanged
    if a.cmd_vx:
        cfg.commands.scheduled_commands = True  # likewise: bound, every entry unused
    if a.force_n:
        cfg.commands.scheduled_commands = cfg.domain_rand.scheduled_forces = True  # likewise: bound, nothing scheduled
    scan_delay_s = [ms / 1000.0 for ms in (a.scan_delay_ms or [0.0])]
    if scan:  # bound with neutral values: the plain run then launches the SENSOR instance of the step kernel
        cfg.domain_rand.scan_model, cfg.domain_rand.max_scan_delay_s = True, max(scan_delay_s)
    args = get_args([f"--task={a.task}", "--headless", f"--num_envs={a.num_envs}", "--seed=1",
                     f"--sim_device={a.device}", f"--rl_device={a.device}"])
    env, _ = task_registry.make_env(a.task, args, env_cfg=cfg)
    runner, _ = task_registry.make_alg_runner(env, args=args, train_cfg=tcfg, log_root=None)
    ev = PolicyEvaluator(env, runner)
    if a.profile:
        r = ev.run(a.steps or 200, graph=False, trace_depth=a.trace_depth, gait=a.gait, joints=a.joints,
                   contacts=a.contacts)
        if a.trace_depth:
            ev.traces("falls", 16)
        if a.cmd_vx:  # (the only run with eval_cmd_reduce_kernel)
            ev.run_command_test(a.cmd_vx, vy=a.cmd_vy, yaw=a.cmd_yaw, num_steps=a.steps or 200, graph=False)
        print(json.dumps({"profiled_steps": r["num_steps"], "total": r["total"]}))
        return
    rates = {"graph": [], "eager": []}
    runs = {"": ev.run}  # mode prefix -> the run it times, called with (steps, graph)

    def add(prefix, run):
        runs[prefix] = run
        rates.update({prefix + "_graph": [], prefix + "_eager": []})

    if a.push_vel:
        add("push", lambda steps, graph: ev.run_push_test(a.push_vel, directions=a.push_dirs, num_steps=steps, graph=graph))
    if a.cmd_vx:
        add("cmd", lambda steps, graph: ev.run_command_test(a.cmd_vx, vy=a.cmd_vy, yaw=a.cmd_yaw, num_steps=steps,
                                                            graph=graph))
    if a.force_n:
        add("force", lambda steps, graph: ev.run_force_test(a.force_n, directions=a.force_dirs, num_steps=steps, graph=graph))
    if scan:
        add("scan", lambda steps, graph: ev.run_scan_test(a.scan_noise_m or (0.0,), a.scan_dropout or (0.0,),
                                                          a.scan_offset_m or (0.0,), scan_delay_s, num_steps=steps, graph=graph))
    records = [flag for flag in ("gait", "joints", "contacts") if getattr(a, flag)]  # flag = mode prefix = report key
    for flag in records:
        add(flag, lambda steps, graph, flag=flag: ev.run(steps, graph, **{flag: True}))
    if a.trace_depth:  # (the last mode: traces() below reads the last timed run's rings)
        add("trace", lambda steps, graph: ev.run(steps, graph, trace_depth=a.trace_depth))
    for run in runs.values():  # warm both paths (the capture included)
        run(20, True)
        run(20, False)
    last = {}  # mode prefix -> its last report
    for _ in range(a.repeats):
        for mode in rates:
            prefix, _, how = mode.rpartition("_")
            r = last[prefix] = runs[prefix](a.steps, how == "graph")
            assert a.device == "cpu" or r["graph"] == (how == "graph")
            rates[mode].append(r["env_steps_per_s"])
    trace_doc = None
    if a.trace_depth:  # (the last timed run was the traced eager one)
        import time
        t0 = time.perf_counter()
        tr = ev.traces("falls", 16)  # ends in host copies: synchronises
        n, k = a.num_envs, a.trace_depth
        trace_doc = {"depth": k, "ring_bytes": n * k * 304, "traces_s": time.perf_counter() - t0,
                     "envs": int(tr["env_id"].shape[0]), "lengths": tr["length"].tolist(),
                     # what lgx_trace_record moves per step when every env records: the source rows
                     # (int64 length, 7 + 3 + 3 + 3 + 4 + 24 + 12 + 12 + 1 floats, all contact forces,
                     # count / status / reset flags) in, one 304-byte row and the count out
                     "record_bytes_in_per_step": n * (8 + 69 * 4 + env.num_bodies * 12 + 4 + 1 + 1),
                     "record_bytes_out_per_step": n * (304 + 4)}
    pr, cr, fr, sr = last.get("push"), last.get("cmd"), last.get("force"), last.get("scan")
    r = ev.run(a.steps) if len(runs) > 1 else r
    doc = {"task": a.task, "num_envs": a.num_envs, "num_steps": r["num_steps"], "fused_act": ev._fused is not None,
           "env_steps_per_s": {m: {"median": sorted(v)[len(v) // 2], "runs": [round(x) for x in v]}
                               for m, v in rates.items()},
           "total": r["total"]}
    if trace_doc:
        doc["flight_recorder"] = trace_doc
    n, nb = a.num_envs, env.num_bodies
    # What lgx_<kind>_record moves per step when every env records, (bytes in, bytes out): the two
    # records in and out (contacts: the env row's first float4) and, in, the sources and the status
    # and reset flags. gait: per foot its force and three floats of its rigid-body row; joints: per
    # joint its torque, dof_state pair and action; contacts: per body its force and position (the
    # terrain samples, 3 int16 per body and 9 more at an onset, come on top on a heightfield).
    record_bytes = {"gait": (n * (256 + 48 + 4 * 24 + 2), n * (256 + 48)),
                    "joints": (n * (768 + 16 + 12 * 16 + 2), n * (768 + 16)),
                    "contacts": (n * (nb * 48 + 16 + nb * 24 + 2), n * (nb * 48 + 16))}
    for flag in records:
        doc[flag] = {"total": last[flag]["total"][flag], "record_bytes_in_per_step": record_bytes[flag][0],
                     "record_bytes_out_per_step": record_bytes[flag][1]}
    if pr:
        doc["push_test"] = {k: pr[k] for k in ("speeds", "directions_deg", "push_step", "settle_tol", "total")}
        doc["push_test"]["per_speed"] = [
            {"speed": v, "episodes": sum(c["episodes"] for c in row), "survivors": sum(c["survivors"] for c in row),
             "pushed": sum(c["pushed"] for c in row)} for v, row in zip(pr["speeds"], pr["bins"])]
    if cr:
        doc["command_test"] = {k: cr[k] for k in ("vx", "vy", "yaw", "start", "switch_step", "steady_after", "settle_tol",
                                                  "yaw_tol", "total")}
        doc["command_test"]["per_vx"] = [
            {"vx": v, "episodes": sum(c["episodes"] for r_ in row for c in r_),
             "survivors": sum(c["survivors"] for r_ in row for c in r_),
             "switched": sum(c["switched"] for r_ in row for c in r_),
             "gain": [[c["gain"] for c in r_] for r_ in row]} for v, row in zip(cr["vx"], cr["bins"])]
    if fr:
        doc["force_test"] = {k: fr[k] for k in ("forces_n", "directions_deg", "onset_step", "force_steps", "point", "command",
                                                "steady_after", "settle_tol", "yaw_tol", "total")}
        doc["force_test"]["per_force"] = [
            {"force_n": v, "episodes": sum(c["episodes"] for c in row), "survivors": sum(c["survivors"] for c in row),
             "forced": sum(c["forced"] for c in row),
             "compliance_m_per_s_per_n": [c["compliance_m_per_s_per_n"] for c in row]} for v, row in zip(fr["forces_n"], fr["bins"])]
    if sr:
        doc["scan_test"] = {k: sr[k] for k in ("noise_m", "dropout", "dropout_value", "offset_x_m", "delay_s", "delay_steps", "total")}
        doc["scan_test"]["survival_rate"] = [[[[c["survival_rate"] for c in r_] for r_ in p_] for p_ in n_] for n_ in sr["bins"]]
        doc["scan_test"]["episodes"] = [[[[c["episodes"] for c in r_] for r_ in p_] for p_ in n_] for n_ in sr["bins"]]
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
