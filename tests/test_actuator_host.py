"""Actuation latency and motor strength (include/lgx.h, ABI 8) on liblgx.so's host backend: the
bodies of tests/test_gpu_actuator.py (tests/actuator_case.py) with device="cpu", the refusals, the
setup draws, and the evaluator's options on the eager CPU loop."""
import json
import os
import subprocess
import sys

import pytest
import torch

import actuator_case as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.mark.parametrize("task,n,steps", [("go2", 64, 12), ("go2", 63, 12), ("go2_parkour", 64, 12),
                                          ("anymal_c_rough", 64, 8)])
def test_host_whole_step_latency_is_a_shifted_action(task, n, steps, tmp_path):
    A.whole_step_shift(task, n, "cpu", steps, tmp_path)


@pytest.mark.parametrize("task,steps", [("go2", 12), ("anymal_c_rough", 8)])
def test_host_substep_latency_matches_a_split_step(task, steps, tmp_path):
    A.substep_delays(task, 64, "cpu", steps, tmp_path)


def test_host_motor_strength_scales_the_gains():
    A.motor_strength_go2("cpu")


def test_host_motor_strength_scales_the_actuator_net(tmp_path):
    A.motor_strength_anymal("cpu", tmp_path)


@pytest.mark.parametrize("n", [64, 63])
def test_host_backend_feature_on_history_follows_last_actions(n):
    A.backend_vs_host(n, "cpu")


def test_host_zero_delay_and_unit_strength_change_nothing():
    A.identity("cpu")


def test_setup_draws_leave_existing_draws_alone_and_slice_by_rank(monkeypatch):
    A.setup_draws("cpu", monkeypatch)


def test_refusals_fail_cleanly():
    A.refusals("cpu")


def test_host_training_with_both_features_on():
    A.training_smoke("cpu", num_steps_per_env=8)


def evaluator_options(device):
    """tests/test_gpu_eval.py's setup (66 envs, a 10-step episode) with the latency options."""
    import eval_case as E
    from legged_gym_custom_amd.utils.evaluator import REPORT_KEYS, PolicyEvaluator

    def make(**over):
        env, tcfg, args = E.make_env("go2", 66, device, **{"env.episode_length_s": 0.19, **over})
        return PolicyEvaluator(env, E.make_runner(env, tcfg, args))

    cap = {"domain_rand.max_action_delay_s": 0.02}
    a, b, plain = make(**cap), make(**cap), make()
    assert a.env.action_history.shape[1] == 1 and plain.env.action_history is None
    a.env.set_motor_strength(1.0)  # the buffer exists before the loop is captured (strength 1 changes nothing)
    own = (torch.arange(66) % 5).to(torch.int32)  # the env's own per-env latencies: a run's constant must not outlive it
    a.env.action_delay_substeps.copy_(own)
    ra = a.run(action_delay_s=0.015)
    assert torch.equal(a.env.action_delay_substeps.cpu(), own)
    a.env.action_delay_substeps.zero_()
    assert ra["action_delay_substeps"] == [3, 3] and ra["motor_strength"] == [1.0, 1.0] and ra["total"]["running"] == 0
    assert ra["graph"] is (device != "cpu")
    delayed = a.last_cells.clone()
    b.run(graph=False, action_delay_s=0.015)
    assert torch.equal(delayed, b.last_cells)  # graph replay == the eager loop
    rp = plain.run()
    assert rp["action_delay_substeps"] is None and set(REPORT_KEYS) == set(rp["total"])
    a.run(action_delay_s=0)
    assert torch.equal(a.last_cells, plain.last_cells)
    assert not torch.equal(delayed, plain.last_cells)  # the latency changes the episode
    graph = a._graph
    sweep = a.sweep_action_delay([0, 0.01, 0.02])
    assert a._graph is graph  # captured once
    assert [r["action_delay_substeps"] for r in sweep] == [[0, 0], [2, 2], [4, 4]]
    for k in REPORT_KEYS:
        assert sweep[0]["total"][k] == rp["total"][k], k
    rs = a.run(action_delay_s=0, motor_strength=0.8)
    assert rs["motor_strength"] == [pytest.approx(0.8)] * 2
    assert float(a.env.motor_strengths.min()) == 1.0 == float(a.env.motor_strengths.max())  # restored after the run
    assert int(a.env.action_delay_substeps.abs().sum()) == 0
    if device != "cpu":  # allocating the buffer now would re-bind under the captured loop: refused
        with pytest.raises(RuntimeError, match="captured"):
            plain.env.set_motor_strength(0.9)
    with pytest.raises(ValueError):
        a.run(action_delay_s=0.03)  # beyond the capacity the env was built with
    with pytest.raises(ValueError):
        plain.run(action_delay_s=0.01)


def evaluate_cli_document(device, tmp_path):
    """legged_gym/scripts/evaluate.py (a child process: it edits the registry's configs) on a checkpoint of
    randomly initialised networks: the latency sweep document with a motor strength."""
    import eval_case as E
    from legged_gym_custom_amd.envs import task_registry
    env, tcfg, args = E.make_env("go2", 8, "cpu")
    runner, tcfg = task_registry.make_alg_runner(env, name="go2", args=args, train_cfg=tcfg,
                                                 log_root=os.path.join(str(tmp_path), tcfg.runner.experiment_name))
    os.makedirs(runner.log_dir, exist_ok=True)
    runner.save(os.path.join(runner.log_dir, "model_0.pt"))
    penv = dict(os.environ, PYTHONPATH=REPO, PYTHONDONTWRITEBYTECODE="1", LGX_LOG_ROOT=str(tmp_path), OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, os.path.join(REPO, "legged_gym", "scripts", "evaluate.py"), "--eval_steps=3",
                        "--action_delay_ms", "0,10,25", "--motor_strength", "0.9", "--task=go2", f"--sim_device={device}",
                        f"--rl_device={device}", "--num_envs=8", "--headless"],
                       cwd=str(tmp_path), env=penv, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    doc = json.loads(r.stdout.strip().splitlines()[-1])
    assert doc["task"] == "go2" and doc["policy"] == "student" and doc["action_delay_ms"] == [0.0, 10.0, 25.0]
    assert [x["action_delay_substeps"] for x in doc["sweep"]] == [[0, 0], [2, 2], [5, 5]]
    assert all(x["motor_strength"] == [pytest.approx(0.9)] * 2 and x["num_steps"] == 3 for x in doc["sweep"])
    out = os.path.join(os.path.dirname(doc["checkpoint"]), "eval_student_latency.json")
    assert os.path.dirname(doc["checkpoint"]).startswith(str(tmp_path))
    with open(out) as f:
        assert json.load(f)["sweep"][2]["total"] == doc["sweep"][2]["total"]


def test_host_evaluator_latency_options():
    evaluator_options("cpu")


def test_host_evaluate_cli_document(tmp_path):
    evaluate_cli_document("cpu", tmp_path)
