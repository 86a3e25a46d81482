"""The command schedule and the command-response evaluation (include/lgx.h, ABI 10) on liblgx.so's
host backend: the bodies of tests/command_case.py on "cpu", the refusals, and the evaluate.py
--cmd_vx entry point on a checkpoint of a one-iteration CPU train."""
import json
import os
import subprocess
import sys

import pytest

import command_case as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("task,n", [("go2", 64), ("go2", 63), ("go2_parkour", 64)])
def test_host_schedule_equals_user_command(task, n):
    K.equals_user_command(task, n, "cpu")


@pytest.mark.parametrize("n", [64, 63])
def test_host_unscheduled_rows_and_unused_buffers_change_nothing(n):
    K.mixed_rows(n, "cpu")


def test_host_switch_timing_and_heading_bypass():
    K.switch_timing(63, "cpu")


def test_host_curriculum_redraw_keeps_the_schedule():
    K.curriculum_redraw(63, "cpu")


@pytest.mark.parametrize("n", [1, 63, 130])
def test_host_records_and_cells_match_the_restatement(n):
    K.records_and_cells(n, "cpu")


def test_host_command_test_end_to_end():
    K.end_to_end("cpu")


def test_host_refusals():
    K.refusals("cpu")
    K.command_test_refusals("cpu")


def test_evaluate_cli_command_mode_on_cpu(tmp_path):
    """legged_gym/scripts/evaluate.py --cmd_vx against the checkpoint of a one-iteration CPU train."""
    env = dict(os.environ, PYTHONPATH=REPO, PYTHONDONTWRITEBYTECODE="1", LGX_LOG_ROOT=str(tmp_path), OMP_NUM_THREADS="4")
    common = ["--task=go2", "--sim_device=cpu", "--rl_device=cpu", "--num_envs=8", "--headless"]
    r = subprocess.run([sys.executable, os.path.join(REPO, "legged_gym", "scripts", "train.py"), "--max_iterations=1"]
                       + common, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    script = os.path.join(REPO, "legged_gym", "scripts", "evaluate.py")
    r = subprocess.run([sys.executable, script, "--eval_steps=8", "--cmd_vx=0,1.0", "--cmd_yaw=-0.5,0.5", "--cmd_at_s=0.04",
                        "--cmd_start=0.2,0,0"] + common, cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    from legged_gym_custom_amd.utils.evaluator import REPORT_KEYS
    doc = json.loads(r.stdout.strip().splitlines()[-1])
    assert doc["policy"] == "student" and doc["num_envs"] == 8 and doc["num_steps"] == 8 and doc["switch_step"] == 2
    assert doc["vx"] == [0.0, 1.0] and doc["vy"] == [0.0] and doc["yaw"] == [-0.5, 0.5] and doc["start"] == [0.2, 0.0, 0.0]
    assert doc["settle_tol"] == 0.3 and doc["yaw_tol"] == 0.3 and doc["steady_after"] == 50
    cells = [c for row in doc["bins"] for col in row for c in col]
    keys = set(REPORT_KEYS) | {"switched", "survivors", "mean_settle_s", "mean_yaw_settle_s", "mean_peak_tilt_rad",
                               "achieved", "gain"}
    assert len(doc["bins"]) == 2 and all(len(row) == 1 and len(row[0]) == 2 for row in doc["bins"])
    assert all(keys <= set(c) for c in cells)
    assert all(c["episodes"] + c["running"] == 2 for c in cells)  # 8 envs over 4 bins
    with open(os.path.join(os.path.dirname(doc["checkpoint"]), "eval_student_command.json")) as f:
        assert json.load(f)["bins"] == doc["bins"]
    r = subprocess.run([sys.executable, script, "--cmd_vx=1.0", "--push_vel=1.0"] + common, cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "mode of its own" in r.stderr
