"""Scheduled pushes and the push-recovery evaluation (include/lgx.h, ABI 9) on liblgx.so's host
backend: the bodies of tests/push_case.py on "cpu", the refusals, and the evaluate.py --push_vel
entry point on a checkpoint of a one-iteration CPU train."""
import json
import os
import subprocess
import sys

import pytest

import push_case as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [64, 63])
def test_host_scheduled_push_is_a_velocity_edit(n):
    P.velocity_edit(n, "cpu")


def test_host_unscheduled_buffers_change_nothing():
    P.identity("cpu")


@pytest.mark.parametrize("n", [1, 63, 130])
def test_host_records_and_cells_match_the_restatement(n):
    P.records_and_cells(n, "cpu")


def test_host_push_test_end_to_end():
    P.end_to_end("cpu")


def test_host_refusals():
    P.refusals("cpu")
    P.push_test_refusals("cpu")


def test_evaluate_cli_push_mode_on_cpu(tmp_path):
    """legged_gym/scripts/evaluate.py --push_vel against the checkpoint of a one-iteration CPU train."""
    env = dict(os.environ, PYTHONPATH=REPO, PYTHONDONTWRITEBYTECODE="1", LGX_LOG_ROOT=str(tmp_path), OMP_NUM_THREADS="4")
    common = ["--task=go2", "--sim_device=cpu", "--rl_device=cpu", "--num_envs=8", "--headless"]
    r = subprocess.run([sys.executable, os.path.join(REPO, "legged_gym", "scripts", "train.py"), "--max_iterations=1"]
                       + common, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    r = subprocess.run([sys.executable, os.path.join(REPO, "legged_gym", "scripts", "evaluate.py"), "--eval_steps=6",
                        "--push_vel=0,1.0", "--push_dirs=2", "--push_at_s=0.04"] + common,
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    from legged_gym_custom_amd.utils.evaluator import REPORT_KEYS
    doc = json.loads(r.stdout.strip().splitlines()[-1])
    assert doc["policy"] == "student" and doc["num_envs"] == 8 and doc["num_steps"] == 6 and doc["push_step"] == 2
    assert doc["speeds"] == [0.0, 1.0] and doc["directions_deg"] == [0.0, 180.0] and doc["settle_tol"] == 0.3
    assert len(doc["bins"]) == 2 and all(len(row) == 2 for row in doc["bins"])
    keys = set(REPORT_KEYS) | {"pushed", "mean_peak_tilt_rad", "mean_peak_lin_vel_err", "survivors", "mean_settle_s"}
    assert keys <= set(doc["total"]) and all(keys <= set(c) for row in doc["bins"] for c in row)
    assert sum(c["episodes"] + c["running"] for row in doc["bins"] for c in row) == 8
    assert all(c["episodes"] + c["running"] == 2 for row in doc["bins"] for c in row)  # 8 envs over 4 bins
    with open(os.path.join(os.path.dirname(doc["checkpoint"]), "eval_student_push.json")) as f:
        assert json.load(f)["bins"] == doc["bins"]
