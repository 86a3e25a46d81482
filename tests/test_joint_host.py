"""The joint-load record (include/lgx.h, ABI 13) on liblgx.so's host backend: the bodies of
tests/joint_case.py on "cpu", joint_cell_report on hand-made rows, and the evaluate.py --joints entry
point on a checkpoint of a one-iteration CPU train."""
import json
import os
import subprocess
import sys

import pytest

import joint_case as J

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [1, 63, 130])
def test_host_records_and_cells_match_the_restatement(n):
    J.records_and_cells(n, "cpu")


@pytest.mark.parametrize("n", [1, 63, 130])
def test_host_frozen_means_frozen(n):
    J.frozen_means_frozen(n, "cpu")


@pytest.mark.parametrize("n", [1, 63, 130])
def test_host_reduce_is_deterministic(n):
    J.reduce_is_deterministic(n, "cpu")


@pytest.mark.parametrize("n", [64, 63])
def test_host_end_to_end_on_real_physics(n):
    J.end_to_end("go2", n, "cpu")


def test_host_composition():
    J.composition("cpu")


def test_joint_cell_report():
    J.report()


def test_host_refusals():
    J.refusals("cpu")


def test_evaluate_cli_joints_on_cpu(tmp_path):
    """legged_gym/scripts/evaluate.py --joints at 64 envs against the checkpoint of a one-iteration CPU
    train; a second run without the flag reports the same totals and cells."""
    env = dict(os.environ, PYTHONPATH=REPO, PYTHONDONTWRITEBYTECODE="1", LGX_LOG_ROOT=str(tmp_path), OMP_NUM_THREADS="4")
    common = ["--task=go2", "--sim_device=cpu", "--rl_device=cpu", "--num_envs=64", "--headless"]
    r = subprocess.run([sys.executable, os.path.join(REPO, "legged_gym", "scripts", "train.py"), "--max_iterations=1"]
                       + common, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    script = os.path.join(REPO, "legged_gym", "scripts", "evaluate.py")
    r = subprocess.run([sys.executable, script, "--eval_steps=12", "--joints"] + common, cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    doc = json.loads(r.stdout.strip().splitlines()[-1])
    assert doc["num_steps"] == 12 and doc["num_envs"] == 64
    j = doc["total"]["joints"]
    names = ["FL_hip_joint", "FL_thigh_joint", "FL_calf_joint", "FR_hip_joint", "FR_thigh_joint", "FR_calf_joint",
             "RL_hip_joint", "RL_thigh_joint", "RL_calf_joint", "RR_hip_joint", "RR_thigh_joint", "RR_calf_joint"]
    assert set(j["joints"]) == set(names) and j["envs"] == doc["total"]["episodes"] and isinstance(j["flags"], (list, type(None)))
    assert all("joints" in c for row in doc["cells"] for c in row)
    assert sum(c["joints"]["envs"] for row in doc["cells"] for c in row) == j["envs"]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("joint ")]  # the human-readable summary
    assert len(lines) == 12 and all(any(ln.startswith(f"joint total {nm}:") for ln in lines) for nm in names)
    with open(os.path.join(os.path.dirname(doc["checkpoint"]), "eval_student.json")) as f:
        assert json.load(f)["total"]["joints"] == j
    r = subprocess.run([sys.executable, script, "--eval_steps=12"] + common, cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    plain = json.loads(r.stdout.strip().splitlines()[-1])
    strip = lambda t: {k: v for k, v in t.items() if k != "joints"}  # noqa: E731
    assert "joints" not in plain["total"] and plain["total"] == strip(doc["total"])
    assert plain["cells"] == [[strip(c) for c in row] for row in doc["cells"]]
    assert not any(ln.startswith("joint ") for ln in r.stdout.splitlines())
