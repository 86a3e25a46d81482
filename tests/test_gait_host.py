"""The gait record (include/lgx.h, ABI 12) on liblgx.so's host backend: the bodies of
tests/gait_case.py on "cpu", gait_cell_report on hand-made rows, and the evaluate.py --gait entry
point on a checkpoint of a one-iteration CPU train."""
import json
import os
import subprocess
import sys

import pytest

import gait_case as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [1, 63, 130])
def test_host_records_and_cells_match_the_restatement(n):
    G.records_and_cells(n, "cpu")


@pytest.mark.parametrize("n", [1, 63, 130])
def test_host_frozen_means_frozen(n):
    G.frozen_means_frozen(n, "cpu")


@pytest.mark.parametrize("n", [1, 63, 130])
def test_host_reduce_is_deterministic(n):
    G.reduce_is_deterministic(n, "cpu")


def test_host_end_to_end_on_real_physics():
    G.end_to_end("go2", 8, "cpu")


def test_host_composition():
    G.composition("cpu")


def test_gait_cell_report():
    G.report()


def test_host_refusals():
    G.refusals("cpu")


def test_evaluate_cli_gait_on_cpu(tmp_path):
    """legged_gym/scripts/evaluate.py --gait against the checkpoint of a one-iteration CPU train; a
    second run without the flag reports the same totals and cells."""
    env = dict(os.environ, PYTHONPATH=REPO, PYTHONDONTWRITEBYTECODE="1", LGX_LOG_ROOT=str(tmp_path), OMP_NUM_THREADS="4")
    common = ["--task=go2", "--sim_device=cpu", "--rl_device=cpu", "--num_envs=8", "--headless"]
    r = subprocess.run([sys.executable, os.path.join(REPO, "legged_gym", "scripts", "train.py"), "--max_iterations=1"]
                       + common, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    script = os.path.join(REPO, "legged_gym", "scripts", "evaluate.py")
    r = subprocess.run([sys.executable, script, "--eval_steps=12", "--gait"] + common, cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    doc = json.loads(r.stdout.strip().splitlines()[-1])
    assert doc["num_steps"] == 12
    g = doc["total"]["gait"]
    assert set(g["feet"]) == {"FL_foot", "FR_foot", "RL_foot", "RR_foot"} and g["envs"] == doc["total"]["episodes"]
    assert all("gait" in c for row in doc["cells"] for c in row)
    assert any(line.startswith("gait ") for line in r.stdout.splitlines())  # the human-readable summary
    with open(os.path.join(os.path.dirname(doc["checkpoint"]), "eval_student.json")) as f:
        assert json.load(f)["total"]["gait"] == g
    r = subprocess.run([sys.executable, script, "--eval_steps=12"] + common, cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    plain = json.loads(r.stdout.strip().splitlines()[-1])
    strip = lambda t: {k: v for k, v in t.items() if k != "gait"}  # noqa: E731
    assert "gait" not in plain["total"] and plain["total"] == strip(doc["total"])
    assert plain["cells"] == [[strip(c) for c in row] for row in doc["cells"]]
