"""The flight recorder (include/lgx.h, ABI 11) on liblgx.so's host backend: the bodies of
tests/trace_case.py on "cpu", and the evaluate.py --trace_falls entry point on a checkpoint of a
one-iteration CPU train."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import trace_case as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [1, 63, 130])
def test_host_ring_and_gather_match_the_restatement(n):
    T.ring_matches_restatement(n, "cpu")


@pytest.mark.parametrize("n", [1, 63])
def test_host_frozen_means_frozen(n):
    T.frozen_means_frozen(n, "cpu")


def test_host_peak_body_ties_and_zero_forces():
    T.peak_ties("cpu")


def test_host_end_to_end_on_real_physics():
    T.end_to_end("go2", 8, "cpu")


def test_host_selection_of_falls():
    T.selection("cpu")


def test_host_refusals():
    T.refusals("cpu")


def test_evaluate_cli_trace_falls_on_cpu(tmp_path):
    """legged_gym/scripts/evaluate.py --trace_falls against the checkpoint of a one-iteration CPU
    train; a second run without the flag reports the same totals."""
    env = dict(os.environ, PYTHONPATH=REPO, PYTHONDONTWRITEBYTECODE="1", LGX_LOG_ROOT=str(tmp_path), OMP_NUM_THREADS="4")
    common = ["--task=go2", "--sim_device=cpu", "--rl_device=cpu", "--num_envs=8", "--headless"]
    r = subprocess.run([sys.executable, os.path.join(REPO, "legged_gym", "scripts", "train.py"), "--max_iterations=1"]
                       + common, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    script = os.path.join(REPO, "legged_gym", "scripts", "evaluate.py")
    r = subprocess.run([sys.executable, script, "--eval_steps=12", "--trace_falls", "4", "--trace_s", "0.1"] + common,
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    doc = json.loads(r.stdout.strip().splitlines()[-1])
    run_dir = os.path.dirname(doc["checkpoint"])
    npz = os.path.join(run_dir, "eval_student_traces.npz")
    assert doc["num_steps"] == 12 and doc["traces"]["file"] == npz and doc["traces"]["depth"] == 5  # 0.1 s / 0.02 s
    assert os.path.exists(npz)
    with np.load(npz) as z:
        m = int(z["env_id"].shape[0])
        assert m == doc["traces"]["envs"] and 0 <= m <= 4
        assert z["trace"].shape == (m, 5, 76) and z["trace"].dtype == np.float32
        for k in ("length", "status", "terrain_level", "terrain_type"):
            assert z[k].shape == (m,)
        assert z["columns"].shape == (76,) and str(z["columns"][0]) == "episode_length" and float(z["dt"]) > 0
        assert set(z["status"].tolist()) <= {2, 3} and bool((z["length"] <= 5).all())
    with open(os.path.join(run_dir, "eval_student.json")) as f:
        assert json.load(f)["traces"] == doc["traces"]
    r = subprocess.run([sys.executable, script, "--eval_steps=12"] + common, cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    plain = json.loads(r.stdout.strip().splitlines()[-1])
    assert "traces" not in plain and plain["total"] == doc["total"] and plain["cells"] == doc["cells"]
