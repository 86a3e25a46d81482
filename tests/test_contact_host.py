"""The contact record (include/lgx.h, ABI 14) on liblgx.so's host backend: the bodies of
tests/contact_case.py on "cpu", contact_cell_report / contact_total_row on hand-made rows, and the
evaluate.py --contacts entry point on a checkpoint of a one-iteration CPU train."""
import json
import os
import subprocess
import sys

import pytest

import contact_case as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("task,n", [("go2", 1), ("go2", 63), ("go2", 130), ("go2_parkour", 1), ("go2_parkour", 63),
                                    ("go2_parkour", 130)])
def test_host_records_and_cells_match_the_restatement(task, n):
    K.records_and_cells(task, n, "cpu")


@pytest.mark.parametrize("n", [1, 63, 130])
def test_host_frozen_means_frozen(n):
    K.frozen_means_frozen(n, "cpu")


@pytest.mark.parametrize("n", [1, 63, 130])
def test_host_reduce_is_deterministic(n):
    K.reduce_is_deterministic(n, "cpu")


@pytest.mark.parametrize("task,n", [("go2", 64), ("go2", 63), ("go2_parkour", 64)])
def test_host_end_to_end_on_real_physics(task, n):
    K.end_to_end(task, n, "cpu")


def test_host_terminal_forces_are_the_steps():
    K.terminal_forces("cpu")


def test_host_composition():
    K.composition("cpu")


def test_contact_cell_report():
    K.report()


def test_host_total_row_matches_the_concatenated_envs():
    K.total_matches_concatenation("cpu")


def test_host_refusals():
    K.refusals("cpu")


def test_evaluate_cli_contacts_on_cpu(tmp_path):
    """legged_gym/scripts/evaluate.py --contacts (with --gait and --joints) at 64 envs against the
    checkpoint of a one-iteration CPU train; a second run without the flag reports the same totals
    and cells."""
    env = dict(os.environ, PYTHONPATH=REPO, PYTHONDONTWRITEBYTECODE="1", LGX_LOG_ROOT=str(tmp_path), OMP_NUM_THREADS="4")
    common = ["--task=go2", "--sim_device=cpu", "--rl_device=cpu", "--num_envs=64", "--headless"]
    r = subprocess.run([sys.executable, os.path.join(REPO, "legged_gym", "scripts", "train.py"), "--max_iterations=1"]
                       + common, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    script = os.path.join(REPO, "legged_gym", "scripts", "evaluate.py")
    r = subprocess.run([sys.executable, script, "--eval_steps=12", "--contacts", "--gait", "--joints"] + common,
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    doc = json.loads(r.stdout.strip().splitlines()[-1])
    assert doc["num_steps"] == 12 and doc["num_envs"] == 64
    c = doc["total"]["contacts"]
    assert len(c["bodies"]) == 19 and {"base", "FL_foot", "RR_calf"} <= set(c["bodies"])
    assert c["envs"] == doc["total"]["episodes"] and "gait" in doc["total"] and "joints" in doc["total"]
    assert all("contacts" in x for row in doc["cells"] for x in row)
    assert sum(x["contacts"]["envs"] for row in doc["cells"] for x in row) == c["envs"]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("contacts ")]  # the human-readable summary
    assert lines and lines[-1].startswith("contacts total: falls ") and "foot touchdowns on an edge" in lines[-1]
    with open(os.path.join(os.path.dirname(doc["checkpoint"]), "eval_student.json")) as f:
        assert json.load(f)["total"]["contacts"] == c
    r = subprocess.run([sys.executable, script, "--eval_steps=12", "--gait", "--joints"] + common, cwd=str(tmp_path),
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    plain = json.loads(r.stdout.strip().splitlines()[-1])
    strip = lambda t: {k: v for k, v in t.items() if k != "contacts"}  # noqa: E731
    assert "contacts" not in plain["total"] and plain["total"] == strip(doc["total"])
    assert plain["cells"] == [[strip(x) for x in row] for row in doc["cells"]]
    assert not any(ln.startswith("contacts ") for ln in r.stdout.splitlines())
