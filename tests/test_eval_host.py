"""lgx_eval_begin / lgx_eval_accumulate / lgx_eval_reduce (include/lgx.h, ABI 7) on liblgx.so's
host backend, through LeggedRobot.eval_begin / eval_accumulate / eval_cells: scripted inputs
(tests/eval_case.py) against a float64 torch restatement, the clean error paths, and the
evaluate.py entry point on a checkpoint of a one-iteration CPU train."""
import json
import os
import subprocess
import sys

import pytest
import torch

import eval_case as E
from legged_gym_custom_amd import _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scripted_env(n, device="cpu"):
    gen = torch.Generator().manual_seed(100 + n)
    env, _, _ = E.make_env("go2", n, device)
    E.bind_grid(env, gen)
    return env, gen


@pytest.mark.parametrize("n", [1, 63, 130])
def test_host_records_and_cells_match_the_restatement(n):
    env, gen = _scripted_env(n)
    ref = E.run_script(env, gen)
    if n >= 63:
        assert set(ref.status.tolist()) == {0, 1, 2, 3}
        assert ref.status[:4].tolist() == [1, 2, 3, 1] and ref.acc[0, 0] == 0 and ref.acc[1, 0] == 2
    E.check_records(env.eval_acc, env.eval_status, ref, f"host n={n}")
    cells = env.eval_cells()
    assert cells.shape == (E.ROWS, E.COLS, 12) and cells.dtype == torch.float64
    E.check_cells(cells, env.eval_acc, env.eval_status, env.terrain_levels, env.terrain_types)
    assert torch.equal(env.eval_cells(), cells)  # deterministic: bit-identical on a second call


def test_host_without_a_terrain_grid_is_one_cell():
    env, _, _ = E.make_env("go2", 8, "cpu")
    ref = E.run_script(env, torch.Generator().manual_seed(5))
    E.check_records(env.eval_acc, env.eval_status, ref, "host 1x1")
    cells = env.eval_cells()
    assert cells.shape == (1, 1, 12)
    E.check_cells(cells, env.eval_acc, env.eval_status, None, None)


def eval_error_paths(device):
    """Each failure raises LgxError and writes nothing."""
    env, gen = _scripted_env(63, device)
    E.run_script(env, gen)
    env._eval_cells.fill_(-7.0)
    snap = lambda: [t.clone() for t in (env.eval_acc, env.eval_status, env._eval_cells)]  # noqa: E731
    before = snap()
    same = lambda: all(torch.equal(a, b) for a, b in zip(before, snap()))  # noqa: E731
    env.reset_buf.zero_()  # an accumulate that went ahead would add a sample to every running env
    # a required buffer that is not bound
    keep = env.base_lin_vel
    env.base_lin_vel = None
    env._bind()
    for call in (env.eval_begin, env.eval_accumulate, env.eval_cells):
        with pytest.raises(_native.LgxError, match="base_lin_vel"):
            call()
    env.base_lin_vel = keep
    env._bind()
    assert same()
    # an empty cell grid, and NULL eval buffers
    ev = env._native.eval_buffers(env.eval_acc, env.eval_status, env._eval_cells, env._eval_overflow)
    ev.cell_rows = 0
    for call in (env._native.eval_begin, env._native.eval_accumulate, env._native.eval_reduce):
        with pytest.raises(_native.LgxError, match="cell_rows"):
            call(ev, env._stream())
    L = _native.lib()
    assert L.lgx_eval_accumulate(env._native.handle, None, None) < 0
    assert b"NULL" in L.lgx_last_error(env._native.handle)
    assert same()
    # a level outside the grid: counted, never used as an index
    env.terrain_levels[5] = E.ROWS
    env.terrain_types[7] = -1
    with pytest.raises(_native.LgxError, match="2 envs"):
        env.eval_cells()
    assert same()
    env.terrain_levels[5] = 0
    env.terrain_types[7] = 0
    cells = env.eval_cells()  # and the evaluation is usable again
    E.check_cells(cells, env.eval_acc, env.eval_status, env.terrain_levels, env.terrain_types)


def test_host_error_paths_fail_cleanly():
    eval_error_paths("cpu")


def test_report_of_empty_cells_is_none_not_nan():
    from legged_gym_custom_amd.utils.evaluator import REPORT_KEYS, cell_report
    r = cell_report(torch.zeros(12, dtype=torch.float64), 0.02, 150.0)
    assert set(r) == set(REPORT_KEYS)
    assert r["episodes"] == 0 and r["running"] == 0 and r["blowups"] == 0
    assert all(r[k] is None for k in REPORT_KEYS if k not in ("episodes", "running", "blowups"))
    cell = torch.tensor([4, 2, 1, 1, 100, 4.0, 1.0, 3.0, 5.0, 60.0, 9.0, 400.0], dtype=torch.float64)
    r = cell_report(cell, 0.02, 150.0)
    assert r["episodes"] == 4 and r["survival_rate"] == 0.5 and r["fall_rate"] == 0.25 and r["blowups"] == 1
    assert r["mean_episode_s"] == pytest.approx(0.5) and r["rms_lin_vel_err"] == pytest.approx(0.2)
    assert r["mean_forward_speed"] == pytest.approx(1.5) and r["cost_of_transport"] == pytest.approx(0.08)
    assert r["mean_peak_foot_force"] == pytest.approx(100.0)


def test_evaluate_cli_on_cpu(tmp_path):
    """legged_gym/scripts/evaluate.py against the checkpoint of a one-iteration CPU train."""
    env = dict(os.environ, PYTHONPATH=REPO, PYTHONDONTWRITEBYTECODE="1", LGX_LOG_ROOT=str(tmp_path), OMP_NUM_THREADS="4")
    common = ["--task=go2", "--sim_device=cpu", "--rl_device=cpu", "--num_envs=8", "--headless"]
    r = subprocess.run([sys.executable, os.path.join(REPO, "legged_gym", "scripts", "train.py"), "--max_iterations=1"]
                       + common, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    r = subprocess.run([sys.executable, os.path.join(REPO, "legged_gym", "scripts", "evaluate.py"), "--eval_steps=3"]
                       + common, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    from legged_gym_custom_amd.utils.evaluator import REPORT_KEYS
    doc = json.loads(r.stdout.strip().splitlines()[-1])
    assert doc["policy"] == "student" and doc["num_envs"] == 8 and doc["num_steps"] == 3
    assert set(REPORT_KEYS) <= set(doc["total"]) and set(REPORT_KEYS) <= set(doc["cells"][0][0])
    assert doc["total"]["episodes"] + doc["total"]["running"] == 8
    assert os.path.dirname(doc["checkpoint"]).startswith(str(tmp_path))
    with open(os.path.join(os.path.dirname(doc["checkpoint"]), "eval_student.json")) as f:
        assert json.load(f)["total"] == doc["total"]
