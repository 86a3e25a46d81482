"""bench.py as a command: a plain run prints the headline line only (what --full adds is absent),
--dump-outputs writes the last timed iteration's arrays as float32 .npy files, and two runs with
the same arguments dump the same arrays, bit for bit (the inputs are seeded, and two builds can
only be compared output for output if one build agrees with itself)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("value_no_episode_tracking", "window_spread", "env_kernel", "roofline", "roofline_valu",
             "roofline_learner", "cpu_baseline")
NUM_ENVS = 256


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The same plain command twice (side by side): [(result line, dump folder)] * 2."""
    env = dict(os.environ)
    for k in ("LGX_LIB", "LGX_MLP_LIB", "LGX_S8_LIB"):
        env.pop(k, None)
    base = tmp_path_factory.mktemp("bench_cli")
    procs = []
    for r in "ab":
        out = str(base / f"dump_{r}")
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
               "--num_envs", str(NUM_ENVS), "--dump-outputs", out]
        procs.append((out, subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                            text=True)))
    res = []
    for out, p in procs:
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, so[-3000:] + se[-3000:]
        lines = [l for l in so.splitlines() if l.startswith("{")]
        assert len(lines) == 1, so[-3000:]
        res.append((json.loads(lines[0]), out))
    return res


def test_plain_run_line_and_dumped_outputs(runs):
    d, out = runs[0]
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1 and len(d["windows"]) == 1
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0
    # value is the env steps of the 2 timed iterations over their wall time
    assert d["value"] == pytest.approx(NUM_ENVS * 24 / (d["ms_per_step"] * 1e-3), rel=1e-3)
    assert not set(FULL_ONLY) & set(d)
    files = sorted(glob.glob(os.path.join(out, "*.npy")))
    names = {os.path.basename(f)[:-4] for f in files}
    assert {"obs", "root_states", "rollout_actions", "rollout_returns", "actor_critic_params"} <= names
    total = 0
    for f in files:
        a = np.load(f)
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(os.path.join(out, "rollout_actions.npy")).shape == (24, NUM_ENVS, 12)


def test_two_runs_dump_identical_outputs(runs):
    (_, a), (_, b) = runs
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(a, "*.npy")))
    assert names and names == sorted(os.path.basename(f) for f in glob.glob(os.path.join(b, "*.npy")))
    for n in names:
        assert np.array_equal(np.load(os.path.join(a, n)), np.load(os.path.join(b, n))), n
