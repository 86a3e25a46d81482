"""The sustained external force (include/lgx.h, ABI 16) on liblgx.so's host backend: the bodies of
tests/test_gpu_force.py (tests/force_case.py) with device="cpu", the two scalar rules of
csrc/lgx_env_common.h in a stand-alone program, the API, the evaluator's force test on the eager CPU
loop and the evaluate.py --force_n document.

Measured on the host backend (64 and 63 envs): momentum law |P - (f + M g) dt| / (|f| dt), bound 2e-2:
Go2 7.1e-5 .. 6.6e-4 for the four fixed 30 N cases, worst 3.6e-3 over the random rows; ANYmal
4.3e-5 .. 1.8e-4. Line of action at 4 N: the point slid 0.2 m along the force 0.07 x the bound,
0.2 m to the side 22 x (at 30 N on a robot still landing: 3.6 x, with one substep per step 0.002 x)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import force_case as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("task,n,epw", F.INSTANCES)
def test_host_off_windows_and_zero_forces_change_nothing(task, n, epw, tmp_path):
    F.identity(task, n, "cpu", tmp_path, epw)


@pytest.mark.parametrize("n", [64, 63])
def test_host_unforced_neighbours_keep_their_bits(n):
    F.neighbours(n, "cpu")


@pytest.mark.parametrize("n", [64, 63])
def test_host_window_rule(n):
    F.window_rule(n, "cpu")


@pytest.mark.parametrize("oriented", [False, True])
@pytest.mark.parametrize("task,n,epw", F.INSTANCES)
def test_host_momentum_law(task, n, epw, oriented, tmp_path):
    F.momentum_law(task, n, "cpu", tmp_path, epw, oriented)


def test_host_line_of_action():
    F.line_of_action("cpu")


def test_force_refusals_fail_cleanly():
    F.refusals("cpu")
    F.force_test_refusals("cpu")


def test_host_allocating_call_is_refused_after_a_capture():
    F.captured_refusal("cpu")


def test_force_setup_draws_leave_existing_draws_alone_and_slice_by_rank(monkeypatch):
    F.setup_draws("cpu", monkeypatch)


def test_host_force_test_end_to_end():
    F.end_to_end("cpu")


def test_host_evaluate_cli_force_document(tmp_path):
    F.evaluate_cli_document("cpu", tmp_path)


def test_host_training_with_the_force_randomisation_on():
    F.training_smoke("cpu", num_steps_per_env=8)


# ------------------------------------------------------------------ the shared scalar rules, stand-alone
GRID = (-1, 0, 1, 2, 3, 5, 1000, 2 ** 31 - 1)
PITCH = 0.3
QUATS = {"yaw 0": (0.0, PITCH), "yaw 90": (90.0, PITCH), "yaw 200": (200.0, PITCH), "straight up": (0.0, 90.0)}

PROGRAM = r"""
#include "include/lgx.h"
#include "legged_gym_custom_amd/csrc/lgx_env_common.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static unsigned bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }

int main(int argc, char** argv) {
  const int grid[] = {-1, 0, 1, 2, 3, 5, 1000, 2147483647};
  for (int start : grid)
    for (int steps : grid)
      for (int period : grid) {
        for (int ep : grid) putchar(lgx::force_window_on(start, steps, period, ep) ? '1' : '0');
        putchar('\n');
      }
  // frame: argv = groups of 7 float bit patterns (quaternion x y z w, force forward left up)
  for (int i = 1; i + 6 < argc; i += 7) {
    float in[7], out[3];
    for (int j = 0; j < 7; ++j) {
      const unsigned u = (unsigned)strtoul(argv[i + j], nullptr, 16);
      memcpy(&in[j], &u, 4);
    }
    lgx::force_to_world(in, in + 4, out);
    printf("frame %08x %08x %08x\n", bits(out[0]), bits(out[1]), bits(out[2]));
  }
  return 0;
}
"""


def bits(x):
    return struct.unpack("I", struct.pack("f", float(x)))[0]


def unbits(u):
    return struct.unpack("f", struct.pack("I", u))[0]


def frame_f32(q, f):
    """The rule of include/lgx.h in numpy float32, operation by operation: quat_apply(q, (1, 0, 0)),
    the heading, the rotation of (forward, left); up passes through."""
    f32 = np.float32
    x, y, z, w = (f32(v) for v in q)
    # quat_apply(q, v) = v (2 w^2 - 1) + 2 w (q x v) + 2 q (q . v), v = (1, 0, 0)
    a = f32(f32(2.0) * f32(w * w)) - f32(1.0)
    fx = f32(f32(a + f32(f32(0.0) * f32(w * f32(2.0)))) + f32(f32(x * x) * f32(2.0)))
    fy = f32(f32(f32(0.0) * a + f32(f32(z) * f32(w * f32(2.0)))) + f32(f32(y * x) * f32(2.0)))
    n = np.sqrt(f32(fx * fx + fy * fy), dtype=f32)
    hx, hy = (f32(fx / n), f32(fy / n)) if n > f32(1e-6) else (f32(1.0), f32(0.0))
    fw, fl, up = (f32(v) for v in f)
    return f32(f32(fw * hx) - f32(fl * hy)), f32(f32(fw * hy) + f32(fl * hx)), up


def test_window_predicate_and_frame_conversion_are_those_of_the_header(tmp_path):
    src, exe = tmp_path / "force_probe.cpp", tmp_path / "force_probe"
    src.write_text(PROGRAM)
    cmd = ["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", ROOT, "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    cases = []
    for yaw_deg, pitch in QUATS.values():
        psi, th = np.radians(yaw_deg), (np.pi / 2 if pitch == 90.0 else pitch)
        # Rz(psi) Ry(-th): the nose pitched up by th (straight up at 90 degrees)
        sz, cz, sy, cy = np.sin(psi / 2), np.cos(psi / 2), np.sin(-th / 2), np.cos(-th / 2)
        q = np.array([-sz * sy, cz * sy, cy * sz, cz * cy], dtype=np.float32)
        for f in ((30.0, 0.0, 0.0), (0.0, 30.0, 0.0), (-7.5, 12.25, 3.0)):
            cases.append((q, np.array(f, dtype=np.float32)))
    args = [f"{bits(v):08x}" for q, f in cases for v in list(q) + list(f)]
    # the program allocates nothing; leak detection needs ptrace, which a container may refuse
    run = subprocess.run([str(exe)] + args, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"),
                         timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr  # (UBSan: a start + steps would overflow here)
    lines = run.stdout.split("\n")
    want = ["".join("1" if F.window_on(start, steps, period, ep) else "0" for ep in GRID)
            for start in GRID for steps in GRID for period in GRID]
    got = [ln for ln in lines if ln and ln[0] in "01"]
    assert got == want
    assert sum(ln.count("1") for ln in want) > 500 and "00111111" in want  # both answers are common
    frames = [[unbits(int(v, 16)) for v in ln.split()[1:]] for ln in lines if ln.startswith("frame")]
    assert len(frames) == len(cases)
    for (q, f), out in zip(cases, frames):
        ref = frame_f32(q, f)
        ulp = [abs(float(a) - float(b)) / max(np.spacing(np.float32(np.abs(f[:2]).max())), 1e-45) for a, b in zip(out[:2], ref[:2])]
        # the same fp32 operations in the same order (quat_apply's own order is the header's affair): a few ulp of |f|
        assert max(ulp) <= 8.0 and out[2] == float(f[2]), (q, f, out, ref)
        # and it is the heading rotation in float64
        x, y, z, w = (float(v) for v in q)
        fx, fy = 1 - 2 * (y * y + z * z), 2 * (w * z + x * y)
        n = np.hypot(fx, fy)
        hx, hy = (fx / n, fy / n) if n > 1e-6 else (1.0, 0.0)
        exact = (f[0] * hx - f[1] * hy, f[0] * hy + f[1] * hx)
        assert max(abs(out[0] - exact[0]), abs(out[1] - exact[1])) <= 1e-5 * 30.0 / max(n, 1e-3), (q, f, out, exact, n)
