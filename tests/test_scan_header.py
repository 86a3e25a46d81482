"""The height-scan model's scalar rules of csrc/lgx_env_common.h (scan_raw, scan_point_model,
scan_point_lost, scan_uniform and the shared terrain lookup terrain_cell_height / scan_point_height /
contact_terrain_height; include/lgx.h ABI 17), stand-alone, as tests/test_sensor_header.py does: a
program that includes only include/lgx.h and that header, built with the host backend's flags plus
-Werror and ASan/UBSan, run as a child process. The point model is driven over its branches against
the rule of include/lgx.h restated here in np.float32; the shared lookup is compared on a small grid,
clamped borders included, with the arithmetic get_heights and contact_terrain_height had before they
shared it, restated in the program."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "include/lgx.h"
#include "legged_gym_custom_amd/csrc/lgx_env_common.h"

#include <initializer_list>
#include <stdio.h>
#include <string.h>

static unsigned bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }

// the step's height scan as it was written before the lookup was shared
static float old_scan_height(const lgx_task_params* Pm, const int16_t* hs, const float* root, float bx, float by) {
  float qz = root[5], qw = root[6];
  float n = sqrtf(qz * qz + qw * qw);
  n = n < 1e-9f ? 1e-9f : n;
  float qy[4] = {0.f, 0.f, qz / n, qw / n};
  float p[3] = {bx, by, 0.f}, w[3];
  lgx::quat_apply(qy, p, w);
  float px = (w[0] + root[0]) + Pm->border_size, py = (w[1] + root[1]) + Pm->border_size;
  long ix = (long)(px / Pm->horizontal_scale), iy = (long)(py / Pm->horizontal_scale);
  ix = ix < 0 ? 0 : (ix > Pm->hf_rows - 2 ? Pm->hf_rows - 2 : ix);
  iy = iy < 0 ? 0 : (iy > Pm->hf_cols - 2 ? Pm->hf_cols - 2 : iy);
  int16_t h1 = hs[ix * Pm->hf_cols + iy];
  int16_t h2 = hs[(ix + 1) * Pm->hf_cols + iy];
  int16_t h3 = hs[ix * Pm->hf_cols + iy + 1];
  int16_t h = h1 < h2 ? h1 : h2;
  h = h < h3 ? h : h3;
  return (float)h * Pm->vertical_scale;
}
// and the contact record's
static float old_contact_height(const lgx_task_params* Pm, const int16_t* hs, float x, float y, long& ix, long& iy) {
  ix = iy = 0;
  if (hs == nullptr) return 0.f;
  const float px = x + Pm->border_size, py = y + Pm->border_size;
  ix = (long)(px / Pm->horizontal_scale);
  iy = (long)(py / Pm->horizontal_scale);
  ix = ix < 0 ? 0 : (ix > Pm->hf_rows - 2 ? Pm->hf_rows - 2 : ix);
  iy = iy < 0 ? 0 : (iy > Pm->hf_cols - 2 ? Pm->hf_cols - 2 : iy);
  const int16_t h1 = hs[ix * Pm->hf_cols + iy];
  const int16_t h2 = hs[(ix + 1) * Pm->hf_cols + iy];
  const int16_t h3 = hs[ix * Pm->hf_cols + iy + 1];
  int16_t h = h1 < h2 ? h1 : h2;
  h = h < h3 ? h : h3;
  return (float)h * Pm->vertical_scale;
}

static lgx_task_params P;

int main() {
  // the point model over its branches: v, amp, u, dz, p, ud, fill
  const float V[] = {0.07f, -0.4f, 0.96f, -1.0f, 1.0f, -0.f};
  const float AMP[] = {0.f, 0.05f, 2.0f};
  const float U[] = {0.f, 0.3125f, 0.99999994f};
  const float DZ[] = {0.f, 0.03f, -1.5f};
  const float PR[] = {0.f, 0.3125f, 1.0f};
  const float UD[] = {0.f, 0.31249997f, 0.3125f, 0.99999994f};
  const float FILL[] = {1.0f, -0.75f};
  for (float v : V) for (float a : AMP) for (float u : U) for (float dz : DZ) for (float p : PR) for (float ud : UD)
    for (float f : FILL)
      printf("pm %08x %08x %08x %08x %08x %08x %08x %08x %d\n", bits(v), bits(a), bits(u), bits(dz), bits(p), bits(ud),
             bits(f), bits(lgx::scan_point_model(v, a, u, dz, p, ud, f)), (int)lgx::scan_point_lost(ud, p));
  const float RZ[] = {0.32f, 1.7f, -2.0f};
  const float H[] = {0.f, 0.25f, -0.4f};
  for (float rz : RZ) for (float h : H) printf("raw %08x %08x %08x\n", bits(rz), bits(h), bits(lgx::scan_raw(rz, h)));
  // the stream: slot -> (block, word) of LGX_SCAN_STREAM, against the block call
  for (int slot : {0, 1, 2, 3, 4, 131, LGX_MAX_HEIGHT_POINTS, LGX_MAX_HEIGHT_POINTS + 131}) {
    float u4[4];
    lgx::scan_uniform_block(0x123456789abcdefULL, 70000u, (1ULL << 33) + 5, slot >> 2, u4);
    printf("uni %d %08x %08x\n", slot, bits(lgx::scan_uniform(0x123456789abcdefULL, 70000u, (1ULL << 33) + 5, slot)),
           bits(u4[slot & 3]));
  }
  uint32_t o[4];
  philox4x32_10(70000u, 5u, 1u | ((uint32_t)LGX_SCAN_STREAM << 16), 2u, 0x89abcdefu, 0x1234567u, o);
  printf("phi %u %u %u %u %d\n", o[0], o[1], o[2], o[3], LGX_SCAN_STREAM);
  // the shared lookup on a 6 x 5 grid: points inside, on cell edges and far outside every border
  static int16_t hs[6 * 5];
  for (int i = 0; i < 30; ++i) hs[i] = (int16_t)((i * 37) % 23 - 11);
  P.border_size = 0.5f; P.horizontal_scale = 0.25f; P.vertical_scale = 0.005f; P.hf_rows = 6; P.hf_cols = 5;
  const float root[7] = {0.31f, -0.12f, 0.4f, 0.f, 0.f, 0.38268343f, 0.92387953f};
  float qy[4];
  lgx::scan_yaw_quat(root[5], root[6], qy);
  int cells = 0, same = 0;
  for (int a = -12; a <= 12; ++a)
    for (int b = -12; b <= 12; ++b) {
      const float bx = 0.11f * (float)a, by = 0.13f * (float)b;
      const float h_new = lgx::scan_point_height(&P, hs, qy, root, bx, by), h_old = old_scan_height(&P, hs, root, bx, by);
      long ix, iy, jx, jy;
      const float c_new = lgx::contact_terrain_height(&P, hs, bx, by, ix, iy), c_old = old_contact_height(&P, hs, bx, by, jx, jy);
      same += bits(h_new) == bits(h_old) && bits(c_new) == bits(c_old) && ix == jx && iy == jy;
      ++cells;
      if ((a + 12) % 6 == 0 && (b + 12) % 6 == 0) printf("cell %d %d %ld %ld %08x %08x\n", a, b, ix, iy, bits(c_new), bits(h_new));
    }
  long ix = 7, iy = 7;
  const float plane = lgx::contact_terrain_height(&P, nullptr, 1.f, 1.f, ix, iy);
  printf("grid %d %d %08x %ld %ld\n", cells, same, bits(plane), ix, iy);
  return 0;
}
"""


def f(word):
    return np.array([int(word, 16)], dtype=np.uint32).view(np.float32)[0]


def b(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def test_scan_rules_are_those_of_the_header(tmp_path):
    src, exe = tmp_path / "scan_probe.cpp", tmp_path / "scan_probe"
    src.write_text(PROGRAM)
    cmd = ["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", ROOT, "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    # the program allocates nothing; leak detection needs ptrace, which a container may refuse
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"),
                         timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.split("\n")
    one, two = np.float32(1.0), np.float32(2.0)

    pm = [ln.split()[1:] for ln in lines if ln.startswith("pm ")]
    assert len(pm) == 6 * 3 * 3 * 3 * 3 * 4 * 2
    neutral = lost_seen = kept_seen = noisy_clipped = 0
    for w in pm:
        v, amp, u, dz, p, ud, fill = (f(x) for x in w[:7])
        got, lost = int(w[7], 16), int(w[8])
        # the rule of include/lgx.h: noise, dz, dropout, clip; each sum a rounding of its own
        x = v
        if amp != 0:
            x = np.float32(x + np.float32(np.float32(two * u - one) * amp))
        if dz != 0:
            x = np.float32(x + dz)
        want_lost = bool(p > 0 and ud < p)
        if want_lost:
            x = fill
        x = np.float32(min(max(x, -one), one))
        assert lost == int(want_lost), w
        assert got == b(x), (w, hex(b(x)))
        if amp == 0 and dz == 0 and p == 0:
            assert got == int(w[0], 16)  # neutral: the identity on the bits (-0.0 included)
            neutral += 1
        lost_seen += want_lost
        kept_seen += (p > 0 and not want_lost)
        noisy_clipped += (amp != 0 and not want_lost and abs(x) == 1)
    assert neutral > 0 and lost_seen > 0 and kept_seen > 0 and noisy_clipped > 0
    # the order of the stages: a lost point ignores noise and dz; dz comes after the noise (two roundings)
    v, amp, u, dz = np.float32(0.07), np.float32(0.05), np.float32(0.3125), np.float32(0.03)
    noise_then_dz = np.float32(np.float32(v + np.float32(np.float32(two * u - one) * amp)) + dz)
    row = [w for w in pm if w[:5] == [f"{b(v):08x}", f"{b(amp):08x}", f"{b(u):08x}", f"{b(dz):08x}", f"{b(0.0):08x}"]][0]
    assert int(row[7], 16) == b(noise_then_dz)
    # the dropout threshold: u' < p is lost, u' == p is kept
    p = f"{b(0.3125):08x}"
    below = [w for w in pm if w[4] == p and w[5] == f"{b(np.float32(0.31249997)):08x}"]
    at = [w for w in pm if w[4] == p and w[5] == p]
    assert below and at and all(w[8] == "1" and w[7] == w[6] for w in below) and all(w[8] == "0" for w in at)
    assert all(w[8] == "1" for w in pm if w[4] == f"{b(1.0):08x}") and all(w[8] == "0" for w in pm if w[4] == f"{b(0.0):08x}")

    for w in (ln.split()[1:] for ln in lines if ln.startswith("raw ")):
        rz, h = f(w[0]), f(w[1])
        assert int(w[2], 16) == b(np.float32(min(max(np.float32(np.float32(rz - np.float32(0.3)) - h), -one), one)))

    uni = [ln.split()[1:] for ln in lines if ln.startswith("uni ")]
    assert len(uni) == 8 and all(w[1] == w[2] for w in uni) and len({w[1] for w in uni}) == 8
    from oracle import philox
    phi = [ln.split()[1:] for ln in lines if ln.startswith("phi ")][0]
    want = philox.philox4x32_10(np.uint32(70000), np.uint32(5), np.uint32(1 | (3 << 16)), np.uint32(2), 0x89abcdef, 0x1234567)
    assert [int(x) for x in phi[:4]] == [int(x) for x in want] and phi[4] == "3"
    slot5 = [w for w in uni if w[0] == "4"][0]  # block 1, word 0 of the same counter
    assert int(slot5[1], 16) == b(philox.to_uniform(want[0]))

    grid = [ln.split()[1:] for ln in lines if ln.startswith("grid ")][0]
    assert grid[0] == "625" and grid[1] == "625"  # every point: the old arithmetic's bits and cell
    assert grid[2] == f"{b(0.0):08x}" and grid[3:] == ["0", "0"]  # a plane: 0, cell (0, 0)
    cells = [[int(x) for x in ln.split()[1:5]] for ln in lines if ln.startswith("cell ")]
    assert {c[2] for c in cells} >= {0, 4} and {c[3] for c in cells} >= {0, 3}  # both clamped borders were reached
