"""The sensor model's scalar rules of csrc/lgx_env_common.h (sensor_channel, sensor_delay_clamp,
sensor_ring_read_row / sensor_ring_write_row, sensor_noise_bias; include/lgx.h ABI 15), stand-alone,
as tests/test_action_age_header.py does: a program that includes only include/lgx.h and that
header, built with the host backend's flags plus -Werror and ASan/UBSan, run as a child process.
The ring-index rule is driven over every K in 1..4, d in -1..K+1 and c in 0..2K+1 against the rule
of include/lgx.h restated here (d_eff = min(clamp(d, 0, K), c), read row (c - d_eff) % K, write row
c % K); the sensor-channel predicate is compared with the layout functions of params.py."""
import os
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "include/lgx.h"
#include "legged_gym_custom_amd/csrc/lgx_env_common.h"

#include <stdio.h>
#include <string.h>

static unsigned bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }

int main() {
  for (int K = 1; K <= LGX_MAX_SENSOR_HISTORY; ++K)
    for (int d = -1; d <= K + 1; ++d)
      for (int c = 0; c <= 2 * K + 1; ++c) {
        const int de = lgx::sensor_delay_clamp(d, K, c);
        // a ring of K rows, as the step uses it: the read stays inside it (ASan / UBSan watch)
        float ring[LGX_MAX_SENSOR_HISTORY];
        for (int r = 0; r < K; ++r) ring[r] = (float)r;
        const int rr = de > 0 ? lgx::sensor_ring_read_row(c, de, K) : -1, wr = lgx::sensor_ring_write_row(c, K);
        const float got = de > 0 ? ring[rr] : -1.f;
        ring[wr] = 100.f;
        printf("ring %d %d %d %d %d %d %g\n", K, d, c, de, rr, wr, got);
      }
  const int big[] = {-2147483647 - 1, 2147483647};
  for (int d : big) printf("clamp %d\n", lgx::sensor_delay_clamp(d, 3, 2147483647));
  for (int go2 = 0; go2 < 2; ++go2) {
    const int P = go2 ? 52 : 235;
    printf("chan %d", go2);
    for (int i = 0; i < P; ++i) printf(" %d", (int)lgx::sensor_channel(go2 != 0, i, 12, 12));
    printf("\n");
  }
  // noise and bias: unbound, scale 1 / bias 0, scale 0, a scale and a bias
  const float v = 0.3f, u = 0.8125f, nv = 0.01f, one = 1.f, zero = 0.f, two = 2.f, b = 0.125f, nz = -0.f;
  printf("nb %08x %08x %08x %08x %08x %08x %08x\n", bits(lgx::sensor_noise_bias(v, true, u, nv, nullptr, nullptr)),
         bits(lgx::sensor_noise_bias(v, true, u, nv, &one, &zero)), bits(lgx::sensor_noise_bias(v, true, u, nv, &zero, nullptr)),
         bits(lgx::sensor_noise_bias(v, false, u, nv, &two, nullptr)), bits(lgx::sensor_noise_bias(v, true, u, nv, &two, &b)),
         bits(lgx::sensor_noise_bias(nz, true, u, nv, &zero, &zero)), bits(lgx::sensor_noise_bias(nz, false, u, nv, nullptr, nullptr)));
  return 0;
}
"""


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def bits(x):
    return struct.unpack("I", struct.pack("f", x))[0]


def test_sensor_rules_are_those_of_the_header(tmp_path):
    src, exe = tmp_path / "sensor_probe.cpp", tmp_path / "sensor_probe"
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
    got = [tuple(int(float(v)) for v in ln.split()[1:]) for ln in lines if ln.startswith("ring")]
    want = []
    for K in range(1, 5):
        for d in range(-1, K + 2):
            for c in range(2 * K + 2):
                de = min(min(max(d, 0), K), c)
                rr = (c - de) % K if de > 0 else -1
                want.append((K, d, c, de, rr, c % K, rr))  # (the ring held its row numbers)
    assert got == want
    assert max(g[3] for g in got) == 4 and any(g[4] == g[5] and g[3] > 0 for g in got)  # d = K reads the row it overwrites
    assert [int(ln.split()[1]) for ln in lines if ln.startswith("clamp")] == [0, 3]

    from legged_gym_custom_amd import params as prm
    for go2, layout in ((1, prm.go2_proprio_layout(12)), (0, prm.legged_proprio_layout(12, 12, 187))):
        mask = []
        for name, width in layout:
            mask += [int(name in prm.SENSOR_GROUPS)] * width
        line = [ln for ln in lines if ln.startswith(f"chan {go2}")][0]
        assert [int(v) for v in line.split()[2:]] == mask, go2
        assert 0 < sum(mask) < len(mask)

    v, n, nv = f32(0.3), f32(f32(2.0 * 0.8125) - 1.0), f32(0.01)
    plain = f32(v + f32(n * nv))
    both = f32(f32(v + f32(n * f32(nv * 2.0))) + 0.125)
    nb = [int(x, 16) for x in [ln for ln in lines if ln.startswith("nb")][0].split()[1:]]
    assert nb == [bits(plain), bits(plain), bits(v), bits(v), bits(both), bits(-0.0), bits(-0.0)]
