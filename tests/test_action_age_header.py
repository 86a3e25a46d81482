"""The actuation-latency index rule of csrc/lgx_env_common.h (action_age, action_delay_clamp,
action_history_push), stand-alone, as tests/test_env_common_header.py does: a program that includes
only include/lgx.h and that header, built with the host backend's flags plus -Werror and
ASan/UBSan, run as a child process. action_age is compared with ceil(max(d - s, 0) / n) (include/lgx.h)
for every n in {1, 2, 4, 5}, d in [0, 4 n] and s in [0, n)."""
import math
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECIMATIONS = (1, 2, 4, 5)

PROGRAM = r"""
#include "include/lgx.h"
#include "legged_gym_custom_amd/csrc/lgx_env_common.h"

#include <stdio.h>

int main() {
  const int ns[] = {%(ns)s};
  for (int n : ns)
    for (int d = 0; d <= LGX_MAX_ACTION_HISTORY * n; ++d)
      for (int s = 0; s < n; ++s) printf("age %%d %%d %%d %%d\n", n, d, s, lgx::action_age(d, s, n));
  const int ds[] = {-2147483647 - 1, -1, 0, 7, 8, 9, 2147483647};
  for (int d : ds) printf("clamp %%d\n", lgx::action_delay_clamp(d, 2, 4));
  // [H = 3, A = 2] history of one env: a step that does not reset, then one that does
  float h[6] = {1, 2, 3, 4, 5, 6};
  for (int j = 0; j < 2; ++j) lgx::action_history_push(h, 3, 2, j, 10.f + j, false);
  printf("push %%g %%g %%g %%g %%g %%g\n", h[0], h[1], h[2], h[3], h[4], h[5]);
  for (int j = 0; j < 2; ++j) lgx::action_history_push(h, 3, 2, j, 20.f + j, true);
  printf("push %%g %%g %%g %%g %%g %%g\n", h[0], h[1], h[2], h[3], h[4], h[5]);
  float one[2] = {1, 2};  // H = 1: only row 0
  for (int j = 0; j < 2; ++j) lgx::action_history_push(one, 1, 2, j, 7.f + j, false);
  printf("push %%g %%g\n", one[0], one[1]);
  return 0;
}
"""


def test_action_age_is_the_rule_of_the_header(tmp_path):
    src, exe = tmp_path / "action_age_probe.cpp", tmp_path / "action_age_probe"
    src.write_text(PROGRAM % {"ns": ", ".join(str(n) for n in DECIMATIONS)})
    cmd = ["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", ROOT, "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    # the program allocates nothing; leak detection needs ptrace, which a container may refuse
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"),
                         timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.split("\n")
    got = [tuple(int(v) for v in ln.split()[1:]) for ln in lines if ln.startswith("age")]
    want = [(n, d, s, math.ceil(max(d - s, 0) / n)) for n in DECIMATIONS for d in range(4 * n + 1) for s in range(n)]
    assert got == want
    assert max(g[3] for g in got) == 4 and min(g[3] for g in got) == 0
    assert [int(ln.split()[1]) for ln in lines if ln.startswith("clamp")] == [0, 0, 0, 7, 8, 8, 8]
    assert [ln for ln in lines if ln.startswith("push")] == ["push 10 11 1 2 3 4", "push 20 21 0 0 0 0", "push 7 8"]
