"""The contact record (include/lgx.h, ABI 14) on the MI355X: the bodies of tests/contact_case.py on the
gfx950 kernels contact_begin_kernel / contact_record_kernel / contact_reduce_kernel (csrc/lgx_env.hip),
the kernels against the host backend on the same script bit for bit, and
PolicyEvaluator.run(contacts=True) end to end on real physics (go2 at 64 and 63 envs; go2_parkour: the
trimesh instance, a terrain grid and the terrain lookups), graph replay against the eager loop bit for
bit. Env counts: 1 = a single 32-lane group, 63 = the last wave half empty, 130 = past a 256-thread
block's 8 envs with a partial tail."""
import pytest

import contact_case as K

pytestmark = pytest.mark.gpu
dev = "cuda:0"


@pytest.mark.parametrize("task,n", [("go2", 1), ("go2", 63), ("go2", 130), ("go2_parkour", 1), ("go2_parkour", 63),
                                    ("go2_parkour", 130)])
def test_records_and_cells_match_the_restatement(task, n):
    K.records_and_cells(task, n, dev)


@pytest.mark.parametrize("n", [1, 63, 130])
def test_frozen_means_frozen(n):
    K.frozen_means_frozen(n, dev)


@pytest.mark.parametrize("n", [1, 63, 130])
def test_reduce_is_deterministic(n):
    K.reduce_is_deterministic(n, dev)


@pytest.mark.parametrize("task,n", [("go2", 63), ("go2", 130), ("go2_parkour", 63), ("go2_parkour", 130)])
def test_kernels_match_the_host_backend(task, n):
    K.kernels_match_host(task, n)


@pytest.mark.parametrize("task,n", [("go2", 64), ("go2", 63), ("go2_parkour", 64)])
def test_end_to_end_on_real_physics(task, n):
    K.end_to_end(task, n, dev)


def test_terminal_forces_are_the_steps():
    K.terminal_forces(dev)


def test_composition():
    K.composition(dev)


def test_total_row_matches_the_concatenated_envs():
    K.total_matches_concatenation(dev)


def test_refusals():
    K.refusals(dev)
