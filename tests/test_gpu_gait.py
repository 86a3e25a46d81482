"""The gait record (include/lgx.h, ABI 12) on the MI355X: the bodies of tests/gait_case.py on the
gfx950 kernels gait_record_kernel / gait_reduce_kernel (csrc/lgx_env.hip), the kernels against the
host backend on the same script, and PolicyEvaluator.run(gait=True) end to end on real physics (go2
at 64 envs: two envs per wave of the step kernel, 63: one; go2_parkour: the trimesh instance and a
terrain grid), graph replay against the eager loop bit for bit."""
import pytest

import gait_case as G

pytestmark = pytest.mark.gpu
dev = "cuda:0"


@pytest.mark.parametrize("n", [1, 63, 130])
def test_records_and_cells_match_the_restatement(n):
    G.records_and_cells(n, dev)


@pytest.mark.parametrize("n", [1, 63, 130])
def test_frozen_means_frozen(n):
    G.frozen_means_frozen(n, dev)


@pytest.mark.parametrize("n", [1, 63, 130])
def test_reduce_is_deterministic(n):
    G.reduce_is_deterministic(n, dev)


@pytest.mark.parametrize("n", [63, 130])
def test_kernels_match_the_host_backend(n):
    G.kernels_match_host(n)


@pytest.mark.parametrize("task,n", [("go2", 64), ("go2", 63), ("go2_parkour", 64)])
def test_end_to_end_on_real_physics(task, n):
    G.end_to_end(task, n, dev)


def test_composition():
    G.composition(dev)


def test_refusals():
    G.refusals(dev)
