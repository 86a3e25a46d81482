"""The joint-load record (include/lgx.h, ABI 13) on the MI355X: the bodies of tests/joint_case.py on
the gfx950 kernels joint_record_kernel / joint_reduce_kernel (csrc/lgx_env.hip), the kernels against
the host backend on the same script, and PolicyEvaluator.run(joints=True) end to end on real physics
(go2 at 64 envs: two envs per wave of the step kernel, 63: one; go2_parkour: the trimesh instance and
a terrain grid), graph replay against the eager loop bit for bit. Env counts: 1 = a single 16-lane
group, 63 = a partial last wave, 130 = past a 256-thread block's 16 envs with a partial group tail."""
import pytest

import joint_case as J

pytestmark = pytest.mark.gpu
dev = "cuda:0"


@pytest.mark.parametrize("n", [1, 63, 130])
def test_records_and_cells_match_the_restatement(n):
    J.records_and_cells(n, dev)


@pytest.mark.parametrize("n", [1, 63, 130])
def test_frozen_means_frozen(n):
    J.frozen_means_frozen(n, dev)


@pytest.mark.parametrize("n", [1, 63, 130])
def test_reduce_is_deterministic(n):
    J.reduce_is_deterministic(n, dev)


@pytest.mark.parametrize("n", [63, 130])
def test_kernels_match_the_host_backend(n):
    J.kernels_match_host(n)


@pytest.mark.parametrize("task,n", [("go2", 64), ("go2", 63), ("go2_parkour", 64)])
def test_end_to_end_on_real_physics(task, n):
    J.end_to_end(task, n, dev)


def test_composition():
    J.composition(dev)


def test_refusals():
    J.refusals(dev)
