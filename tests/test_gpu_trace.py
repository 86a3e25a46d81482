"""The flight recorder (include/lgx.h, ABI 11) on the MI355X: the bodies of tests/trace_case.py on the
gfx950 kernels trace_record_kernel / trace_gather_kernel (csrc/lgx_env.hip), the kernels against the
host backend on the same script, and PolicyEvaluator.run(trace_depth=...) end to end on real physics
(go2 at 64 envs: two envs per wave of the step kernel, 63: one; go2_parkour: the trimesh instance and
a terrain grid), graph replay against the eager loop bit for bit."""
import pytest
import torch

import trace_case as T

pytestmark = pytest.mark.gpu
dev = "cuda:0"


@pytest.mark.parametrize("n", [1, 63, 130])
def test_ring_and_gather_match_the_restatement(n):
    T.ring_matches_restatement(n, dev)


@pytest.mark.parametrize("n", [1, 63])
def test_frozen_means_frozen(n):
    T.frozen_means_frozen(n, dev)


def test_peak_body_ties_and_zero_forces():
    T.peak_ties(dev)


@pytest.mark.parametrize("n", [63, 130])
def test_kernels_match_the_host_backend(n):
    env, _ = T.scripted(n, dev)
    host, _ = T.scripted(n, "cpu")  # the same generator seed: the same script
    assert torch.equal(env.trace_count.cpu(), host.trace_count)
    assert torch.equal(env.trace_status.cpu(), host.trace_status)
    ring, hring = env.trace_ring.cpu(), host.trace_ring
    assert torch.equal(ring[..., T.COPIED], hring[..., T.COPIED])
    err = (ring[..., T.NORMS] - hring[..., T.NORMS]).abs()
    print(f"hip vs host n={n}: norm columns max abs err {float(err.max()):.3e}")
    assert bool((err <= 1e-6 * hring[..., T.NORMS]).all())
    assert torch.equal(ring[..., 75], hring[..., 75])  # (the script leaves no near-tie: trace_case asserts it)
    ids = torch.arange(n - 1, -1, -1)
    (out, out_len), (hout, hlen) = env.trace_gather(ids), host.trace_gather(ids)
    assert torch.equal(out_len.cpu(), hlen) and torch.equal(out.cpu()[..., T.COPIED], hout[..., T.COPIED])


@pytest.mark.parametrize("task,n", [("go2", 64), ("go2", 63), ("go2_parkour", 64)])
def test_end_to_end_on_real_physics(task, n):
    T.end_to_end(task, n, dev)


def test_selection_of_falls():
    T.selection(dev)


def test_refusals():
    T.refusals(dev)
