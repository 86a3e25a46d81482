"""Scheduled pushes and the push-recovery evaluation (include/lgx.h, ABI 9) on the MI355X: the
bodies of tests/push_case.py on the gfx950 kernels (64 envs: two envs per wave, 63: one), the step
kernel against the host backend with a schedule on, the records of the scripted inputs against the
host backend's, PolicyEvaluator.run_push_test end to end (graph replay against the eager loop),
and the refusal of a first allocation after a capture."""
import pytest
import torch

import push_case as P

pytestmark = pytest.mark.gpu
dev = "cuda:0"


@pytest.mark.parametrize("n", [64, 63])
def test_scheduled_push_is_a_velocity_edit(n):
    P.velocity_edit(n, dev)


def test_unscheduled_buffers_change_nothing():
    P.identity(dev)


def test_kernel_matches_the_host_backend_with_a_schedule():
    P.backend_vs_host(63, dev)


@pytest.mark.parametrize("n", [1, 63, 130])
def test_records_and_cells_match_the_restatement_and_the_host_backend(n):
    env, ref = P.records_and_cells(n, dev)
    host, href = P.scripted_env(n, "cpu")[::2]  # the same generator seed: the same script
    assert torch.equal(href.rec, ref.rec)
    assert torch.equal(env.push_eval_status.cpu(), host.push_eval_status)
    rec, hrec = env.push_rec.cpu(), host.push_rec
    assert torch.equal(rec[:, [0, 3]], hrec[:, [0, 3]])
    ref.rec = hrec.double()
    P.check_push_records(rec, ref, f"hip vs host n={n}")


def test_push_test_end_to_end():
    P.end_to_end(dev)


def test_refusals():
    P.refusals(dev)
    P.push_test_refusals(dev)


def test_first_allocation_after_a_capture_is_refused():
    ev = P.evaluator(66, dev)
    ev.run(2)  # captures the plain loop on an env without push buffers
    assert ev._graph is not None and ev.env.push_step is None
    with pytest.raises(RuntimeError, match="captured"):
        ev.env.set_push_schedule(3, torch.zeros(3))
    with pytest.raises(RuntimeError, match="captured"):
        ev.run_push_test([1.0], directions=4, at_s=0.06)
    assert ev.env.push_step is None
