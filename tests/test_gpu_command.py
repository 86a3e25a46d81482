"""The command schedule and the command-response evaluation (include/lgx.h, ABI 10) on the MI355X:
the bodies of tests/command_case.py on the gfx950 kernels (64 envs: two envs per wave on the plane,
63: one; go2_parkour: the trimesh instance), the step kernel against the host backend with a
schedule on, the records of the scripted inputs against the host backend's,
PolicyEvaluator.run_command_test end to end (graph replay against the eager loop), and the refusal
of a first allocation after a capture."""
import pytest
import torch

import command_case as K

pytestmark = pytest.mark.gpu
dev = "cuda:0"


@pytest.mark.parametrize("task,n", [("go2", 64), ("go2", 63), ("go2_parkour", 64)])
def test_schedule_equals_user_command(task, n):
    K.equals_user_command(task, n, dev)


@pytest.mark.parametrize("n", [64, 63])
def test_unscheduled_rows_and_unused_buffers_change_nothing(n):
    K.mixed_rows(n, dev)


def test_switch_timing_and_heading_bypass():
    K.switch_timing(64, dev)


def test_curriculum_redraw_keeps_the_schedule():
    K.curriculum_redraw(64, dev)


def test_kernel_matches_the_host_backend_with_a_schedule():
    K.backend_vs_host(63, dev)


@pytest.mark.parametrize("n", [1, 63, 130])
def test_records_and_cells_match_the_restatement_and_the_host_backend(n):
    env, ref = K.records_and_cells(n, dev)
    host, href = K.scripted_env(n, "cpu")[::2]  # the same generator seed: the same script
    assert torch.equal(href.rec, ref.rec)
    assert torch.equal(env.cmd_eval_status.cpu(), host.cmd_eval_status)
    rec, hrec = env.cmd_rec.cpu(), host.cmd_rec
    assert torch.equal(rec[:, [0, 1, 2, 4]], hrec[:, [0, 1, 2, 4]])
    K.check_command_records(rec, ref, f"hip n={n}")
    K.check_command_records(hrec, ref, f"host n={n}")


def test_command_test_end_to_end():
    K.end_to_end(dev)


def test_refusals():
    K.refusals(dev)
    K.command_test_refusals(dev)


def test_first_allocation_after_a_capture_is_refused():
    ev = K.evaluator(64, dev)
    ev.run(2)  # captures the plain loop on an env without schedule buffers
    assert ev._graph is not None and ev.env.cmd_step is None
    with pytest.raises(RuntimeError, match="captured"):
        ev.env.set_command_schedule([0], torch.zeros(1, 4))
    with pytest.raises(RuntimeError, match="captured"):
        ev.run_command_test([1.0], at_s=0.1)
    assert ev.env.cmd_step is None
