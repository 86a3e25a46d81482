"""The per-env sensor model (include/lgx.h, ABI 15) on liblgx.so's host backend: the bodies of
tests/test_gpu_sensor.py (tests/sensor_case.py) with device="cpu", the layouts, the refusals, the
setup draws, and the evaluator's sensor test on the eager CPU loop."""
import pytest

import sensor_case as S


@pytest.mark.parametrize("task,n,steps", S.CASES)
def test_host_latency_is_a_shifted_row(task, n, steps, tmp_path):
    S.latency_shift(task, n, "cpu", steps, tmp_path)


def test_host_latency_on_the_trimesh_at_two_envs_per_wave(tmp_path):
    S.latency_shift("go2_parkour", 64, "cpu", 10, tmp_path, envs_per_wave=2)


@pytest.mark.parametrize("task,n,steps", S.CASES)
def test_host_bias_is_an_added_constant(task, n, steps, tmp_path):
    S.bias_added(task, n, "cpu", steps, tmp_path)


@pytest.mark.parametrize("task,n,steps", S.CASES)
def test_host_noise_scale_interpolates_between_noise_off_and_on(task, n, steps, tmp_path):
    S.noise_scale(task, n, "cpu", steps, tmp_path)


@pytest.mark.parametrize("task,n", [c[:2] for c in S.CASES])
def test_host_neutral_buffers_change_nothing(task, n, tmp_path):
    S.identity(task, n, "cpu", tmp_path)


def test_host_command_curriculum_rewrite_carries_scale_and_bias():
    S.curriculum_rewrite(64, "cpu")


@pytest.mark.parametrize("n", [64, 63])
def test_host_backend_all_three_on(n):
    S.backend_vs_host(n, "cpu")


def test_sensor_setup_draws_leave_existing_draws_alone_and_slice_by_rank(monkeypatch):
    S.setup_draws("cpu", monkeypatch)


def test_layouts_groups_and_amplitudes():
    S.layouts_and_amplitudes()


def test_sensor_refusals_fail_cleanly():
    S.refusals("cpu")


def test_host_allocating_setter_is_refused_after_a_capture():
    S.captured_refusal("cpu")


def test_host_evaluator_sensor_test():
    S.evaluator("cpu")


def test_host_evaluate_cli_sensor_document(tmp_path):
    S.evaluate_cli_document("cpu", tmp_path)


def test_host_training_with_the_sensor_randomisations_on():
    S.training_smoke("cpu", num_steps_per_env=8)
