"""The per-env sensor model (include/lgx.h, ABI 15) in the gfx950 step kernel: every
env_step_kernel instance (plane at two envs and one env per wave, trimesh terrain, actuator net
with the long history shifted in HBM) on the reductions of tests/sensor_case.py, the kernel against the host
backend with all three features on, the evaluator's sensor test on the captured loop, and a
graph-captured training run."""
import pytest

import sensor_case as S

pytestmark = pytest.mark.gpu
dev = "cuda:0"


@pytest.mark.parametrize("task,n,steps", S.CASES)
def test_latency_is_a_shifted_row(task, n, steps, tmp_path):
    S.latency_shift(task, n, dev, steps, tmp_path)


def test_latency_on_the_trimesh_at_two_envs_per_wave(tmp_path):
    S.latency_shift("go2_parkour", 64, dev, 10, tmp_path, envs_per_wave=2)


@pytest.mark.parametrize("task,n,steps", S.CASES)
def test_bias_is_an_added_constant(task, n, steps, tmp_path):
    S.bias_added(task, n, dev, steps, tmp_path)


@pytest.mark.parametrize("task,n,steps", S.CASES)
def test_noise_scale_interpolates_between_noise_off_and_on(task, n, steps, tmp_path):
    S.noise_scale(task, n, dev, steps, tmp_path)


@pytest.mark.parametrize("task,n", [c[:2] for c in S.CASES])
def test_neutral_buffers_change_nothing(task, n, tmp_path):
    S.identity(task, n, dev, tmp_path)


def test_command_curriculum_rewrite_carries_scale_and_bias():
    S.curriculum_rewrite(64, dev)


@pytest.mark.parametrize("n", [64, 63])
def test_kernel_matches_the_host_backend_with_all_three_on(n):
    S.backend_vs_host(n, dev)


def test_setup_draws_on_the_device(monkeypatch):
    S.setup_draws(dev, monkeypatch)


def test_refusals_and_clamps_on_the_device():
    S.refusals(dev)


def test_allocating_setter_is_refused_after_a_capture():
    S.captured_refusal(dev)


def test_evaluator_sensor_test_on_the_captured_loop():
    S.evaluator(dev)


def test_evaluate_cli_sensor_document(tmp_path):
    S.evaluate_cli_document(dev, tmp_path)


def test_training_with_the_sensor_randomisations_on_stays_captured():
    S.training_smoke(dev)
