"""Actuation latency and motor strength (include/lgx.h, ABI 8) in the gfx950 step kernel: every
env_step_kernel instance (plane at two envs and one env per wave, trimesh terrain, actuator net) on
the reductions of tests/actuator_case.py, the kernel against the host backend with both features
on, the evaluator's latency options on the captured loop, and a graph-captured training run."""
import pytest

import actuator_case as A
from test_actuator_host import evaluate_cli_document, evaluator_options

pytestmark = pytest.mark.gpu
dev = "cuda:0"


@pytest.mark.parametrize("task,n,steps", [("go2", 64, 12), ("go2", 63, 12), ("go2_parkour", 64, 12),
                                          ("anymal_c_rough", 64, 8)])
def test_whole_step_latency_is_a_shifted_action(task, n, steps, tmp_path):
    A.whole_step_shift(task, n, dev, steps, tmp_path)


@pytest.mark.parametrize("task,steps", [("go2", 12), ("anymal_c_rough", 8)])
def test_substep_latency_matches_a_split_step(task, steps, tmp_path):
    A.substep_delays(task, 64, dev, steps, tmp_path)


def test_motor_strength_scales_the_gains():
    A.motor_strength_go2(dev)


def test_motor_strength_scales_the_actuator_net(tmp_path):
    A.motor_strength_anymal(dev, tmp_path)


@pytest.mark.parametrize("n", [64, 63])
def test_kernel_matches_the_host_backend_with_both_features_on(n):
    A.backend_vs_host(n, dev)


def test_zero_delay_and_unit_strength_change_nothing():
    A.identity(dev)


def test_setup_draws_on_the_device(monkeypatch):
    A.setup_draws(dev, monkeypatch)


def test_refusals_fail_cleanly_on_the_device():
    A.refusals(dev)


def test_evaluator_latency_options_on_the_captured_loop():
    evaluator_options(dev)


def test_evaluate_cli_document(tmp_path):
    evaluate_cli_document(dev, tmp_path)


def test_training_with_both_features_on_keeps_the_captured_rollout():
    A.training_smoke(dev)
