"""The per-env height-scan model (include/lgx.h, ABI 17) in the gfx950 step kernel's SENSOR
instances (plane at two envs and one env per wave, trimesh terrain at one and two envs per wave)
on the reductions of tests/scan_case.py, the kernel against the host backend with all four effects
on, the evaluator's scan test on the captured loop, and a graph-captured training run."""
import pytest

import scan_case as S

pytestmark = pytest.mark.gpu
dev = "cuda:0"
CASES = pytest.mark.parametrize("task,n,epw,steps", S.CASES, ids=S.IDS)


@CASES
def test_neutral_scan_buffers_change_nothing(task, n, epw, steps):
    S.identity(task, n, dev, epw, steps)


@CASES
def test_scan_model_touches_the_scan_only(task, n, epw, steps):
    S.others_untouched(task, n, dev, epw, steps)


@CASES
def test_scan_latency_is_a_shifted_row(task, n, epw, steps):
    S.latency_shift(task, n, dev, epw, steps)


@CASES
def test_scan_noise_is_the_philox_stream_of_its_own(task, n, epw, steps):
    S.noise(task, n, dev, epw, steps)


@CASES
def test_scan_dropout_loses_exactly_the_drawn_points(task, n, epw, steps):
    S.dropout(task, n, dev, epw, steps)


@pytest.mark.parametrize("epw", [None, 2])
def test_scan_xy_offset_is_a_scan_at_the_shifted_points(epw):
    S.offset_xy(64, dev, epw, 8)


@CASES
def test_scan_z_offset_is_an_added_constant(task, n, epw, steps):
    S.offset_z(task, n, dev, epw, steps)


@pytest.mark.parametrize("n", [64, 63])
def test_kernel_matches_the_host_backend_with_all_four_on(n):
    S.backend_vs_host(n, dev)


def test_scan_refusals_and_clamps_on_the_device(tmp_path):
    S.refusals(dev, tmp_path)


def test_allocating_scan_setter_is_refused_after_a_capture():
    S.captured_refusal(dev)


def test_scan_setup_draws_on_the_device(monkeypatch):
    S.setup_draws(dev, monkeypatch)


def test_evaluator_scan_test_on_the_captured_loop():
    S.evaluator(dev)


def test_evaluate_cli_scan_document(tmp_path):
    S.evaluate_cli_document(dev, tmp_path)


def test_training_with_the_scan_randomisations_on_stays_captured():
    S.training_smoke(dev)
