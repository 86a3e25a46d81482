"""The per-env height-scan model (include/lgx.h, ABI 17) on liblgx.so's host backend: the bodies of
tests/test_gpu_scan.py (tests/scan_case.py) with device="cpu", the refusals, the setup draws, and
the evaluator's scan test on the eager CPU loop."""
import pytest

import scan_case as S

CASES = pytest.mark.parametrize("task,n,epw,steps", S.CASES, ids=S.IDS)


@CASES
def test_host_neutral_scan_buffers_change_nothing(task, n, epw, steps):
    S.identity(task, n, "cpu", epw, steps)


@CASES
def test_host_scan_model_touches_the_scan_only(task, n, epw, steps):
    S.others_untouched(task, n, "cpu", epw, steps)


@CASES
def test_host_scan_latency_is_a_shifted_row(task, n, epw, steps):
    S.latency_shift(task, n, "cpu", epw, steps)


@CASES
def test_host_scan_noise_is_the_philox_stream_of_its_own(task, n, epw, steps):
    S.noise(task, n, "cpu", epw, steps)


@CASES
def test_host_scan_dropout_loses_exactly_the_drawn_points(task, n, epw, steps):
    S.dropout(task, n, "cpu", epw, steps)


@pytest.mark.parametrize("epw", [None, 2])
def test_host_scan_xy_offset_is_a_scan_at_the_shifted_points(epw):
    S.offset_xy(64, "cpu", epw, 8)


@CASES
def test_host_scan_z_offset_is_an_added_constant(task, n, epw, steps):
    S.offset_z(task, n, "cpu", epw, steps)


@pytest.mark.parametrize("n", [64, 63])
def test_host_backend_all_four_on(n):
    S.backend_vs_host(n, "cpu")


def test_scan_refusals_fail_cleanly(tmp_path):
    S.refusals("cpu", tmp_path)


def test_host_allocating_scan_setter_is_refused_after_a_capture():
    S.captured_refusal("cpu")


def test_scan_setup_draws_leave_existing_draws_alone_and_slice_by_rank(monkeypatch):
    S.setup_draws("cpu", monkeypatch)


def test_host_evaluator_scan_test():
    S.evaluator("cpu")


def test_host_evaluate_cli_scan_document(tmp_path):
    S.evaluate_cli_document("cpu", tmp_path)


def test_host_training_with_the_scan_randomisations_on():
    S.training_smoke("cpu", num_steps_per_env=8)
