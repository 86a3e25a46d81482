"""The sustained external force (include/lgx.h, ABI 16) on the MI355X: the bodies of
tests/force_case.py on the gfx950 kernels (the plane at two envs per wave and at one, the trimesh,
the actuator net), the step kernel against the host backend with forces on,
PolicyEvaluator.run_force_test end to end (graph replay against the eager loop), the evaluate.py
--force_n document, the refusal of a first allocation after a capture and a short training run
with the randomisation on.

Measured on the MI355X (64 and 63 envs): momentum law |P - (f + M g) dt| / (|f| dt), bound 2e-2: Go2 on
the plane at two envs per wave and at one, and on the trimesh: 6.9e-5 .. 6.7e-4 for the four fixed
30 N cases, worst 3.6e-3 over the random rows (5 .. 27 N); ANYmal 4.5e-5 .. 1.8e-4. Line of action
at 4 N: the point slid 0.2 m along the force 0.10 x the bound (7.5e-5 root state, 1.7e-3 N), 0.2 m
to the side 23 x. Kernel against host backend, 16 steps, forces on in 65 % of the env steps: joint
state 6.5e-4, torques 8.8e-4 N m, contact forces 2.1e-3 N, root state 4.7e-5, observations 3.3e-5.
Evaluator records against the float64 restatement: sums 2.7e-7 relative, peak tilt 1.0e-7 rad,
achieved-velocity sums 0.06 x their bound."""
import pytest

import force_case as F

pytestmark = pytest.mark.gpu
dev = "cuda:0"


@pytest.mark.parametrize("task,n,epw", F.INSTANCES)
def test_off_windows_and_zero_forces_change_nothing(task, n, epw, tmp_path):
    F.identity(task, n, dev, tmp_path, epw)


@pytest.mark.parametrize("n", [64, 63])
def test_unforced_neighbours_in_a_wave_keep_their_bits(n):
    F.neighbours(n, dev)


@pytest.mark.parametrize("n", [64, 63])
def test_window_rule(n):
    F.window_rule(n, dev)


@pytest.mark.parametrize("oriented", [False, True])
@pytest.mark.parametrize("task,n,epw", F.INSTANCES)
def test_momentum_law(task, n, epw, oriented, tmp_path):
    F.momentum_law(task, n, dev, tmp_path, epw, oriented)


def test_line_of_action():
    F.line_of_action(dev)


@pytest.mark.parametrize("n", [64, 63])
def test_kernel_matches_the_host_backend_with_forces_on(n):
    F.backend_vs_host(n, dev)


def test_refusals():
    F.refusals(dev)
    F.force_test_refusals(dev)


def test_first_allocation_after_a_capture_is_refused():
    F.captured_refusal(dev)


def test_setup_draws_leave_existing_draws_alone_and_slice_by_rank(monkeypatch):
    F.setup_draws(dev, monkeypatch)


def test_force_test_end_to_end():
    F.end_to_end(dev)


def test_evaluate_cli_force_document(tmp_path):
    F.evaluate_cli_document(dev, tmp_path)


def test_training_with_the_force_randomisation_on():
    F.training_smoke(dev)
