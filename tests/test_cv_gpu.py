"""Correction-vector sweeps on the MI355X: G(x, omega) against exact diagonalisation with the derived bar of the CPU test, the
amplitude convention, warm starts, the truncated run against the figure recorded on the CPU baseline library, refusals,
plan-cache hygiene.  Only the product library is loaded; the bodies are in cv_common.py."""
import pytest

import cv_common as cv

pytestmark = pytest.mark.gpu


def test_particle_part_against_exact_diagonalisation(hip_ops):
    print("largest deviation (MI355X):", cv.check_against_ed(hip_ops, "su2", "particle"))


@pytest.mark.parametrize("kind,part", [("u1", "particle"), ("su2", "hole")])
def test_single_spin_and_hole_part_against_exact_diagonalisation(hip_ops, kind, part):
    cv.check_against_ed(hip_ops, kind, part)


def test_amplitude_times_overlap_is_g_and_the_right_hand_side_is_only_read(hip_ops):
    cv.check_amplitude(hip_ops)


def test_scan_needs_no_more_sweeps_than_cold_solves(hip_ops):
    cv.check_warm_start(hip_ops)


def test_truncated_run_stays_at_the_cpu_figure(hip_ops):
    """same algorithm, only rounding and the SVD path differ: <= 2 x the deviation recorded on the CPU baseline library + 1e-9
    (no bound on the truncation error itself is derivable here)"""
    dev, tw = cv.truncated_case(hip_ops)
    print("truncated run, MI355X: deviation", dev, "trunc_weight", tw, "recorded CPU figure", cv.TRUNC_CPU_DEV)
    assert dev <= 2.0 * cv.TRUNC_CPU_DEV + 1e-9


def test_refusals(hip_ops):
    from hubbardtn_amd.device import HipOps
    cv.check_refusals(hip_ops, lambda: HipOps(0))


def test_sweep_after_a_correction_vector_plans_what_it_planned_without_it(hip_ops):
    cv.check_cache_hygiene(hip_ops)
