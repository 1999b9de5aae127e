"""Correction-vector sweeps on the CPU baseline library (the product's engine sources on host kernels, the host statement of the
shifted solve): G(x, omega) against exact diagonalisation, the amplitude convention, warm starts, a truncated run, refusals,
plan-cache hygiene.  The bodies are in cv_common.py."""
import pytest

import cv_common as cv
from cpu_ops import CpuOps


@pytest.fixture(scope="module")
def cpu_ops():
    return CpuOps()


def test_particle_part_against_exact_diagonalisation(cpu_ops):
    print("largest deviation (CPU baseline library):", cv.check_against_ed(cpu_ops, "su2", "particle"))


@pytest.mark.parametrize("kind,part", [("u1", "particle"), ("su2", "hole")])
def test_single_spin_and_hole_part_against_exact_diagonalisation(cpu_ops, kind, part):
    cv.check_against_ed(cpu_ops, kind, part)


def test_amplitude_times_overlap_is_g_and_the_right_hand_side_is_only_read(cpu_ops):
    cv.check_amplitude(cpu_ops)


def test_scan_needs_no_more_sweeps_than_cold_solves(cpu_ops):
    cv.check_warm_start(cpu_ops)


def test_truncated_run_reports_its_deviation(cpu_ops):
    dev, tw = cv.truncated_case(cpu_ops)
    print("truncated run, CPU baseline library: deviation", dev, "trunc_weight", tw, "recorded", cv.TRUNC_CPU_DEV)
    assert dev <= 2.0 * cv.TRUNC_CPU_DEV + 1e-9             # (the recorded figure is this run's: the GPU test holds the same line)


def test_refusals(cpu_ops):
    cv.check_refusals(cpu_ops, CpuOps)


def test_sweep_after_a_correction_vector_plans_what_it_planned_without_it(cpu_ops):
    cv.check_cache_hygiene(cpu_ops)
