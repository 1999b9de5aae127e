"""Two-site TDVP through the C ABI on the CPU baseline library (the engine's host logic and the host statement of the Krylov
exponential, htn::Backend::krylov_expm): dense exact diagonalisation of small chains is the reference (tests/tdvp_common.py)."""
import pytest

import tdvp_common as tc
from cpu_ops import CpuOps


@pytest.fixture(scope="module")
def cpu_ops():
    return CpuOps()


def test_l2_is_exact(cpu_ops):
    tc.body_l2_exact(cpu_ops)


def test_energy_and_density_conserved(cpu_ops):
    tc.body_conservation(cpu_ops)


def test_reversibility(cpu_ops):
    tc.body_reversibility(cpu_ops)


def test_second_order_against_ed(cpu_ops):
    tc.body_second_order(cpu_ops)


def test_imaginary_time_reaches_the_ground_state(cpu_ops):
    tc.body_imaginary_time(cpu_ops)


def test_log_norm_l2(cpu_ops):
    tc.body_log_norm_l2(cpu_ops)


def test_truncation(cpu_ops):
    tc.body_truncation(cpu_ops)


def test_spinful_mode(cpu_ops):
    tc.body_spinful(cpu_ops)


def test_refusals(cpu_ops):
    tc.body_refusals(cpu_ops)


def test_api_time_evolve(cpu_ops):
    tc.body_api_time_evolve(cpu_ops)
