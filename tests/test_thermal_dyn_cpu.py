"""Finite-temperature dynamics through the C ABI on the CPU baseline library: api.thermal_greens_function (both states of the
purification evolved by two-site TDVP) and api.thermal_spectral_function against dense exact diagonalisation
(tests/thermal_dyn_common.py)."""
import pytest

import thermal_dyn_common as td
from cpu_ops import CpuOps


@pytest.fixture(scope="module")
def cpu_ops():
    return CpuOps()


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("mode,case", td.COMBOS)
def test_equal_time_is_the_correlation_function(cpu_ops, mode, case, beta):
    td.body_equal_time(cpu_ops, mode, case, beta)


@pytest.mark.parametrize("mode,case", td.COMBOS)
def test_without_truncation_against_ed(cpu_ops, mode, case):
    td.body_against_ed(cpu_ops, mode, case)


def test_order_of_the_splitting(cpu_ops):
    td.body_splitting(cpu_ops)


@pytest.mark.parametrize("mode,case", td.COMBOS)
def test_spectral_function_and_sum_rule(cpu_ops, mode, case):
    td.body_spectral(cpu_ops, mode, case)


def test_state_that_was_never_cooled(cpu_ops):
    td.body_beta0_dynamics(cpu_ops)


def test_truncating_run(cpu_ops):
    td.body_truncating(cpu_ops)


def test_source_state_is_untouched(cpu_ops):
    td.body_untouched(cpu_ops)


def test_refusals(cpu_ops):
    td.body_refusals(cpu_ops, CpuOps)
