"""Finite-temperature dynamics on the MI355X: the bodies of test_thermal_dyn_cpu.py on the HIP library, with the same bounds, against
dense exact diagonalisation (not against the CPU run)."""
import pytest

import thermal_dyn_common as td

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("mode,case", td.COMBOS)
def test_equal_time_is_the_correlation_function(hip_ops, mode, case, beta):
    td.body_equal_time(hip_ops, mode, case, beta)


@pytest.mark.parametrize("mode,case", td.COMBOS)
def test_without_truncation_against_ed(hip_ops, mode, case):
    td.body_against_ed(hip_ops, mode, case)


def test_order_of_the_splitting(hip_ops):
    td.body_splitting(hip_ops)


@pytest.mark.parametrize("mode,case", td.COMBOS)
def test_spectral_function_and_sum_rule(hip_ops, mode, case):
    td.body_spectral(hip_ops, mode, case)


def test_state_that_was_never_cooled(hip_ops):
    td.body_beta0_dynamics(hip_ops)


def test_truncating_run(hip_ops):
    td.body_truncating(hip_ops)


def test_source_state_is_untouched(hip_ops):
    td.body_untouched(hip_ops)


def test_refusals(hip_ops):
    from hubbardtn_amd.device import HipOps
    td.body_refusals(hip_ops, lambda: HipOps(0))
