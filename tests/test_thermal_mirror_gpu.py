"""The mirrored purification on the MI355X: the library bodies of test_thermal_mirror_cpu.py on the HIP library, with the same bounds,
against dense exact diagonalisation (not against the CPU run)."""
import pytest

import thermal_common as th
import thermal_mirror_common as tm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode,case", th.COMBOS)
def test_thermal_state_is_stationary_under_the_mirror_generator(hip_ops, mode, case):
    tm.body_stationarity(hip_ops, mode, case)


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("mode,case", th.COMBOS)
def test_mirror_scheme_against_ed(hip_ops, mode, case, beta):
    tm.body_against_ed(hip_ops, mode, case, beta)


def test_mirror_scheme_against_ed_four_sites(hip_ops):
    tm.body_against_ed_l4(hip_ops)


def test_default_is_the_idle_scheme(hip_ops):
    tm.body_idle_unchanged(hip_ops)


def test_one_sweep_per_interval_and_the_source_is_untouched(hip_ops):
    tm.body_cost_and_purity(hip_ops)


def test_purification_defect_orderings(hip_ops):
    tm.body_defect(hip_ops)


@pytest.mark.parametrize("mode,case", th.COMBOS)
def test_mirror_spectral_sum_rule(hip_ops, mode, case):
    tm.body_sum_rule(hip_ops, mode, case)
