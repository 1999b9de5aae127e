"""The mirrored purification through the C ABI on the CPU baseline library: the rung conjugation and the generator G = K x 1 - 1 x K~ on
the host, api.thermal_greens_function(..., ancilla="mirror") and api.purification_defect against dense exact diagonalisation
(tests/thermal_mirror_common.py)."""
import pytest

import thermal_common as th
import thermal_mirror_common as tm
from cpu_ops import CpuOps


@pytest.fixture(scope="module")
def cpu_ops():
    return CpuOps()


@pytest.mark.parametrize("mode", th.MODES)
def test_rung_conjugate_of_every_site_operator(mode):
    tm.body_rung_conjugate(mode)


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("mode,case", th.COMBOS)
def test_mirror_generator_annihilates_the_infinite_temperature_state_dense(mode, case, L):
    tm.body_conjugation(mode, case, L)


@pytest.mark.parametrize("name,L", [("U13", 3), ("U13_u1", 3), ("two_band", 1), ("two_band_p", 1)])
def test_mirror_generator_of_assisted_hopping_and_two_bands_dense(name, L):
    tm.body_conjugation_extra(name, L)


def test_purified_hamiltonian_refusals_and_default():
    tm.body_refusals_host()


@pytest.mark.parametrize("mode,case", th.COMBOS)
def test_thermal_state_is_stationary_under_the_mirror_generator(cpu_ops, mode, case):
    tm.body_stationarity(cpu_ops, mode, case)


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("mode,case", th.COMBOS)
def test_mirror_scheme_against_ed(cpu_ops, mode, case, beta):
    tm.body_against_ed(cpu_ops, mode, case, beta)


def test_mirror_scheme_against_ed_four_sites(cpu_ops):
    tm.body_against_ed_l4(cpu_ops)


def test_default_is_the_idle_scheme(cpu_ops):
    tm.body_idle_unchanged(cpu_ops)


def test_one_sweep_per_interval_and_the_source_is_untouched(cpu_ops):
    tm.body_cost_and_purity(cpu_ops)


def test_purification_defect_orderings(cpu_ops):
    tm.body_defect(cpu_ops)


@pytest.mark.parametrize("mode,case", th.COMBOS)
def test_mirror_spectral_sum_rule(cpu_ops, mode, case):
    tm.body_sum_rule(cpu_ops, mode, case)
