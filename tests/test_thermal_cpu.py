"""Finite temperature through the C ABI on the CPU baseline library: purified thermal states (api.thermal_state) cooled by two-site
TDVP (api.cool) against dense grand-canonical exact diagonalisation (tests/thermal_common.py)."""
import pytest

import thermal_common as th
from cpu_ops import CpuOps


@pytest.fixture(scope="module")
def cpu_ops():
    return CpuOps()


@pytest.mark.parametrize("L", [3, 4])
@pytest.mark.parametrize("mode,case", th.COMBOS)
def test_beta_zero_is_exact(cpu_ops, mode, case, L):
    th.body_beta0(cpu_ops, mode, case, L)


@pytest.mark.parametrize("mode,case", th.COMBOS)
def test_purified_hamiltonian_traces_and_ancilla_parities_dense(mode, case):
    th.body_dense_identity(mode, case)


def test_hamiltonian_is_what_it_was_before_the_term_list_was_split_off():
    th.body_refactor_guard()


@pytest.mark.parametrize("L", [3, 4])
@pytest.mark.parametrize("mode,case", th.COMBOS)
def test_cooling_without_truncation_against_ed(cpu_ops, mode, case, L):
    th.body_cooling(cpu_ops, mode, case, L)


def test_small_steps_keep_both_seed_sweeps(cpu_ops):
    th.body_small_steps(cpu_ops)


def test_continuation(cpu_ops):
    th.body_continuation(cpu_ops)


def test_truncating_run(cpu_ops):
    th.body_truncating(cpu_ops)


def test_refusals(cpu_ops):
    th.body_refusals(cpu_ops, CpuOps)
