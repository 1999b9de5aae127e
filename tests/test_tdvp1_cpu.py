"""One-site TDVP at fixed bond tables on the CPU baseline library (the product's planner and driver on host kernels): the
zero-site effective Hamiltonian against Q^H H_eff1 Q, conservation, reversibility, the splitting error against exact
diagonalisation, imaginary time, the API selector and the C entry points.  Bodies in tdvp1_common.py."""
import ctypes as C

import pytest

import tdvp1_common as t1
from cpu_ops import CpuOps
from hubbardtn_amd import abi


@pytest.fixture(scope="module")
def cpu_ops():
    return CpuOps()


@pytest.fixture(scope="module")
def ed_errors(cpu_ops):
    return t1.ed_errors(cpu_ops)


@pytest.mark.parametrize("case", t1.CASES)
def test_heff0_is_heff1_between_the_isometries(cpu_ops, case):
    t1.body_heff0_identity(cpu_ops, case)


def test_heff0_on_sectors_wider_than_one_quadrant(cpu_ops):
    """a cap of 300 at L = 10: sectors of dimension 20 and 22, an apply tile of more than one 16 x 16 quadrant"""
    t1.body_heff0_identity(cpu_ops, "SU2U1", chi=300, sweeps=2, wider_than=16)


def test_energy_norm_and_tables_are_conserved_under_a_cap(cpu_ops):
    t1.body_conservation(cpu_ops)


def test_a_step_is_reversible(cpu_ops):
    t1.body_reversibility(cpu_ops)


def test_splitting_error_against_exact_diagonalisation(ed_errors):
    """the figures of tdvp1_common.CPU_ED_ERRORS were measured by this test's own run on this library"""
    t1.check_ed_errors(ed_errors)
    assert all(abs(ed_errors[k] / v - 1.0) <= 0.05 for k, v in t1.CPU_ED_ERRORS.items())       # (the record is this library's)


def test_imaginary_time_reaches_the_one_site_dmrg_energy(cpu_ops):
    t1.body_imaginary_time(cpu_ops)


def test_api_selector_hand_over_and_refusals(cpu_ops, ed_errors):
    t1.body_api(cpu_ops, ed_errors[0.05])


def test_entry_points_of_both_libraries(cpu_ops):
    """the four new symbols in the CPU baseline library and in the HIP library (loading needs no GPU), the version number both
    sides share, a sweep refused with the centre off site 0"""
    t1.body_abi(cpu_ops, cpu_ops.lib)
    hip = abi.load_library()
    for n in t1.NEW_SYMBOLS:
        assert hasattr(hip, n), n
    assert hip.htn_abi_version() == cpu_ops.lib.htn_abi_version() == abi.ABI_VERSION
    assert hip.htn_mps_bond_size.restype is C.c_int64
