"""Two-site energy variance (htn_mps_variance / api.energy_variance) on the CPU baseline library: the driver, the item lists and
the host default of the projection (Backend::block_nullproj in htn_backend_host.cpp) are the product's own host code; the
H_eff applies and the bond moves run on that library's host kernels.  The bodies are in variance_common.py."""
import pytest

import variance_common as vc
from cpu_ops import CpuOps
from hubbardtn_amd import abi


@pytest.fixture(scope="module")
def cpu_ops():
    return CpuOps()


@pytest.mark.parametrize("kind", vc.KINDS)
def test_variance_is_exact_for_a_nearest_neighbour_mpo(cpu_ops, kind):
    """L = 6, U = 4, t = [1], grown by two-site sweeps, cut to truncdim(8): total = dense ||(H - E) psi||^2 and energy =
    <psi|H|psi> within max(10 x 1.3e-16, 1e-12 ||H||^2), with the centre on site 0, 3 and 5.  Measured on this library:
    max |total - dense| = 1.3e-16 (variance_common.EXACT_CPU_DEV)."""
    dev = vc.check_exact(cpu_ops, kind)
    assert dev <= 10.0 * vc.EXACT_CPU_DEV or dev <= vc.bar_of(kind, (1.0,))


@pytest.mark.parametrize("kind", vc.KINDS)
def test_variance_is_a_lower_bound_for_an_mpo_of_range_two(cpu_ops, kind):
    vc.check_lower_bound(cpu_ops, kind)


@pytest.mark.parametrize("kind", vc.KINDS)
def test_variance_of_a_converged_eigenstate(cpu_ops, kind):
    vc.check_eigenstate(cpu_ops, kind)


def test_state_is_untouched_and_the_second_call_repeats_the_first(cpu_ops):
    vc.check_untouched(cpu_ops)


def test_sweep_after_the_call_plans_what_it_planned_without_it(cpu_ops):
    vc.check_cache_hygiene(cpu_ops)


@pytest.mark.parametrize("kind", ("SU2U1", "U1U1"))
def test_applied_state_reports_the_variance_of_the_normalised_state(cpu_ops, kind):
    vc.check_applied(cpu_ops, kind)


def test_refusals_and_another_hamiltonian(cpu_ops):
    vc.check_refusals(cpu_ops, CpuOps)


def test_extrapolate_energy():
    vc.check_extrapolate()


def test_host_default_of_the_projection_against_numpy(cpu_ops):
    vc.check_kernel(vc.cpu_run(cpu_ops.lib))
    vc.check_kernel_leak(vc.cpu_run(cpu_ops.lib))


def test_abi_structs_and_exports(cpu_ops):
    assert abi.NULLPROJ_DT.itemsize == 64 and abi.NULLPROJ_DT.fields["side"][1] == 36 and abi.NULLPROJ_DT.fields["out"][1] == 40
    for n in ("htn_mps_variance", "htn_block_nullproj_z"):
        assert hasattr(cpu_ops.lib, n) and n in abi.ENGINE_EXPORTS, n
    assert abi.nullproj_units(33, 17, 0) == 2 and abi.nullproj_units(33, 17, 1) == 3 and abi.nullproj_units(0, 5, 0) == 0
