"""Bond-operator correlators on the device: the HIP library against the CPU baseline library and against exact diagonalisation,
blocks beyond one tile of the trace-dot / grouped-GEMM kernels, repeatability and read-only behaviour."""
import numpy as np
import pytest

import bondcorr_common as bc
from cpu_ops import CpuOps
from hubbardtn_amd import engine, models, mps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cpu_ops():
    return CpuOps()


@pytest.fixture(scope="module")
def ed_ref():
    return bc.ed_reference(*bc.CASES["L6"][:5])


@pytest.mark.parametrize("mode", bc.MODES)
def test_hip_against_cpu_library_and_ed(hip_ops, cpu_ops, ed_ref, mode):
    """L = 6 of every mode: the same converged run on both libraries, every kind within 1e-8 (the tolerance of the GPU two-point
    test against ED), and the device result within the same of ED"""
    E0, corr, mean = ed_ref
    dev, host = bc.converged_engine(hip_ops, "L6", mode), bc.converged_engine(cpu_ops, "L6", mode)
    bc.compare_with_ed(dev, corr, bc.kinds_of(mode))
    for k in bc.kinds_of(mode):
        d = float(np.abs(dev.bond_correlator(k) - host.bond_correlator(k)).max())
        print("HIP vs CPU library", mode, k, d)
        assert d <= bc.TOL_ED, (k, d)


def test_blocks_beyond_one_tile(hip_ops, cpu_ops):
    """L = 8, U / t = 4, spinful mode, two sweeps at truncdim 240 of 256: the (N = 4, Sz = 0) sector of the middle bond keeps more
    than 32 states, more than one 32 x 32 tile of the trace-dot kernel and no multiple of it.  The state is optimised on the CPU
    baseline library and its tensors are handed to the device as they are: rounding is the only difference, so the bound is
    that of the sum-rule test of the two-point pass, 1e-12 L^2 (tighter than the 1e-8 of the comparison above)."""
    L, chi = 8, 240
    H = models.hamiltonian(models.OB_Sim([1.0], [4.0], 0.0, 1, 1, 2.0, 50, spin=True), L)
    bonds, tens = mps.random_mps(L, (L, 0), 40, seed=21, sym=H.sym)
    host = engine.DMRG2(cpu_ops, H, bonds, tens, chi_full=chi, lanczos_tol=1e-10)
    for _ in range(2):
        host.sweep()
    bonds = [dict(b.dims) for b in host.bonds]
    biggest = max(max(b.values()) for b in bonds)
    print("largest sector block", biggest, "bond dimensions", host.bond_dims())
    assert biggest > 32 and biggest % 32 != 0 and max(host.bond_dims()) <= chi < 256
    dev = engine.DMRG2(hip_ops, H, bonds, [host.download_site(i) for i in range(L)], chi_full=chi)
    tol = 1e-12 * L * L
    for k in ("bond", "dimer", "spair", "bond_up", "dimer_xy"):
        A, B = dev.bond_correlator(k), host.bond_correlator(k)
        d = float(np.abs(A - B).max())
        print("truncated state, HIP vs CPU library", k, d, "scale", float(np.abs(B).max()), "tol", tol)
        assert d <= tol, (k, d)


def test_repeatable_read_only_and_two_point_unchanged(hip_ops):
    eng = bc.converged_engine(hip_ops, "L6", "su2")
    eng.move_centre(eng.L // 2)
    hop_before = eng.correlator("hop")
    before = [eng.site_vector(i).copy() for i in range(eng.L)]
    ref = {k: eng.bond_correlator(k) for k in bc.SU2_KINDS}
    for k, r in ref.items():
        assert np.array_equal(eng.bond_correlator(k), r), k
    for i in range(eng.L):
        assert np.array_equal(eng.site_vector(i), before[i]), i
    assert eng.centre() == eng.L // 2
    assert np.array_equal(eng.correlator("hop"), hop_before)      # the probe plans of the two entries do not replace each other


def test_centre_independence_and_site_tensors_unchanged(hip_ops):
    """L = 6, SU(2): the re-lay path of both passes of htn_mps_correlator2, centre in the middle and on the last site"""
    eng = bc.converged_engine(hip_ops, "L6", "su2")
    ref = {k: eng.bond_correlator(k) for k in bc.SU2_KINDS}       # centre on site 0
    bc.check_centre_independence(eng, ref, (eng.L // 2, eng.L - 1))


def test_repeated_calls_plan_nothing(hip_ops):
    bc.check_repeated_calls_plan_nothing(bc.converged_engine(hip_ops, "L6", "su2"))
