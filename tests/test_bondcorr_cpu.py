"""Bond-operator correlators (htn_mps_correlator2 / engine.DMRG2.bond_correlator / api.bond_correlation_function) on the CPU
baseline library: the driver, the probe plans and the block weight are the product's own host code (htn_correlator.cpp,
htn_plan.cpp).  References: exact diagonalisation with explicitly built operator strings, Wick's theorem on a free-fermion
state, structural identities."""
import ctypes

import numpy as np
import pytest

import bondcorr_common as bc
import correlator_common as cc
from cpu_ops import CpuOps
from hubbardtn_amd import abi, api, bondcorr, engine, idmrg, models, mps
from oracle import ed


@pytest.fixture(scope="module")
def cpu_ops():
    return CpuOps()


@pytest.fixture(scope="module")
def ed_ref():
    return {case: bc.ed_reference(*bc.CASES[case][:5]) for case in bc.CASES}


@pytest.fixture(scope="module")
def engines(cpu_ops):
    return {(case, mode): bc.converged_engine(cpu_ops, case, mode) for case in bc.CASES for mode in bc.MODES}


@pytest.mark.parametrize("mode", bc.MODES)
@pytest.mark.parametrize("case", list(bc.CASES))
def test_all_kinds_against_exact_diagonalisation(engines, ed_ref, case, mode):
    """L = 6 (t = 1, t' = 0.5, U = 4, half filling) and L = 4, full bond dimension, every entry of every kind -- the same bond
    twice, bonds that share a site, disjoint bonds -- within 1e-8 of ED, the tolerance of the two-point tests"""
    L, t, u, nu, nd, mu = bc.CASES[case]
    E0, corr, mean = ed_ref[case]
    eng = engines[case, mode]
    assert abs(eng.energy - (E0 - (mu * (nu + nd) if mode == "su2p" else 0.0))) < 1e-9
    bc.compare_with_ed(eng, corr, bc.kinds_of(mode))
    for k in bc.kinds_of(mode):
        if k == "spair":
            continue
        d = float(np.abs(eng.bond_expectation(k) - mean[k]).max())
        dc = float(np.abs(eng.bond_correlator(k, connected=True) - (corr[k] - np.outer(mean[k], mean[k]))).max())
        print("bond expectation", k, d, "connected", dc)
        assert d <= bc.TOL_ED and dc <= bc.TOL_ED


def test_wick_contractions_of_a_free_fermion_state(cpu_ops):
    """U = 0, half filling: <B_i B_j> and <Delta+_i Delta_j> against Wick's theorem.
    Untruncated L = 6, Wick applied to correlator("hop") of the SAME state: a Slater determinant to rounding; measured deviations
    3.2e-15 (bond), 6.3e-15 (spair); the bound is 1e-10 as for every rounding-limited comparison of converged states here.
    L = 12, truncdim 256 (the untruncated middle bond has dimension 2568): the state is not a determinant.  The bound comes from the
    reference's own error, the energy of the state above the exact free-fermion energy, dE (measured: 4.9e-10): with
    gap = 4 sin(pi / 26) = 0.482, the lowest excitation inside the sector (N, S = 0), the infidelity is 1 - F <= dE / gap, and an
    expectation value differs from the ground state's by at most 2 |O| eta, eta = sqrt(1 - F) (trace distance of two pure states).
      (a) against the closed form (Wick on the exact G): |B_i| = 2, so |B_i B_j| <= 4: 8 eta = 2.6e-4; |Delta_i| = 1: 2 eta = 6.4e-5.
          Measured: 1.4e-6 (bond), 9.4e-7 (spair).  The connected parts of <B_i B_j> are 1e-2 .. 1e-1: an error in them fails.
      (b) against Wick on correlator("hop") of the same state, as the two routes would be compared on any state: G moves by
          at most 2 |E_ab| eta = 4 eta, each of the four terms G_ab G_cd + 2 g_ad (delta_bc - g_cb) by at most 16 eta + 8 eta, plus the
          direct 8 eta: 104 eta = 3.3e-3 (bond); 2 eta + 2 (2 eta + 2 eta) = 10 eta (spair).  Measured: 1.4e-6, 9.3e-7.
    Both bounds are worst cases over all states of that energy; they hold for any correct implementation."""
    eng6, E6 = bc.free_fermion_engine(cpu_ops, 6, None)
    dev6 = bc.wick_deviations(eng6)
    print("L = 6 untruncated: energy error", abs(E6 - ed.free_fermion_energy(6, 3, 3)), "Wick deviations", dev6)
    assert max(dev6.values()) <= 1e-10
    L = 12
    eng, E = bc.free_fermion_engine(cpu_ops, L, 256, sweeps=6)
    dE = E - ed.free_fermion_energy(L, L // 2, L // 2)
    eta = np.sqrt(max(dE, 0.0) / (4.0 * np.sin(np.pi / 26.0)))
    G0 = cc.free_fermion_G(L, L)
    closed = {"bond": float(np.abs(eng.bond_correlator("bond") - bc.wick_bond(G0)).max()),
              "spair": float(np.abs(eng.bond_correlator("spair") - bc.wick_spair(G0)).max())}
    same = bc.wick_deviations(eng)
    print("L = 12 truncdim 256: dE", dE, "eta", eta, "against the closed form", closed, "bounds", 8 * eta, 2 * eta,
          "against Wick on the same state", same, "bounds", 104 * eta, 10 * eta, "bond dimensions", eng.bond_dims())
    assert -1e-10 <= dE <= 1e-8                                   # truncated, and close enough for the bounds to mean something
    assert closed["bond"] <= 8.0 * eta + 1e-10 and closed["spair"] <= 2.0 * eta + 1e-10
    assert same["bond"] <= 104.0 * eta + 1e-10 and same["spair"] <= 10.0 * eta + 1e-10


def test_gram_matrix_raw_diagonal_and_su2_equals_spinful(engines):
    """<O+_i O_j> is a Gram matrix: positive semidefinite (the entries of identical, adjacent and disjoint bonds come from three
    different sets of strings; a wrong relative factor shows here).  The matrix is Hermitian by construction, so what is checked
    is the raw diagonal before its imaginary part is dropped."""
    for case in bc.CASES:
        su, ab = engines[case, "su2"], engines[case, "u1"]
        for k in bc.SU2_KINDS:
            A, B = su.bond_correlator(k), ab.bond_correlator(k)
            assert A.shape == (su.L - 1, su.L - 1)
            for e, M in ((su, A), (ab, B)):
                raw = np.diag(e._string_values(bondcorr.strings(e.sym, k)[0], 2), 1)
                assert np.abs(raw.imag).max() <= 1e-14 and np.abs(raw.real - np.real(np.diag(M))).max() <= 1e-14
                w = np.linalg.eigvalsh(M)
                print("Gram matrix", case, k, "lowest eigenvalue", float(w.min()))
                assert w.min() >= -1e-12
            d = float(np.abs(A - B).max())
            print("SU(2) vs spinful", case, k, d)
            assert d <= bc.TOL_ED
        for k in ("bond", "dimer"):
            assert np.abs(engines[case, "su2p"].bond_correlator(k) - su.bond_correlator(k)).max() <= bc.TOL_ED


@pytest.mark.parametrize("mode", bc.MODES)
def test_bond_order_sums_to_the_kinetic_energy(engines, mode):
    """nearest-neighbour model: H = -t sum_i B_i + U sum_i docc_i (- mu N): <B_i> from the two-site route of the diagonal"""
    L, t, u, nu, nd, mu = bc.CASES["L4"]
    eng = engines["L4", mode]
    docc = eng.site_expectation("docc")
    kin = eng.energy - u[0] * docc.sum() + (mu * (nu + nd) if mode == "su2p" else 0.0)
    got = -t[0] * eng.bond_expectation("bond").sum()
    print("kinetic energy", kin, got)
    assert abs(kin - got) <= bc.TOL_ED


def test_centre_independence_read_only_repeatable_and_cache_tags(cpu_ops):
    eng = bc.converged_engine(cpu_ops, "L6", "su2")
    fresh = bc.converged_engine(cpu_ops, "L6", "su2")
    L = eng.L
    hop_before = fresh.correlator("hop")                          # on an engine that has never run the new call
    ref = {k: eng.bond_correlator(k) for k in bc.SU2_KINDS}
    assert np.array_equal(eng.correlator("hop"), hop_before)      # the probe plans of the two entries do not replace each other
    for k, r in ref.items():
        assert np.array_equal(eng.bond_correlator(k), r), k       # repeated calls: bit-identical
    bc.check_centre_independence(eng, ref, (L // 2, L - 1, 0))
    assert np.abs(eng.correlator("hop") - hop_before).max() <= 1e-12


@pytest.mark.parametrize("mode", bc.MODES)
def test_repeated_calls_plan_nothing(cpu_ops, mode):
    bc.check_repeated_calls_plan_nothing(bc.converged_engine(cpu_ops, "L6", mode))


def test_error_paths(cpu_ops):
    eng = bc.converged_engine(cpu_ops, "L4", "su2")
    with pytest.raises(abi.HtnError, match="do not add up to zero"):
        eng.correlator2_channel(["cdagF", "cdag"], "id", ["Fc", "cdag"], (2, 0))
    with pytest.raises(abi.HtnError, match="do not add up to zero"):
        eng.correlator2_channel(["S", "S"], "id", ["n", "n"], (0, 2))          # rank 1 level closed by a scalar
    with pytest.raises(abi.HtnError, match="cannot couple to the level"):
        eng.correlator2_channel(["cdagF", "cdag"], "id", ["Fc", "c"], (2, 4))
    with pytest.raises(abi.HtnError, match="cannot couple to the level"):
        eng.correlator2_channel(["cdagF", "c"], "id", ["cdagF", "c"], (2, 0))
    with pytest.raises(abi.HtnError, match="pass operator carries a charge"):
        eng.correlator2_channel(["cdagF", "c"], "c", ["cdagF", "c"], (0, 0))
    with pytest.raises(ValueError):
        eng.correlator2_channel(["cdagF"], "id", ["c"], (1, 1))
    with pytest.raises(ValueError, match="not available"):
        eng.bond_correlator("bond_up")                           # single components exist in the spinful mode only
    with pytest.raises(ValueError, match="connected"):
        eng.bond_correlator("spair", connected=True)
    with pytest.raises(ValueError, match="not available"):
        bc.converged_engine(cpu_ops, "L4", "su2p").bond_correlator("spair")
    H3 = models.hamiltonian(models.OB_Sim([1.0], [4.0]), 3)
    b3, t3 = mps.random_mps(3, (3, 1), 8, seed=2)
    e3 = engine.DMRG2(cpu_ops, H3, b3, t3)
    with pytest.raises(abi.HtnError, match="3 sites, two disjoint bonds need at least 4"):
        e3.correlator2_channel(["cdagF", "c"], "id", ["cdagF", "c"], (0, 0))
    win = idmrg.idmrg2(cpu_ops, models.OB_Sim([1.0], [4.0]), chi_full=16, maxiter=2, driver="native").engine
    with pytest.raises(abi.HtnError, match="boundary environments"):
        win.correlator2_channel(["cdagF", "c"], "id", ["cdagF", "c"], (0, 0))
    hooked = CpuOps()
    hooked.set_exchange(0, 1, lambda y: None)
    H = models.hamiltonian(models.OB_Sim([1.0], [4.0]), 4)
    bonds, tens = mps.random_mps(4, (4, 0), 8, seed=2)
    e2 = engine.DMRG2(hooked, H, bonds, tens)
    with pytest.raises(abi.HtnError, match="communicator or an exchange hook"):
        e2.bond_correlator("dimer")
    with pytest.raises(NotImplementedError, match="chain length"):
        api.bond_correlation_function(api.InfiniteMPS(8), "bond")
    thermal = api.ThermalMPS(eng, eng.L, n_phys=eng.L // 2)
    with pytest.raises(NotImplementedError, match="two chain sites apart"):
        api.bond_correlation_function(thermal, "bond")


def test_api_functions_and_structure_factor(engines):
    eng = engines["L6", "su2"]
    psi = api.FiniteMPS(eng, eng.L)
    for k in bc.SU2_KINDS:
        assert np.array_equal(api.bond_correlation_function(psi, k), eng.bond_correlator(k))
    n = eng.L - 1
    q = np.linspace(-np.pi, np.pi, 7)
    ph = np.exp(1j * np.outer(q, np.arange(n)))
    for k, conn in (("bond", True), ("dimer", True), ("spair", False)):
        Cm = eng.bond_correlator(k, connected=conn)
        ref = np.array([ph[m] @ Cm @ ph[m].conj() for m in range(len(q))]) / n
        assert np.abs(api.bond_structure_factor(psi, k, q) - ref).max() <= 1e-13
    assert abs(api.bond_structure_factor(psi, "bond", 0.3) - api.bond_structure_factor(psi, "bond", np.array([0.3]))[0]) <= 1e-15
    # a structure factor of a Hermitian correlation matrix is real, and non-negative for <O+ O>
    assert np.all(np.real(api.bond_structure_factor(psi, "spair", q)) >= -1e-12)


def test_abi_struct_exports_and_tables(cpu_ops):
    assert ctypes.sizeof(abi.CorrChannel2) == 5 * ctypes.sizeof(abi.SiteOp) + 16 == 696      # five htn_site_op + four int32
    assert abi.CorrChannel2.open_dN.offset == 680 and abi.CorrChannel2.n_close.offset == 688
    assert hasattr(cpu_ops.lib, "htn_mps_correlator2") and hasattr(abi.load_library(), "htn_mps_correlator2")
    assert "htn_mps_correlator2" in abi.ENGINE_EXPORTS
    # the SU(2) table: the disjoint bond order is four strings, the shared-site products merge into fewer passes than strings
    same, shared, far = bondcorr.strings(models.SU2U1, "bond")
    assert len(far) == 4 and len(shared) < 9 and len(same) < 6
    assert len(bondcorr.strings(models.U1U1, "bond")[2]) == 16 and len(bondcorr.strings(models.U1U1, "dimer")[2]) == 9
