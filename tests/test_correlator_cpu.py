"""Two-point correlation functions (htn_mps_correlator / engine.DMRG2.correlator / api.correlation_function) on the CPU
baseline library: the driver, the probe plans and the block weight are the product's own host code (htn_correlator.cpp,
htn_plan.cpp); only the trace-dot kernel is the host default.  References: exact diagonalisation with the operators applied to
the ED vector by bit operations, dense ED, exact sum rules."""
import ctypes

import numpy as np
import pytest

import correlator_common as cc
from cpu_ops import CpuOps
from hubbardtn_amd import abi, api, engine, models, mps


@pytest.fixture(scope="module")
def cpu_ops():
    return CpuOps()


@pytest.fixture(scope="module")
def ed_ref():
    return {case: cc.ed_correlators(cc.ED_L, *cc.ED_CASES[case]) for case in cc.ED_CASES}


@pytest.mark.parametrize("case", list(cc.ED_CASES))
def test_all_kinds_against_exact_diagonalisation(cpu_ops, ed_ref, case):
    """L = 6, t = 1, U = 4 at half filling, and U = 4, u[1] = 1 at N = 4; full bond dimension; full L x L matrices, 1e-8"""
    E0, ref = ed_ref[case]
    eng = cc.ed_engine(cpu_ops, case)
    assert abs(eng.energy - E0) < 1e-9
    cc.compare_with_ed(eng, ref)


@pytest.mark.parametrize("case", list(cc.ED_CASES))
def test_spinful_mode_channels_against_the_su2_result_and_ed(cpu_ops, ed_ref, case):
    E0, ref = ed_ref[case]
    su = cc.ed_engine(cpu_ops, case)
    ab = cc.ed_engine(cpu_ops, case, spin=True)
    assert abs(ab.energy - E0) < 1e-9
    cc.compare_with_ed(ab, ref, kinds=cc.KINDS + ("hop_up", "hop_dn", "szsz", "s+-", "s-+"))
    hop = ab.correlator("hop_up") + ab.correlator("hop_dn")
    ss = ab.correlator("szsz") + 0.5 * (ab.correlator("s+-") + ab.correlator("s-+"))
    d_hop, d_ss = np.abs(hop - su.correlator("hop")).max(), np.abs(ss - su.correlator("ss")).max()
    print("spinful vs SU(2)", d_hop, d_ss)
    assert d_hop <= 1e-8 and d_ss <= 1e-8
    assert np.abs(ab.correlator("hop") - hop).max() <= 1e-12 and np.abs(ab.correlator("ss") - ss).max() <= 1e-12
    conn = ab.correlator("szsz", connected=True)
    assert np.abs(conn - ref["szsz"]).max() <= 1e-8             # <sz_i> = 0 in an S = 0 state


def test_parity_only_mode_against_dense_ed(cpu_ops):
    """fZ2 x SU(2) labels (chemical-potential model): the level charges dN = +-1, +-2 are wrapped modulo 2"""
    L, t, u, mu = 4, [1.0], [4.0], 1.7
    E0, ref = cc.dense_parity_reference(L, t, u, mu)
    H = models.hamiltonian(models.OBC_Sim2(t, u, mu), L)
    bonds, tens = mps.random_mps(L, (0, 0), 400, seed=3, sym=H.sym)
    eng = engine.DMRG2(cpu_ops, H, bonds, tens, chi_full=None, lanczos_tol=1e-13)
    for _ in range(6):
        E = eng.sweep()
    assert abs(E - E0) < 1e-9
    cc.compare_with_ed(eng, ref, kinds=("nn", "ss"))
    n = np.real(np.diag(eng.correlator("hop")))
    assert np.abs(eng.correlator("nn", connected=True) - (ref["nn"] - np.outer(n, n))).max() <= 1e-8


def test_sum_rules_on_a_random_unoptimised_state(cpu_ops):
    cc.check_sum_rules(cpu_ops, L=10, cap=12)


def test_gauge_independence_read_only_and_plan_cache_keys(cpu_ops):
    cc.check_gauge_and_readonly(cpu_ops)


def test_error_paths(cpu_ops):
    eng = cc.ed_engine(cpu_ops, "half")
    with pytest.raises(abi.HtnError, match="do not add up to zero"):
        eng.correlator_channel("cdagF", "F", "cdag")
    with pytest.raises(abi.HtnError, match="do not add up to zero"):
        eng.correlator_channel("S", "id", "n")
    with pytest.raises(abi.HtnError, match="pass operator carries a charge"):
        eng.correlator_channel("cdagF", "c", "c")
    with pytest.raises(ValueError):
        eng.correlator("hop_up")                                 # single spin channels exist in the spinful mode only
    with pytest.raises(ValueError):
        eng.correlator("hop", connected=True)
    hooked = CpuOps()
    hooked.set_exchange(0, 1, lambda y: None)
    H = models.hamiltonian(models.OB_Sim([1.0], [4.0]), 4)
    bonds, tens = mps.random_mps(4, (4, 0), 8, seed=2)
    e2 = engine.DMRG2(hooked, H, bonds, tens)
    with pytest.raises(abi.HtnError, match="communicator or an exchange hook"):
        e2.correlator("nn")
    with pytest.raises(NotImplementedError, match="chain length"):
        api.correlation_function(api.InfiniteMPS(8), "hop")


def test_api_structure_factor_and_momentum_distribution(cpu_ops):
    eng = cc.ed_engine(cpu_ops, "doped")
    psi = api.FiniteMPS(eng, eng.L)
    L = eng.L
    G = api.correlation_function(psi, "hop")
    assert np.array_equal(G, eng.correlator("hop"))
    q = np.linspace(-np.pi, np.pi, 7)
    ph = np.exp(1j * np.outer(q, np.arange(L)))
    ref = np.array([ph[k] @ G @ ph[k].conj() for k in range(len(q))]) / L
    assert np.abs(api.structure_factor(psi, "hop", q, connected=False) - ref).max() <= 1e-13
    assert np.abs(api.momentum_distribution(psi, q) - ref.real / 2).max() <= 1e-13
    assert abs(api.momentum_distribution(psi, 0.3) - api.momentum_distribution(psi, np.array([0.3]))[0]) <= 1e-15
    # q = 0: the connected density structure factor is the particle-number variance, zero in a U(1) sector
    assert abs(api.structure_factor(psi, "nn", 0.0)) <= 1e-9


def test_abi_structs_and_exports(cpu_ops):
    assert ctypes.sizeof(abi.TrdotItem) == 64 and abi.TRDOT_DT.itemsize == 64
    assert ctypes.sizeof(abi.CorrChannel) == 4 * ctypes.sizeof(abi.SiteOp) + 8 == 552      # four htn_site_op + two int32
    assert abi.TRDOT_DT.fields["w_re"][1] == 48 and abi.TrdotItem.w_re.offset == 48
    assert hasattr(cpu_ops.lib, "htn_mps_correlator")
    hip = abi.load_library()
    for n in ("htn_mps_correlator", "htn_block_trdots_z", "htn_trdots_scratch_elems"):
        assert hasattr(hip, n), n
    assert "htn_mps_correlator" in abi.ENGINE_EXPORTS and "htn_block_trdots_z" in abi.EXPORTS
