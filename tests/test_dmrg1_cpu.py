"""One-site DMRG at fixed bond tables on the CPU baseline library (the product's planner and driver, host kernels; the gauge
move is htn::Backend::qr_blocks' host default, Householder reflections): the one-site effective Hamiltonian, convergence to
exact diagonalisation, the invariants of the state after a sweep, polishing of a truncated state, the refused
combinations, and the host QR / LQ itself on the matrix cases of the GPU kernel test."""
import ctypes as C

import numpy as np
import pytest

import dmrg1_common as d1
import excited_common as xc
import qr_cases as qc
from cpu_ops import CpuOps
from hubbardtn_amd import abi, api, engine, models, mps


@pytest.fixture(scope="module")
def cpu_ops():
    return CpuOps()


def _range2(L):
    return models.hamiltonian(models.OB_Sim([1.0, 0.3], [4.0, 0.5]), L)


@pytest.mark.parametrize("case", d1.SYMS + ["range2"])
def test_heff1_is_hermitian_and_carries_the_energy(cpu_ops, case):
    """centre moved to the middle of an L = 8 chain: H_eff^1 Hermitian on random x, y to 1e-13 ||H|| |x| |y| (||H|| bounded
    below by |H x| / |x|), <c|H_eff^1|c> = <psi|H|psi> to 1e-12, |c| = 1 -- in the stored right layout, and after a one-site
    update without a move in place"""
    L = 8
    e = d1.loose_state(cpu_ops, "SU2U1", H=_range2(L)) if case == "range2" else d1.loose_state(cpu_ops, case)
    E = e.bond_energies()[0]
    for i in range(L // 2):
        e.update_bond(i, +1, "right", optimise=False, record=False, cutoff=0.0)
    i = L // 2
    assert e.centre() == i
    c = e.site_vector(i)
    n = c.size
    rng = np.random.default_rng(7)
    x = rng.normal(size=n) + 1j * rng.normal(size=n)
    y = rng.normal(size=n) + 1j * rng.normal(size=n)
    Hx, Hy = e.apply_heff1(i, x), e.apply_heff1(i, y)
    hnorm = max(np.linalg.norm(Hx) / np.linalg.norm(x), np.linalg.norm(Hy) / np.linalg.norm(y))
    herm = abs(np.vdot(x, Hy) - np.conj(np.vdot(y, Hx)))
    Ec = np.vdot(c, e.apply_heff1(i, c))
    print(case, "n", n, "herm", herm, "scale", hnorm * np.linalg.norm(x) * np.linalg.norm(y), "E", E, "<c|H|c>", Ec,
          "|c|", np.linalg.norm(c))
    assert herm <= 1e-13 * hnorm * np.linalg.norm(x) * np.linalg.norm(y)
    assert abs(Ec - E) <= 1e-12 * max(abs(E), 1.0)
    assert abs(np.linalg.norm(c) - 1.0) <= 1e-12
    E0 = e.update_site(i, 0, optimise=False, record=False)          # expectation value only: the state does not move
    assert abs(E0 - E) <= 1e-12 * max(abs(E), 1.0) and e.centre() == i


@pytest.mark.parametrize("symname", d1.SYMS)
def test_one_site_sweeps_converge_to_exact_diagonalisation(cpu_ops, symname):
    """L = 8 untruncated, from a state after ONE loose two-site sweep: every Ritz value <= the previous one + 1e-12, the
    final energy = ED to 1e-10; afterwards the bond tables are unchanged, every left / right tensor is orthonormal to
    1e-12, the centre is on site 0 and bond_energies() (a genuine expectation value) equals the last Ritz value to 1e-10"""
    e = d1.loose_state(cpu_ops, symname)
    before = d1.tables(e)
    E, ritz = d1.converge_onesite(e)
    ref = d1.ed_energy(symname)
    print(symname, "E", repr(E), "ED", repr(ref), "diff", abs(E - ref), "updates", len(ritz))
    assert all(b <= a + 1e-12 for a, b in zip(ritz, ritz[1:])), "a Ritz value rose"
    assert abs(E - ref) <= 1e-10
    assert d1.tables(e) == before
    assert e.centre() == 0
    assert d1.isometry_defects(e) <= 1e-12
    assert abs(e.bond_energies()[0] - ritz[-1]) <= 1e-10


def test_polishing_a_truncated_state(cpu_ops):
    """L = 16, U = 4: two-site sweeps at truncdim 48 (they truncate and converge on the CPU library), then one-site sweeps at
    those tables: E_one-site <= <psi|H|psi> of the stored truncated state + 1e-12 and >= the two-site energy at truncdim 200.
    (An untruncated L = 16 run, bonds of dimension 4^8, is out of reach of a quick test; the run at 200 is variational, so its
    energy lies ABOVE the untruncated one and the assertion asks more, not less.)"""
    L = 16
    H = models.hamiltonian(models.OB_Sim([1.0], [4.0]), L)
    bonds, tens = mps.random_mps(L, (L, 0), 6, seed=5)
    e = engine.DMRG2(cpu_ops, H, bonds, tens, chi_full=48, krylovdim=20)
    for _ in range(4):
        e.sweep()
    assert sum(s.trunc_weight for s in e.stats[-(2 * L - 3):]) > 0.0, "the run must truncate"
    E_stored = e.bond_energies()[0]
    E1, ritz = d1.converge_onesite(e)
    full = engine.DMRG2(cpu_ops, H, bonds, tens, chi_full=200, krylovdim=20)
    for _ in range(3):
        E_full = full.sweep()
    print("stored", repr(E_stored), "one-site", repr(E1), "two-site at 200", repr(E_full))
    assert E1 <= E_stored + 1e-12
    assert E1 >= E_full - 1e-10
    assert all(b <= a + 1e-12 for a, b in zip(ritz, ritz[1:]))


def test_truncstate_with_one_site_polish(cpu_ops, monkeypatch):
    """TruncState(polish="onesite") returns an energy <= that of scheme 1 (SVD cut only) at the same dimension; the API's
    DMRG() selector runs one-site sweeps through find_groundstate"""
    monkeypatch.setattr(api, "_ops", lambda device=0: cpu_ops)
    sim = models.OB_Sim([1.0], [4.0], 0.0, 1, 1, 2.0, 8)
    cut = api.TruncState(sim, 24, trunc_scheme=1, L=8, maxiter=6)
    pol = api.TruncState(sim, 24, trunc_scheme=0, L=8, polish="onesite", maxiter=6)
    E_cut = cut["ψ_trunc"].engine.bond_energies()[0]
    E_pol = pol["ψ_trunc"].engine.bond_energies()[0]
    print("svd cut", repr(E_cut), "one-site polish", repr(E_pol))
    assert E_pol <= E_cut + 1e-12
    psi, envs, delta = api.find_groundstate(pol["ψ_trunc"], None, api.DMRG(tol=1e-10, maxiter=4))
    assert delta < 1e-8 and psi.engine.centre() == 0
    with pytest.raises(ValueError):
        api.TruncState(sim, 24, L=8, polish="threesite")


def test_refused_calls_say_why(cpu_ops):
    L = 8
    e = d1.loose_state(cpu_ops, "SU2U1")
    with pytest.raises(abi.HtnError, match="centre is on site 0"):
        e.update_site(3, +1)
    other = d1.loose_state(cpu_ops, "SU2U1", seed=9)
    e.set_orthogonal([other])
    with pytest.raises(abi.HtnError, match="attached orthogonal states"):
        e.sweep1()
    e.set_orthogonal([])
    # a context with an exchange hook (the rehearsal stand-in for a communicator)
    ops2 = CpuOps()
    ops2.set_exchange(0, 2, lambda y: None)
    sym, H, target = xc.model("SU2U1", L)
    b, t = mps.random_mps(L, target, 6, seed=3, sym=sym)
    e2 = engine.DMRG2(ops2, H, b, t)
    with pytest.raises(abi.HtnError, match="communicator"):
        e2.update_site(0, +1)
    # a block with fewer rows than columns, built by hand: bond 1 wider than site 0 can support
    bonds = [{(0, 0): 1}, {(1, 1): 3}, {(2, 0): 1}]
    tens = [{((0, 0), 1, (1, 1)): np.ones((1, 3)) / np.sqrt(3)}, {((1, 1), 1, (2, 0)): np.eye(3, 1) * np.sqrt(1.0)}]
    H2 = models.hamiltonian(models.OB_Sim([1.0], [4.0]), 2)
    e3 = engine.DMRG2(cpu_ops, H2, bonds, tens)
    with pytest.raises(abi.HtnError, match="run a two-site sweep first"):
        e3.update_site(0, +1)


def test_gauge_moves_on_tall_blocks_keep_the_state(cpu_ops):
    """tall_state's L = 14 chain at its cap of 150 per sector (the largest factorised block has m = 600 rows: the GPU kernel's
    panel width 8): the centre goes from site I0 to the right end and back to site 0 by update_site(optimise=False).  Every
    returned <x|H_eff|x> equals the first to 1e-11 relative, the left isometries at the turning point and the right ones at
    the end are orthonormal to 1e-12, and |<moved|untouched twin>| = 1 to 1e-12."""
    d1.assert_tall_gauge_round_trip(cpu_ops)


CASES = qc.cases()


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_qr_blocks_on_the_kernel_cases(cpu_ops, name, trans):
    """htn_qr_blocks_z of the CPU library (host memory, Householder): same cases, bars and sign rule as the GPU kernel, the
    same exact zeros on R's diagonal at planted dependent columns, and on an R buffer full of a sentinel the same written
    zero triangle and untouched padding (qc.check_padding)"""
    mats = CASES[name]
    flat, desc, rsize = qc.pack(mats, trans)
    R = np.full(rsize, qc.R_SENTINEL)
    cpu_ops.lib.htn_qr_blocks_z.argtypes = [C.c_void_p] * 4 + [C.c_int32, C.c_void_p]
    rc = cpu_ops.lib.htn_qr_blocks_z(flat.ctypes.data, R.ctypes.data, desc.ctypes.data, desc.ctypes.data, len(mats), None)
    assert rc == 0, cpu_ops.lib.htn_last_error()
    qc.check(name, trans, mats, flat, R, desc, well_conditioned_orth_bar=qc.orth_bar(name, mats))
