"""Shared by test_thermal_mirror_cpu.py / test_thermal_mirror_gpu.py: the bodies of the tests of the mirrored purification -- the rung
conjugation and models.purified_hamiltonian(..., "mirror") on the host, api.thermal_greens_function(..., ancilla="mirror") and
api.purification_defect on either library.  The reference is dense throughout (the ED apparatus of thermal_common / thermal_dyn_common,
the dense expansion of an MPO and of a state): never the CPU run, never the code under test."""
import numpy as np
import pytest

from hubbardtn_amd import api, engine, models, mps
import thermal_common as th
import thermal_dyn_common as td
from thermal_dyn_common import ANTICOMMUTATOR, OPS, PAIR, TIMES, c_ed, cooled, full   # noqa: F401

KRYLOV_TOL = 1e-12                     # tol of td.full() / th.untruncated()


# ---- (a) conjugation, host only ------------------------------------------------------------------------------------------------
# every case of thermal_common.COMBOS ("J" is t = [t1, t2], u = [U, V], J = [J1], mu = 2: all term kinds of OB_Sim but the assisted
# hopping); on top a case with the three-equal-index integral U13 (density-assisted hopping, whose conjugate is a sum of two named
# operators) in both fixed-filling kinds and a two-band MB_Sim (intra-cell terms: ancilla strings that cross one physical site)
def extra_simulations():
    t = np.array([[0.3, 1.1, -0.2, 0.0], [1.1, -0.1, 0.7, -0.3]])
    u = np.array([[5.0, 2.0, 0.4, 0.0], [2.0, 6.0, 0.6, 0.1]])
    Jm = np.array([[0.0, 0.2, 0.1, 0.0], [0.2, 0.0, 0.0, 0.05]])
    return {"U13": models.OB_Sim(th.T2, th.U2, 0.7, [0.5], 1, 1, U13=[0.2]),
            "U13_u1": models.OB_Sim(th.T2, th.U2, 0.7, [0.5], 1, 1, 2.0, 8, spin=True, U13=[0.2], JMs=(0.7, 0.4)),
            "two_band": models.MB_Sim(t, u, Jm, np.array([[0.0, 0.3], [0.1, 0.0]])),
            "two_band_p": models.MBC_Sim(t, u, Jm)}


def dense_pair(sim, L):
    """dense G ("mirror"), dense K x 1 ("idle") and |I> of one model (4^(2 L) square: made once per test, kept by no one)"""
    G, K = models.purified_hamiltonian(sim, L, ancilla="mirror"), models.purified_hamiltonian(sim, L, ancilla="idle")
    assert len(G) == len(K) and G.sym is K.sym
    bonds, tensors = mps.infinite_temperature_mps(len(G) // 2, G.sym)
    return th.dense_mpo(G), th.dense_mpo(K), th.dense_state(bonds, tensors, G.sym)


def check_conjugation(sim, L):
    Gd, Kd, I = dense_pair(sim, L)
    n = int(round(np.log(Gd.shape[0]) / np.log(4.0)))          # chain sites
    normK = np.linalg.norm(Kd) / np.sqrt(Kd.shape[0])          # Frobenius norm / sqrt(dim) <= |K|: the bounds below only get tighter
    r = np.linalg.norm(Gd @ I)
    print("conjugation: chain sites", n, "|G I|", r, "|K|", normK, "ratio", r / normK)
    assert abs(np.vdot(I, I) - 1.0) <= 1e-13
    assert r <= 1e-12 * normK
    assert np.abs(Gd - Gd.conj().T).max() == 0.0 or np.abs(Gd - Gd.conj().T).max() <= 1e-13 * normK     # Hermitian
    # the physical half of G is the idle MPO: what is left, -1 x K~, moves no physical site (its Jordan-Wigner strings cross
    # physical sites with F, which is diagonal), it is not zero, and it commutes with K x 1
    D = (Gd - Kd).reshape([4] * (2 * n))
    phys_out, anc_out = list(range(0, n, 2)), list(range(1, n, 2))
    D = D.transpose(phys_out + [n + p for p in phys_out] + anc_out + [n + a for a in anc_out])
    D = D.reshape(4 ** (n // 2), 4 ** (n // 2), -1)            # [physical out, physical in, ancillas]
    off = D[~np.eye(4 ** (n // 2), dtype=bool)]
    assert np.abs(off).max() <= 1e-13 * normK and np.abs(D).max() > 1e-2
    A, v = Gd - Kd, np.random.default_rng(5).standard_normal((Gd.shape[0], 4))      # [K x 1, 1 x K~] = 0, on four random vectors
    assert np.abs(Kd @ (A @ v) - A @ (Kd @ v)).max() <= 1e-12 * normK ** 2 * np.sqrt(Gd.shape[0])
    Kr = Kd.reshape([4] * (2 * n)).transpose(anc_out + [n + a for a in anc_out] + phys_out + [n + p for p in phys_out])
    Kr = Kr.reshape(4 ** (n // 2), 4 ** (n // 2), -1)          # the idle MPO moves no ancilla (as before)
    assert np.abs(Kr[~np.eye(4 ** (n // 2), dtype=bool)]).max() == 0.0


def body_conjugation(mode, case, L):
    check_conjugation(th.simulation(mode, case), L)


def body_conjugation_extra(name, L):
    check_conjugation(extra_simulations()[name], L)


def _dense_op(sym, op):
    return models._dense_components(sym, models._op_tuple(sym, op))


def body_rung_conjugate(mode):
    """the site-level statement: (O x 1)|rung> = (1 x O~)|rung> component by component for every named operator, O~ carries the
    charge and rank of O, conjugating twice gives O back up to the sign the rung's symmetry fixes, and (A B)~ = B~ A~"""
    sym = {"su2": models.SU2U1, "u1": models.U1U1, "p": models.SU2P}[mode]
    fn = {"su2": models.rung_conjugate_su2u1, "u1": models.rung_conjugate_u1u1, "p": models.rung_conjugate_su2p}[mode]
    bonds, tensors = mps.infinite_temperature_mps(1, sym)
    rung = th.dense_state(bonds, tensors, sym)                  # site 0 (physical) most significant
    assert np.abs(models.rung_matrix(sym).ravel() - rung).max() <= 1e-15
    conj = {}
    for name, O in sym.site_ops.items():
        k, dN, red = conj[name] = fn(O)
        assert (k, dN) == (O[0], O[1]) and red.shape == O[2].shape
        assert models.rung_conjugate(sym, name)[2].tolist() == red.tolist()
        for Oq, Cq in zip(_dense_op(sym, O), _dense_op(sym, conj[name])):
            assert np.abs(np.kron(Oq, np.eye(4)) @ rung - np.kron(np.eye(4), Cq) @ rung).max() <= 1e-14, name
        # twice: R^T = R F in the SU(2) kinds (the singlet is antisymmetric), R^T = R in the abelian one, so O~~ = F O F and O
        twice = -1.0 if sym.su2 and O[1] % 2 else 1.0
        assert np.abs(fn(conj[name])[2] - twice * O[2]).max() <= 1e-14, name
    assert np.abs(conj["n"][2] - (2.0 * sym.site_ops["id"][2] - sym.site_ops["n"][2])).max() <= 1e-14     # derived, not put in
    assert np.abs(conj["F"][2] - sym.site_ops["F"][2]).max() <= 1e-14
    # products of scalars with anything (reduced matrices multiply as matrices when one factor has rank 0)
    names = ("cdag", "c", "S", "pair_dag") if sym.su2 else ("cdag_up", "c_dn", "sp", "pair_dag")
    for a in ("n", "docc", "F"):
        for b in names:
            A, B = sym.site_ops[a], sym.site_ops[b]
            AB = (B[0], B[1], A[2] @ B[2])
            want = conj[b][2] @ conj[a][2]
            assert np.abs(fn(AB)[2] - want).max() <= 1e-14, (a, b)
    if not sym.su2:                                              # abelian kind: any two matrices
        A, B = sym.site_ops["cdag_up"], sym.site_ops["c_dn"]
        assert np.abs(fn((A[0] + B[0], A[1] + B[1], A[2] @ B[2]))[2] - conj["c_dn"][2] @ conj["cdag_up"][2]).max() <= 1e-14


def body_refusals_host():
    t = np.array([[0.3, 1.1, -0.2, 0.0], [1.1, -0.1, 0.7, -0.3]])
    u = np.array([[5.0, 2.0, 0.4, 0.0], [2.0, 6.0, 0.6, 0.1]])
    Jm = np.array([[0.0, 0.2, 0.1, 0.0], [0.2, 0.0, 0.0, 0.05]])
    for anc in ("idle", "mirror"):
        with pytest.raises(NotImplementedError, match="U112"):
            models.purified_hamiltonian(models.MB_Sim(t, u, Jm, U112={(1, 2, 3, 3): 0.2}), 3, ancilla=anc)
    with pytest.raises(ValueError, match="ancilla"):
        models.purified_hamiltonian(th.simulation("su2", "mu05"), 3, ancilla="both")
    sim = th.simulation("su2", "J")
    old, new = models.purified_hamiltonian(sim, 3), models.purified_hamiltonian(sim, 3, ancilla="idle")
    for a, b in zip(old, new):
        assert a.left == b.left and a.right == b.right and a.entries == b.entries


# ---- (b) stationarity --------------------------------------------------------------------------------------------------------------
def library_state(psi):
    """the state of a ThermalMPS as a dense vector (centre on site 0)"""
    eng = psi.engine
    return th.dense_state([dict(b.dims) for b in eng.bonds], [eng.download_site(i) for i in range(psi.L)], eng.sym)


def dense_thermal_state(sim, L, beta):
    """exp(-beta K' / 2)|I> normalised, K' the dense idle MPO, and the dense G"""
    Gd, Kd, I = dense_pair(sim, L)
    n = 2 * L
    phys, anc = list(range(0, n, 2)), list(range(1, n, 2))
    Kb = Kd.reshape([4] * (2 * n)).transpose(anc + [n + a for a in anc] + phys + [n + p for p in phys])
    Kb = Kb.reshape(4 ** L, 4 ** L, 4 ** L, 4 ** L)            # [ancillas out, ancillas in, physical out, physical in]
    Ib = I.reshape([4] * n).transpose(anc + phys).reshape(4 ** L, 4 ** L)
    out = np.zeros_like(Ib)
    for a in range(4 ** L):                                    # K x 1 moves no ancilla: one 4^L block per ancilla configuration
        w, v = np.linalg.eigh(Kb[a, a])
        out[a] = v @ (np.exp(-0.5 * beta * w) * (v.T @ Ib[a]))
    psi = out.reshape([4] * n).transpose(np.argsort(anc + phys)).reshape(-1)
    return psi / np.linalg.norm(psi), Gd


# L = 3, beta = 1 reached with dbeta = 0.05 and nothing truncated, then five tdvp_sweep(0.1) under G on a copy.  A state psi moves under
# exp(-i G t) by at most |G psi| t, so |<psi|copy> - 1| <= |G psi_lib| t with psi_lib the library's state expanded densely and G the
# dense mirror MPO.  Measured on the CPU baseline library over all COMBOS: |G psi_lib| <= 4.9e-11, psi_lib at a distance of
# at most 1.1e-11 from the dense exp(-beta K / 2)|I> -- what the cooling run's solves left -- so the first term is 2.5e-11 at t = 0.5.
# The solves add their tolerance each: 5 sweeps x (2 n - 2 bond steps + 2 n - 3 backward site steps) = 95 solves at n = 6 chain
# sites, 1e-12 each.  The test evaluates the first term on the state it has (capped at four times the figure above, the margin of
# the cooling tests), the second is fixed.  What the sweeps did on that library: |<psi|copy> - 1| <= 1.4e-15
STATIONARY_T, STATIONARY_SWEEPS = 0.5, 5
GPSI_MEASURED = 4.9e-11


def body_stationarity(ops, mode, case):
    L, beta = 3, 1.0
    sim = th.simulation(mode, case)
    psi = cooled(ops, mode, case, L, beta)
    exact, Gd = dense_thermal_state(sim, L, beta)
    lib = library_state(psi)
    assert abs(np.linalg.norm(lib) - 1.0) <= 1e-12
    dist = np.linalg.norm(lib - np.vdot(exact, lib) * exact)
    gpsi = float(np.linalg.norm(Gd @ lib))
    solves = STATIONARY_SWEEPS * (4 * psi.L - 5)
    bound = gpsi * STATIONARY_T + KRYLOV_TOL * solves
    assert np.linalg.norm(Gd @ exact) <= 1e-12 * np.linalg.norm(Gd) / np.sqrt(Gd.shape[0])        # (the dense statement G psi_beta = 0)
    assert gpsi <= 4.0 * GPSI_MEASURED, gpsi
    work = psi.engine.copy()
    work.lanczos_tol, work.chi_full, work.cutoff = KRYLOV_TOL, None, 0.0
    work.set_mpo(models.purified_hamiltonian(sim, L, ancilla="mirror"))
    worst = 0.0
    for _ in range(STATIONARY_SWEEPS):
        work.tdvp_sweep(STATIONARY_T / STATIONARY_SWEEPS)
        worst = max(worst, abs(psi.engine.overlap(work) - 1.0))
    print("RESULT stationarity", mode, case, "|G psi_lib|", gpsi, "distance from the dense state", dist, "bound", bound,
          "|<psi|copy> - 1|", worst)
    assert worst <= bound, (worst, bound)
    return gpsi


# ---- (c) C against ED ----------------------------------------------------------------------------------------------------------------
_RESULTS = {}


def mirror_result(ops, mode, case, L, beta, op, times=TIMES, alg=None):
    key = (id(ops), mode, case, L, beta, op, tuple(times))
    if key not in _RESULTS:
        _RESULTS[key] = api.thermal_greens_function(cooled(ops, mode, case, L, beta), times, alg or full(), op=op, ancilla="mirror")
    return _RESULTS[key]


def body_against_ed(ops, mode, case, beta):
    """beta = 1: the bound of the idle test of the same case (thermal_dyn_common.body_against_ed), four times its MEASURED.  beta = 0:
    the bound of the idle test of a state that was never cooled (body_beta0_dynamics at dt = 0.1), four times BETA0_MEASURED[0.1];
    that test runs one case, the bound is applied to all of them here.  The mirror scheme stays inside it: largest deviation over
    all COMBOS and OPS on the CPU baseline library 1.3e-6 at dt = 0.1 (idle: 5.7e-7; the seed sweeps act on one state only)"""
    L = 3
    tol = 4.0 * td.MEASURED if beta > 0.0 else 4.0 * td.BETA0_MEASURED[0.1]
    worst = 0.0
    for op in OPS[mode]:
        res = mirror_result(ops, mode, case, L, beta, op)
        assert res["C"].shape == (len(TIMES), L) and res["C"].dtype == np.complex128 and res["trunc_weight"].shape == (len(TIMES), 2)
        assert res["ancilla"] == "mirror" and res["site"] == L // 2 and res["beta"] == beta and res["op"] == op
        assert not res["trunc_weight"][:, 0].any() and res["trunc_weight"].max() <= 1e-20
        ref = c_ed(L, case, beta, op, L // 2)
        assert np.abs(ref[-1] - ref[0]).max() > 1e-2               # (the reference moves: no comparison of constants)
        d = float(np.abs(res["C"] - ref).max())
        print("RESULT mirror against ED", mode, case, "beta", beta, op, d)
        worst = max(worst, d)
    assert worst <= tol, (worst, tol)
    return worst


def body_against_ed_l4(ops):
    """L = 4, SU(2) x U(1), the case and the bound of the idle test thermal_dyn_common.body_splitting at dt = 0.1"""
    L, beta = 4, 1.0
    psi = cooled(ops, "su2", "mu05", L, beta)
    for site in (None,):
        res = api.thermal_greens_function(psi, TIMES, th.untruncated(), op="c+", site=site, ancilla="mirror")
        s = L // 2 if site is None else site
        d = float(np.abs(res["C"] - c_ed(L, "mu05", beta, "c+", s)).max())
        print("RESULT mirror against ED, L = 4, site", s, d)
        assert res["site"] == s and res["trunc_weight"].max() <= 1e-20
        assert d <= 4.0 * td.MEASURED_L4[0.1], d


def body_idle_unchanged(ops):
    """the default is the idle scheme, bit for bit, and says so"""
    psi = cooled(ops, "su2", "mu05", 3, 1.0)
    a = api.thermal_greens_function(psi, TIMES[:3], full(), op="c+")
    b = api.thermal_greens_function(psi, TIMES[:3], full(), op="c+", ancilla="idle")
    assert a["ancilla"] == b["ancilla"] == "idle" and a["trunc_weight"].shape == (3, 2)
    assert np.abs(a["C"] - b["C"]).max() <= 1e-13 and np.abs(a["C"] - c_ed(3, "mu05", 1.0, "c+", 1)[:3]).max() <= 4.0 * td.MEASURED
    with pytest.raises(ValueError, match="ancilla"):
        api.thermal_greens_function(psi, TIMES, full(), ancilla="backwards")
    with pytest.raises(TypeError, match="tables"):
        api.thermal_greens_function(psi, TIMES, api.TDVP(), ancilla="mirror")
    with pytest.raises(NotImplementedError, match="finite temperature"):
        api.energy_variance(psi)
    with pytest.raises(TypeError, match="ThermalMPS"):
        api.purification_defect(api.InfiniteMPS(8))


# ---- (d) cost and purity ---------------------------------------------------------------------------------------------------------------
def body_cost_and_purity(ops):
    sim = th.simulation("su2", "mu05")
    used, fresh, never = (api.thermal_state(sim, 3, ops=ops) for _ in range(3))
    for psi in (used, fresh):
        api.cool(psi, [0.5], th.untruncated(), dbeta=td.DBETA)
    engines, sweep = [], engine.DMRG2.tdvp_sweep

    def spy(self, dt):
        if not any(e is self for e in engines):
            engines.append(self)
        return sweep(self, dt)
    for psi, seeds in ((used, 0), (never, len(api.SEED_STEPS))):
        before = td.snapshot(psi)
        mpo, n_stats = psi.engine.cmpo, len(psi.engine.stats)
        del engines[:]
        engine.DMRG2.tdvp_sweep = spy
        try:
            res = api.thermal_greens_function(psi, TIMES, full(), op="c+", ancilla="mirror")
        finally:
            engine.DMRG2.tdvp_sweep = sweep
        assert len(engines) == 1 and engines[0] is not psi.engine            # one state is evolved: the ket
        records = len(engines[0].stats)
        assert records == (len(TIMES) - 1 + seeds) * (2 * psi.L - 2), records  # a sweep leaves 2 n - 2 bond records in the stats
        assert not res["trunc_weight"][:, 0].any()
        assert td.same(before, td.snapshot(psi))                               # every site tensor bit-identical
        assert psi.engine.cmpo is mpo and len(psi.engine.stats) == n_stats
        # (`transition` memoises its transfer plans on the bra's handle, as every measurement of psi does, under keys no sweep reads:
        # the hit / miss counters of psi move, the plans `cool` uses do not -- the continuation below is the check)
        assert psi.mirror is not None
    assert not never.seeded and never.beta == 0.0 and max(never.bond_dimensions()) == 4
    a = api.cool(used, [1.0], th.untruncated(), dbeta=td.DBETA)
    b = api.cool(fresh, [1.0], th.untruncated(), dbeta=td.DBETA)
    assert abs(a["energy"][0] - b["energy"][0]) <= 1e-10 and abs(used.log_z - fresh.log_z) <= 1e-10


# ---- (e) defect ----------------------------------------------------------------------------------------------------------------------------
def body_defect(ops):
    """only orderings: the two-site variance of G is a lower bound of |G psi|^2 = 4 (|G psi| t)^2 at t = 0.5, the value of (b) squared
    within the factor 10 allowed; truncation raises it"""
    psi = cooled(ops, "su2", "mu05", 3, 1.0)
    before = td.snapshot(psi)
    v = api.purification_defect(psi)
    assert td.same(before, td.snapshot(psi))
    _, Gd = dense_thermal_state(th.simulation("su2", "mu05"), 3, 1.0)
    value_b = float(np.linalg.norm(Gd @ library_state(psi))) * STATIONARY_T
    print("RESULT defect L = 3", v.total, "value of (b) squared", value_b ** 2, "<G>", v.energy)
    assert type(v) is engine.Variance and v.site.shape == (6,) and v.bond.shape == (5,)
    assert 0.0 <= v.total <= 10.0 * value_b ** 2 and abs(v.energy) <= 1e-10
    exact = cooled(ops, "su2", "mu05", 4, 1.0)
    cut = cooled(ops, "su2", "mu05", 4, 1.0, alg=api.TDVP2(trscheme=api.truncdim(16), tol=1e-10), tag="D16")
    d_exact, d_cut = api.purification_defect(exact).total, api.purification_defect(cut).total
    print("RESULT defect L = 4: untruncated", d_exact, "truncdim(16)", d_cut)
    assert d_cut > d_exact >= 0.0


# ---- (f) spectral sum rule --------------------------------------------------------------------------------------------------------------
def body_sum_rule(ops, mode, case):
    """the grid and the margin of thermal_dyn_common.body_spectral (its comment derives both): the rectangle rule over one period of the
    transform is exact, the weight is the anticommutator at equal time"""
    L, beta = 3, 1.0
    p, h = PAIR[mode]
    part, hole = mirror_result(ops, mode, case, L, beta, p), mirror_result(ops, mode, case, L, beta, h)
    dt, N, eta = TIMES[1] - TIMES[0], 64, 2.0
    grid = -np.pi / dt + (2.0 * np.pi / dt / N) * np.arange(N)
    weight = float(api.thermal_spectral_function(part, hole, 0.0, grid, eta).sum() * (2.0 * np.pi / dt / N))
    print("RESULT mirror sum rule", mode, case, weight - ANTICOMMUTATOR[mode])
    assert abs(weight - ANTICOMMUTATOR[mode]) <= 1e-11
    q, om = np.array([0.0, 0.7, np.pi]), np.linspace(-8.0, 8.0, 9)
    A = api.thermal_spectral_function(part, hole, q, om, eta)
    both = dict(part, C=c_ed(L, case, beta, p, L // 2) + np.conj(c_ed(L, case, beta, h, L // 2)))
    assert A.shape == (3, 9) and np.abs(A - api.spectral_function(both, q, om, eta)).max() <= 10.0 * 4.0 * td.MEASURED
