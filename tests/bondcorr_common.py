"""Shared by test_bondcorr_cpu.py / test_bondcorr_gpu.py: bond-operator correlators of exact-diagonalisation ground states
(explicit operator strings applied to the oracle's SectorED vector, correlator_common._apply), the converged DMRG runs of the
three symmetry modes they are compared with, and the Wick forms of a free-fermion state."""
import numpy as np

import correlator_common as cc
from hubbardtn_amd import engine, models, mps
from oracle import ed

SU2_KINDS = ("bond", "dimer", "spair")
U1_KINDS = SU2_KINDS + ("bond_up", "bond_dn", "dimer_zz", "dimer_xy")
TOL_ED = 1e-8                      # the tolerance of the two-point correlator tests against ED (correlator_common.compare_with_ed)
# (L, t, u, N_up, N_dn, mu of the no-U(1) run): nearest- and next-nearest-neighbour hopping, U / t = 4, half filling; the minimum chain
CASES = {"L6": (6, [1.0, 0.5], [4.0], 3, 3, 2.0), "L4": (4, [1.0], [4.0], 2, 2, 2.0)}
MODES = ("su2", "u1", "su2p")

cd = lambda i, s: (1, i, s)
c = lambda i, s: (0, i, s)


def _bond_strings(j):
    """Hermitian bond operators on (j, j+1) as [(factor, operator string)] of correlator_common._apply"""
    n_s = lambda i, s: [cd(i, s), c(i, s)]
    hop = lambda s: [(1.0, [cd(j, s), c(j + 1, s)]), (1.0, [cd(j + 1, s), c(j, s)])]
    sgn = lambda s: 0.5 if s == 0 else -0.5
    zz = [(sgn(s) * sgn(s2), n_s(j, s) + n_s(j + 1, s2)) for s in (0, 1) for s2 in (0, 1)]
    xy = [(0.5, [cd(j, 0), c(j, 1), cd(j + 1, 1), c(j + 1, 0)]), (0.5, [cd(j, 1), c(j, 0), cd(j + 1, 0), c(j + 1, 1)])]
    return {"bond": hop(0) + hop(1), "bond_up": hop(0), "bond_dn": hop(1), "dimer": zz + xy, "dimer_zz": zz, "dimer_xy": xy}


def ed_reference(L, t, u, n_up, n_dn, mu=0.0):
    """-> E0 (with -mu N), {kind: (L-1) x (L-1) matrix <O+_i O_j>}, {kind: <O_i>} on the ED ground state of the sector"""
    e = ed.SectorED(L, n_up, n_dn, t, u, mu)
    E0, psi = e.ground_state()
    psi = np.asarray(psi, dtype=float)
    corr, mean = {}, {}
    for kind in _bond_strings(0):
        v = [sum(f * cc._apply(e, psi, s) for f, s in _bond_strings(j)[kind]) for j in range(L - 1)]
        corr[kind] = np.array([[vi @ vj for vj in v] for vi in v])
        mean[kind] = np.array([psi @ vj for vj in v])
    # Delta_j = (c_{j up} c_{j+1 dn} - c_{j dn} c_{j+1 up}) / sqrt 2,  Delta+_i = (c+_{i+1 dn} c+_{i up} - c+_{i+1 up} c+_{i dn}) / sqrt 2
    sp = np.zeros((L - 1, L - 1))
    for i in range(L - 1):
        for j in range(L - 1):
            for fa, (s1, s2) in ((1.0, (1, 0)), (-1.0, (0, 1))):
                for fb, (s3, s4) in ((1.0, (0, 1)), (-1.0, (1, 0))):
                    sp[i, j] += 0.5 * fa * fb * (psi @ cc._apply(e, psi, [cd(i + 1, s1), cd(i, s2), c(j, s3), c(j + 1, s4)]))
    corr["spair"] = sp
    return E0, corr, mean


def converged_engine(ops, case, mode, sweeps=6, seed=5):
    """two-site DMRG at full bond dimension (nothing truncated) in one of the three symmetry modes -> engine, centre on site 0"""
    L, t, u, nu, nd, mu = CASES[case]
    if mode == "su2p":
        sim, target = models.OBC_Sim2(t, u, mu), (0, 0)
    else:
        sim, target = (models.OB_Sim(t, u, 0.0, 1, 1, 2.0, 50, spin=True) if mode == "u1" else models.OB_Sim(t, u)), (nu + nd, nu - nd)
    H = models.hamiltonian(sim, L)
    bonds, tens = mps.random_mps(L, target, 4000, seed=seed, max_twoS=L, sym=H.sym)
    eng = engine.DMRG2(ops, H, bonds, tens, chi_full=None, lanczos_tol=1e-13)
    for _ in range(sweeps):
        eng.sweep()
    return eng


def kinds_of(mode):
    return U1_KINDS if mode == "u1" else SU2_KINDS if mode == "su2" else ("bond", "dimer")


def compare_with_ed(eng, corr, kinds, tol=TOL_ED):
    """prints every deviation (disjoint, adjacent and identical bonds apart), then asserts all of them"""
    devs = {}
    for k in kinds:
        C = eng.bond_correlator(k)
        assert C.shape == corr[k].shape
        D = np.abs(C - corr[k])
        n = D.shape[0]
        sep = np.abs(np.subtract.outer(np.arange(n), np.arange(n)))
        devs[k] = float(D.max())
        print("bond correlator", k, "max deviation from ED: same bond", float(D[sep == 0].max()), "shared site",
              float(D[sep == 1].max()) if n > 1 else 0.0, "disjoint", float(D[sep >= 2].max()) if n > 2 else 0.0)
    for k, d in devs.items():
        assert d <= tol, (k, d)
    return devs


def check_centre_independence(eng, ref, centres):
    """with the centre moved to each of `centres` (both passes re-lay site tensors): every kind of `ref` = {kind: result with the
    centre on site 0} within 1e-12, the centre where it was put, the site tensors unchanged bit for bit"""
    for centre in centres:
        eng.move_centre(centre)
        before = [eng.site_vector(i).copy() for i in range(eng.L)]
        for k, r in ref.items():
            d = float(np.abs(eng.bond_correlator(k) - r).max())
            print("centre", centre, k, d)
            assert d <= 1e-12, (centre, k, d)
        assert eng.centre() == centre
        for i in range(eng.L):
            assert np.array_equal(eng.site_vector(i), before[i]), i


def check_repeated_calls_plan_nothing(eng):
    """eng: a converged L6 engine, centre on site 0.  The second call of correlator("hop") and of bond_correlator("dimer") finds
    every plan in the cache (no miss) and returns the same bits.  With the centre on site 3 the passes re-lay site tensors: the
    two-point pass plans the two re-lay directions (at most 2 misses), the bond pass after it and every repeat plan nothing."""
    assert eng.centre() == 0
    calls = (("hop", lambda: eng.correlator("hop")), ("dimer", lambda: eng.bond_correlator("dimer")))
    for moved, allowed in ((False, (None, None)), (True, (2, 0))):
        if moved:
            eng.move_centre(3)
        for (name, call), limit in zip(calls, allowed):
            m0 = eng.cache_misses
            a = call()
            m1 = eng.cache_misses
            b = call()
            print(name, "centre", eng.centre(), "misses of the first call", m1 - m0, "of the repeat", eng.cache_misses - m1)
            assert limit is None or m1 - m0 <= limit, (name, m1 - m0)
            assert eng.cache_misses == m1 and np.array_equal(a, b), name


# ---- free fermions: Wick's theorem from G = sum_s <c+_is c_js> of a spin-symmetric Slater determinant ------------------------------
def wick_bond(G):
    """<B_i B_j>: <E_ab E_cd> = G_ab G_cd + 2 g_ad (delta_bc - g_cb), g = G / 2, E_ab = sum_s c+_as c_bs, B_i = E_{i,i+1} + E_{i+1,i}"""
    g, n = G / 2.0, G.shape[0]
    EE = lambda a, b, c_, d: G[a, b] * G[c_, d] + 2.0 * g[a, d] * ((b == c_) - g[c_, b])
    out = np.zeros((n - 1, n - 1))
    for i in range(n - 1):
        for j in range(n - 1):
            out[i, j] = sum(EE(a, b, c_, d) for a, b in ((i, i + 1), (i + 1, i)) for c_, d in ((j, j + 1), (j + 1, j)))
    return out


def wick_spair(G):
    """<Delta+_i Delta_j> = g_ij g_{i+1,j+1} + g_{i,j+1} g_{i+1,j}"""
    g = G / 2.0
    return g[:-1, :-1] * g[1:, 1:] + g[:-1, 1:] * g[1:, :-1]


def free_fermion_engine(ops, L, chi, sweeps=8):
    H = models.hamiltonian(models.OB_Sim([1.0], [0.0]), L)
    bonds, tens = mps.random_mps(L, (L, 0), 8, seed=11)
    eng = engine.DMRG2(ops, H, bonds, tens, chi_full=chi, lanczos_tol=1e-13)
    for _ in range(sweeps):
        E = eng.sweep()
    return eng, E


def wick_deviations(eng):
    G = np.real(eng.correlator("hop"))
    return {"bond": float(np.abs(eng.bond_correlator("bond") - wick_bond(G)).max()),
            "spair": float(np.abs(eng.bond_correlator("spair") - wick_spair(G)).max())}
