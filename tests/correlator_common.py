"""Shared by test_correlator_cpu.py / test_correlator_gpu.py: two-point functions of exact-diagonalisation ground states
(operators applied to the ED vector with bit operations, in the basis oracle.ed.SectorED documents), the converged DMRG runs
they are compared with, free-fermion closed forms and the sum rules of a random state."""
import numpy as np

from hubbardtn_amd import engine, models, mps
from oracle import ed, su2

KINDS = ("hop", "nn", "ss", "pair")
# (t, u, N_up, N_dn): half filling, and N = 4 with a nearest-neighbour repulsion (nothing particle-hole symmetric)
ED_CASES = {"half": ([1.0], [4.0], 3, 3), "doped": ([1.0], [4.0, 1.0], 2, 2)}
ED_L = 6


def _popcount(x):
    return bin(x).count("1")


def _apply(e, psi, string):
    """|out> = (product of the string's operators, leftmost factor first) |psi> inside the sector of `e`; an operator is
    (dagger, site, spin); fermion order of SectorED: up modes 0..L-1, then down modes; basis index = i_up * n_dn + i_dn"""
    nd = len(e.dn)
    out = np.zeros_like(psi)
    for a, bu in enumerate(e.up):
        for b, bd in enumerate(e.dn):
            amp = psi[a * nd + b]
            if amp == 0.0:
                continue
            u, d, sign = bu, bd, 1
            for (dag, site, spin) in reversed(string):
                bits = u if spin == 0 else d
                occ = (bits >> site) & 1
                if occ == dag:                      # create on an occupied / annihilate on an empty mode
                    sign = 0
                    break
                before = _popcount(u & ((1 << site) - 1)) if spin == 0 else _popcount(u) + _popcount(d & ((1 << site) - 1))
                if before & 1:
                    sign = -sign
                if spin == 0:
                    u ^= 1 << site
                else:
                    d ^= 1 << site
            if sign and u in e.iu and d in e.idn:
                out[e.iu[u] * nd + e.idn[d]] += sign * amp
    return out


def ed_correlators(L, t, u, n_up, n_dn):
    """{kind: L x L matrix} on the ED ground state of the (n_up, n_dn) sector (the S = Sz ground state: n_up = n_dn here)"""
    e = ed.SectorED(L, n_up, n_dn, t, u)
    E0, psi = e.ground_state()
    psi = np.asarray(psi, dtype=float)
    ex = lambda string: float(psi @ _apply(e, psi, string))
    cd = lambda i, s: (1, i, s)
    c = lambda i, s: (0, i, s)
    n_s = lambda i, s: [cd(i, s), c(i, s)]
    out = {k: np.zeros((L, L)) for k in KINDS}
    for i in range(L):
        for j in range(L):
            out["hop"][i, j] = sum(ex([cd(i, s), c(j, s)]) for s in (0, 1))
            out["nn"][i, j] = sum(ex(n_s(i, s) + n_s(j, s2)) for s in (0, 1) for s2 in (0, 1))
            # D = c_dn c_up, D+ = c+_up c+_dn
            out["pair"][i, j] = ex([cd(i, 0), cd(i, 1), c(j, 1), c(j, 0)])
            szsz = sum((0.5 if s == 0 else -0.5) * (0.5 if s2 == 0 else -0.5) * ex(n_s(i, s) + n_s(j, s2)) for s in (0, 1) for s2 in (0, 1))
            spm = ex([cd(i, 0), c(i, 1), cd(j, 1), c(j, 0)])          # S+_i S-_j
            smp = ex([cd(i, 1), c(i, 0), cd(j, 0), c(j, 1)])          # S-_i S+_j
            out["ss"][i, j] = szsz + 0.5 * (spm + smp)
            out.setdefault("szsz", np.zeros((L, L)))[i, j] = szsz
            out.setdefault("s+-", np.zeros((L, L)))[i, j] = spm
            out.setdefault("s-+", np.zeros((L, L)))[i, j] = smp
            out.setdefault("hop_up", np.zeros((L, L)))[i, j] = ex([cd(i, 0), c(j, 0)])
            out.setdefault("hop_dn", np.zeros((L, L)))[i, j] = ex([cd(i, 1), c(j, 1)])
    return E0, out


def converged_engine(ops, L, t, u, target, spin=False, sweeps=6, seed=5):
    """two-site DMRG at full bond dimension (nothing truncated) -> engine, centre on site 0"""
    sim = models.OB_Sim(t, u, 0.0, 1, 1, 2.0, 50, spin=True) if spin else models.OB_Sim(t, u)
    H = models.hamiltonian(sim, L)
    bonds, tens = mps.random_mps(L, target, 4000, seed=seed, max_twoS=L, sym=H.sym)
    eng = engine.DMRG2(ops, H, bonds, tens, chi_full=None, lanczos_tol=1e-13)
    for _ in range(sweeps):
        eng.sweep()
    return eng


def ed_engine(ops, case, spin=False):
    t, u, nu, nd = ED_CASES[case]
    return converged_engine(ops, ED_L, t, u, (nu + nd, nu - nd), spin=spin)


def compare_with_ed(eng, ref, kinds=KINDS, tol=1e-8):
    """prints every deviation, then asserts all of them"""
    devs = {}
    for k in kinds:
        C = eng.correlator(k)
        devs[k] = float(np.abs(C - ref[k]).max())
        print("correlator", k, "max deviation from ED", devs[k], "anti-Hermitian part", float(np.abs(C - C.conj().T).max()))
    for k, d in devs.items():
        assert d <= tol, (k, d)
    return devs


def dense_parity_reference(L, t, u, mu):
    """<n_i n_j> and <S_i . S_j> on the ground state of oracle.ed.dense_hamiltonian (all particle numbers, Jordan-Wigner
    product basis, site 1 most significant)"""
    H = ed.dense_hamiltonian(L, t, u, mu)
    w, v = np.linalg.eigh(H)
    assert w[1] - w[0] > 1e-6, "degenerate dense ground state"
    psi = v[:, 0]
    lm = su2.local_matrices()

    def site(mats):
        out = np.eye(1)
        for s in range(L):
            out = np.kron(out, mats.get(s, lm["id"]))
        return out
    sp_loc = lm["a_up"].T @ lm["a_dn"]
    sz_loc = 0.5 * (lm["a_up"].T @ lm["a_up"] - lm["a_dn"].T @ lm["a_dn"])
    nn, ss = np.zeros((L, L)), np.zeros((L, L))
    for i in range(L):
        for j in range(L):
            nn[i, j] = psi @ site({i: lm["n"]}) @ site({j: lm["n"]}) @ psi
            sdots = site({i: sz_loc}) @ site({j: sz_loc}) + 0.5 * (site({i: sp_loc}) @ site({j: sp_loc.T}) + site({i: sp_loc.T}) @ site({j: sp_loc}))
            ss[i, j] = psi @ sdots @ psi
    return float(w[0]), {"nn": nn, "ss": ss}


# ---- free fermions ------------------------------------------------------------------------------------------------------------
def free_fermion_G(L, N):
    """sum_s <c+_is c_js> of the U = 0 open chain with N / 2 filled levels per spin"""
    x = np.arange(1, L + 1)
    G = np.zeros((L, L))
    for k in range(1, N // 2 + 1):
        phi = np.sqrt(2.0 / (L + 1)) * np.sin(k * np.pi * x / (L + 1))
        G += 2.0 * np.outer(phi, phi)
    return G


def wick(G):
    """<n_i n_j> and <S_i . S_j> of a spin-symmetric Slater determinant with G = sum_s <c+_is c_js> (g = G / 2 per spin):
    i != j: <n_i n_j> = n_i n_j - 2 g_ij^2, <S_i . S_j> = -3/2 g_ij^2; i == j: <n^2> = n + 2 g_ii^2 (n + 2 docc, docc = g_ii^2),
    <S^2> = 3/4 (n - 2 docc)"""
    g = G / 2.0
    n = np.diag(G)
    nn = np.outer(n, n) - 2.0 * g ** 2
    ss = -1.5 * g ** 2
    docc = np.diag(g) ** 2
    nn[np.diag_indices_from(nn)] = n + 2.0 * docc
    ss[np.diag_indices_from(ss)] = 0.75 * (n - 2.0 * docc)
    return nn, ss


def free_fermion_deviations(ops, L=12, chi=200, sweeps=8):
    """max deviations of hop / nn / ss of the truncated U = 0 ground state from the closed forms"""
    H = models.hamiltonian(models.OB_Sim([1.0], [0.0]), L)
    bonds, tens = mps.random_mps(L, (L, 0), 8, seed=11)
    eng = engine.DMRG2(ops, H, bonds, tens, chi_full=chi, lanczos_tol=1e-13)
    for _ in range(sweeps):
        eng.sweep()
    G = free_fermion_G(L, L)
    nn, ss = wick(G)
    return {"hop": float(np.abs(eng.correlator("hop") - G).max()), "nn": float(np.abs(eng.correlator("nn") - nn).max()),
            "ss": float(np.abs(eng.correlator("ss") - ss).max())}


# ---- sum rules --------------------------------------------------------------------------------------------------------------------
def check_sum_rules(ops, L, cap, target=(8, 2), seed=21):
    """exact for ANY state of the sector (N, 2S): tr G = N, sum_j <n_i n_j> = N G_ii, sum_ij <S_i . S_j> = S (S + 1), G Hermitian
    with eigenvalues in [0, 2]; the state is random and unoptimised, so rounding is the only error: 1e-12 L^2"""
    N, twoS = target
    H = models.hamiltonian(models.OB_Sim([1.0], [4.0]), L)
    bonds, tens = mps.random_mps(L, target, cap, seed=seed)
    eng = engine.DMRG2(ops, H, bonds, tens, chi_full=None)
    tol = 1e-12 * L * L
    G, Cnn, Css = eng.correlator("hop"), eng.correlator("nn"), eng.correlator("ss")
    S = twoS / 2.0
    figs = {"trace": abs(np.trace(G) - N), "nn rows": float(np.abs(Cnn.sum(axis=1) - N * np.diag(G)).max()),
            "spin": abs(Css.sum() - S * (S + 1)), "hermitian": float(np.abs(G - G.conj().T).max())}
    w = np.linalg.eigvalsh(0.5 * (G + G.conj().T))
    figs["eig low"], figs["eig high"] = max(0.0, -w.min()), max(0.0, w.max() - 2.0)
    print("sum rules", figs, "tol", tol, "max block", max(max(b.values()) for b in bonds))
    for k, v in figs.items():
        assert v <= tol, (k, v, tol)
    return eng, bonds


# ---- gauge independence, read-only behaviour, plan-cache keys ----------------------------------------------------------------------
def check_gauge_and_readonly(ops, case="half"):
    t, u, nu, nd = ED_CASES[case]
    eng = ed_engine(ops, case)
    L = eng.L
    ref = {k: eng.correlator(k) for k in ("hop", "ss")}
    for i in range(L // 2):                                   # centre to the middle: no optimisation, no truncation
        eng.update_bond(i, +1, "right", optimise=False, record=False, cutoff=0.0)
    assert eng.centre() == L // 2
    before = [eng.site_vector(i).copy() for i in range(L)]
    kinds_before = [eng.site_kind(i) for i in range(L)]
    for k, r in ref.items():
        d = float(np.abs(eng.correlator(k) - r).max())
        print("gauge", k, d)
        assert d <= 1e-12, (k, d)
    assert [eng.site_kind(i) for i in range(L)] == kinds_before and eng.centre() == L // 2
    for i in range(L):
        assert np.array_equal(eng.site_vector(i), before[i]), i
    # a probe plan filed under the Hamiltonian's environment keys would replace those plans: the sweep after a correlator call
    # must plan exactly what it plans without one (same misses) and find the same energy
    def sweep_misses(measure):
        e2 = ed_engine(ops, case)
        if measure:
            e2.correlator("hop")
        m0 = e2.cache_misses
        E = e2.sweep()
        return e2.cache_misses - m0, E
    (m_plain, E_plain), (m_meas, E_meas) = sweep_misses(False), sweep_misses(True)
    print("cache misses of the following sweep", m_plain, m_meas, "energies", E_plain, E_meas)
    assert m_meas <= m_plain and abs(E_plain - E_meas) <= 1e-12 * max(1.0, abs(E_plain))
