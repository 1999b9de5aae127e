"""Shared by test_sample_cpu.py / test_sample_gpu.py: perfect sampling (htn_mps_sample / engine.DMRG2.sample / api.sample) against
the dense expansion of the same stored state.  The reference probability of a configuration of site multiplets is
p_ref = <psi|prod_i P_{s_i}|psi>: the state is expanded with excited_common.dense_state (Clebsch-Gordan tensors in the SU(2) kinds),
squared, and summed over the basis states of every multiplet -- neither the code under test nor the log-probabilities it returns.
The bodies run on either library."""
import numpy as np
import pytest

import correlator_common as cc
import excited_common as xc
import thermal_common as tc
from hubbardtn_amd import abi, api, engine, models, mps

L = cc.ED_L
KINDS = ("su2", "u1", "parity")
CASES = ("half", "doped")
COMBOS = [(k, c) for k in KINDS for c in CASES]
PARITY_MU = {"half": 2.0, "doped": 0.0}          # chemical potentials of the parity-only model at U = 4 (mu = U / 2: half filling)
N_EXACT, SEED_EXACT = 256, 11
N_STAT, SEED_STAT = 4096, 5
# Largest relative deviation of exp(logp) from p_ref over the 256 samples of every (kind, case), measured on the CPU baseline
# library (test_exact_probabilities prints it): 3.3e-15 (spinful kind, doped; 1.8e-15 .. 3.0e-15 for the other five states).  The bar
# of the exact-probability and marginal tests is 100 times that, and never more than 1e-9.
CPU_MEASURED = 3.3e-15
TOL = min(100.0 * CPU_MEASURED, 1e-9)
EDGE = 1e-9                                      # a uniform this close to a cumulative threshold (relative to the total) decides nothing

_cache = {}


def build_engine(ops, kind, case):
    """converged two-site DMRG at full bond dimension (nothing truncated), centre on site 0"""
    if kind == "su2":
        return cc.ed_engine(ops, case)
    if kind == "u1":
        return cc.ed_engine(ops, case, spin=True)
    H = models.hamiltonian(models.OBC_Sim2([1.0], [4.0], PARITY_MU[case]), L)
    bonds, tens = mps.random_mps(L, (0, 0), 4000, seed=3, sym=H.sym)
    eng = engine.DMRG2(ops, H, bonds, tens, chi_full=None, lanczos_tol=1e-13)
    for _ in range(6):
        eng.sweep()
    return eng


def multiplet_table(eng):
    """P[s_0, .., s_{L-1}] of the stored state from its dense expansion (normalised by its own sum)"""
    sym = eng.sym
    bonds = [dict(b.dims) for b in eng.bonds]
    tensors = [eng.download_site(i) for i in range(eng.L)]
    psi = xc.dense_state(bonds, tensors, sym, 0)
    w = (np.abs(psi) ** 2).sum(axis=1)
    dims = [(sym.site_mult[s][1] if sym.su2 else 0) + 1 for s in range(sym.n_site)]
    d = sum(dims)
    G = np.zeros((sym.n_site, d))
    pos = 0
    for s, k in enumerate(dims):
        G[s, pos:pos + k] = 1.0
        pos += k
    P = w.reshape([d] * eng.L)
    for ax in range(eng.L):
        P = np.moveaxis(np.tensordot(G, P, axes=(1, ax)), 0, ax)
    tot = P.sum()
    assert abs(tot - 1.0) <= 1e-12, tot
    return P / tot


def state(ops, kind, case):
    """(engine, P_ref, site_probabilities of a copy): built once per library and shared by the tests, never modified"""
    key = (id(ops), kind, case)
    if key not in _cache:
        eng = build_engine(ops, kind, case)
        _cache[key] = (eng, multiplet_table(eng), eng.copy().site_probabilities())
    return _cache[key]


def uniforms(n, seed, L_=L):
    return np.random.default_rng(seed).random((n, L_))


def p_of(P, occ):
    return P[tuple(np.asarray(occ).T)]


# ---- 1. exact probabilities ---------------------------------------------------------------------------------------------------------
def check_exact(ops, kind, case, tol=TOL):
    eng, P, _ = state(ops, kind, case)
    occ, logp = eng.sample(uniforms(N_EXACT, SEED_EXACT))
    ref = p_of(P, occ)
    assert occ.shape == (N_EXACT, L) and occ.min() >= 0 and occ.max() < eng.sym.n_site and ref.min() > 0.0
    dev = float((np.abs(np.exp(logp) - ref) / ref).max())
    n = np.asarray(eng.sym.site_electrons)[occ].sum(axis=1)
    print("RESULT exact", kind, case, "max relative deviation of exp(logp) from p_ref", dev, "bar", tol, "smallest p drawn", float(ref.min()),
          "mean N", float(n.mean()))
    if case == "doped":
        assert abs(n.mean() - L) > 0.5                                   # (the doped case is doped)
    assert dev <= tol, (kind, case, dev)
    return dev


# ---- 2. the rule of the draw --------------------------------------------------------------------------------------------------------
def reference_draws(P, u, occ):
    """every draw recomputed from the reference conditionals along the library's own history: -> (expected multiplets, mask of the
    samples none of whose uniforms lies within EDGE of a cumulative threshold)"""
    n, Ls = u.shape
    want = np.zeros_like(occ)
    safe = np.ones(n, dtype=bool)
    margs = [P.sum(axis=tuple(range(i + 1, Ls))) if i + 1 < Ls else P for i in range(Ls)]
    for b in range(n):
        for i in range(Ls):
            p = np.array(margs[i][tuple(occ[b, :i])], dtype=float)
            p[p < 1e-20] = 0.0                                           # (structural zeros of the state come out as rounding dust)
            tot = p.sum()
            cum = np.cumsum(p)
            target = u[b, i] * tot
            live = np.nonzero(p > 0.0)[0]
            hit = [s for s in live if cum[s] >= target]
            want[b, i] = hit[0] if hit else live[-1]
            if np.abs(cum[live] - target).min() <= EDGE * tot:
                safe[b] = False
    return want, safe


def check_choice_rule(ops, kind, case):
    eng, P, _ = state(ops, kind, case)
    u = uniforms(N_EXACT, SEED_EXACT)
    occ, _ = eng.sample(u)
    want, safe = reference_draws(P, u, occ)
    left_out = int((~safe).sum())
    print("RESULT choice", kind, case, "samples left out", left_out, "of", len(u))
    assert left_out <= len(u) // 100
    assert np.array_equal(occ[safe], want[safe])


# ---- 3. reproducibility -----------------------------------------------------------------------------------------------------------------
def check_reproducible(ops, kind, case):
    eng, _, _ = state(ops, kind, case)
    u = uniforms(N_EXACT, SEED_EXACT)
    occ, logp = eng.sample(u)
    again = eng.sample(u)
    assert np.array_equal(occ, again[0]) and np.array_equal(logp.view(np.int64), again[1].view(np.int64))
    for batch in (1, 5, 64):
        o, l = eng.sample(u, batch=batch)
        assert np.array_equal(o, occ), batch
        assert np.array_equal(l.view(np.int64), logp.view(np.int64)), batch


# ---- 4. marginals: the closing weight ---------------------------------------------------------------------------------------------------
def check_marginals(ops, kind, case, tol=TOL):
    eng, _, Psite = state(ops, kind, case)
    worst = 0.0
    for i in range(L):
        measure = np.zeros(L, dtype=int)
        measure[i] = 1
        occ, logp = eng.sample(uniforms(64, 100 + i), measure=measure)
        assert np.all(occ[:, np.arange(L) != i] == -1) and occ[:, i].min() >= 0
        ref = Psite[i, occ[:, i]]
        worst = max(worst, float((np.abs(np.exp(logp) - ref) / ref).max()))
    print("RESULT marginals", kind, case, "max relative deviation from site_probabilities", worst, "bar", tol)
    assert worst <= tol, (kind, case, worst)


# ---- 5. statistics ------------------------------------------------------------------------------------------------------------------------
def statistics_pass(P, occ, electrons, density):
    """mean n_i within 5 standard errors of `density`, the frequencies of the ten most probable configurations within 5 binomial
    standard errors of p_ref -> (passes, worst ratio)"""
    n = len(occ)
    Ls = occ.shape[1]
    Ns = np.asarray(electrons, dtype=float)
    worst = 0.0
    for i in range(Ls):
        pm = P.sum(axis=tuple(a for a in range(Ls) if a != i))
        var = float(pm @ Ns ** 2 - (pm @ Ns) ** 2)
        worst = max(worst, abs(Ns[occ[:, i]].mean() - density[i]) / np.sqrt(var / n))
    flat = np.ravel_multi_index(tuple(occ.T), P.shape)
    for idx in np.argsort(P.ravel())[::-1][:10]:
        p = float(P.ravel()[idx])
        worst = max(worst, abs(float(np.mean(flat == idx)) - p) / np.sqrt(p * (1.0 - p) / n))
    return worst <= 5.0, worst


def check_statistics(ops, kind, case):
    eng, P, _ = state(ops, kind, case)
    psi = api.FiniteMPS(eng.copy(), L)                                   # (density_state carries the centre through the chain)
    density = api.density_state(psi)
    # the seed: the reference probabilities fed through numpy's own sampler pass with it
    ref_idx = np.random.default_rng(SEED_STAT).choice(P.size, size=N_STAT, p=P.ravel())
    ok_ref, w_ref = statistics_pass(P, np.array(np.unravel_index(ref_idx, P.shape)).T, eng.sym.site_electrons, density)
    assert ok_ref, w_ref
    s = api.sample(api.FiniteMPS(eng, L), N_STAT, seed=SEED_STAT)
    assert np.array_equal(s.sites, np.arange(L)) and s.multiplets.shape == (N_STAT, L) and len(s) == N_STAT
    assert np.array_equal(s.electrons, np.asarray(eng.sym.site_electrons)[s.multiplets])
    ok, worst = statistics_pass(P, s.multiplets, eng.sym.site_electrons, density)
    print("RESULT statistics", kind, case, "worst deviation in standard errors", worst, "numpy's sampler on p_ref", w_ref)
    assert ok, worst
    # full counting statistics of the left half against the reference distribution of its particle number
    vals, f, err = api.full_counting_statistics(s, [0, 1, 2])
    Ns = np.asarray(eng.sym.site_electrons)
    pm = P.sum(axis=(3, 4, 5))
    want = np.zeros(7)
    for a in range(P.shape[0]):
        for b in range(P.shape[0]):
            for c in range(P.shape[0]):
                want[Ns[a] + Ns[b] + Ns[c]] += pm[a, b, c]
    assert np.array_equal(vals, np.arange(7)) and abs(f.sum() - 1.0) <= 1e-12
    assert np.all(np.abs(f - want) <= 5.0 * np.sqrt(want * (1.0 - want) / N_STAT) + 1e-15)
    if kind == "u1":
        assert np.array_equal(s.sz, np.array([0.0, 0.5, -0.5, 0.0])[s.multiplets]) and abs(s.sz.sum(axis=1)).max() == 0.0


# ---- 6. thermal states --------------------------------------------------------------------------------------------------------------------
def check_thermal_beta0(ops, mode):
    Lp = 3
    psi = api.thermal_state(tc.simulation(mode, "mu2"), Lp, ops=ops)
    s = api.sample(psi, 64, seed=3)
    assert s.multiplets.shape == (64, Lp) and np.array_equal(s.sites, np.arange(0, 2 * Lp, 2)) and s.multiplets.min() >= 0
    if mode == "u1":
        want = np.full(64, -Lp * np.log(4.0))
    else:
        want = np.log(np.array([0.25, 0.5, 0.25]))[s.multiplets].sum(axis=1)
    dev = float(np.abs(s.log_prob - want).max())
    print("RESULT thermal beta = 0", mode, "max |logp - exact|", dev)
    assert dev <= 1e-12


def check_thermal_cooled(ops, mode, case="mu2"):
    """beta = 1, L = 3, nothing truncated: exp(logp) against the diagonal of exp(-beta H) / Z summed over the basis states of every
    multiplet; the bar is ten times the error of cool's own energy against ED on this run"""
    Lp, beta = 3, 1.0
    psi = api.thermal_state(tc.simulation(mode, case), Lp, ops=ops)
    out = api.cool(psi, [beta], tc.untruncated())
    ref = tc.thermal_reference(Lp, case)
    dE = abs(out["energy"][0] - ref.at(beta)["energy"])
    pk = np.exp(-beta * (ref.w - ref.w[0]))
    pk /= pk.sum()
    diag = (ref.v ** 2) @ pk                                             # site basis |0>, |up>, |dn>, |up dn>, site 0 most significant
    mult = [0, 1, 1, 2] if mode != "u1" else [0, 1, 2, 3]
    ns = 3 if mode != "u1" else 4
    P = np.zeros([ns] * Lp)
    for x, p in enumerate(diag):
        P[tuple(mult[(x // 4 ** (Lp - 1 - i)) % 4] for i in range(Lp))] += p
    s = api.sample(psi, 256, seed=7)
    dev = float(np.abs(np.exp(s.log_prob) - p_of(P, s.multiplets)).max())
    print("RESULT thermal beta = 1", mode, "max |exp(logp) - p_thermal|", dev, "energy error of cool", dE, "bar", 10.0 * dE)
    assert dev <= 10.0 * dE, (dev, dE)


# ---- 8. refusals and plans ----------------------------------------------------------------------------------------------------------------
def check_refusals(ops, make_hooked_ops):
    eng = build_engine(ops, "su2", "half")
    u = uniforms(4, 1)
    with pytest.raises(ValueError, match="shape"):
        eng.sample(u[:, :3])
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        eng.sample(u + 1.0)
    eng.update_bond(0, +1, "right", optimise=False, record=False, cutoff=0.0)
    with pytest.raises(abi.HtnError, match="the centre is on site 1, not on site 0"):
        eng.sample(u)
    s = api.sample(api.FiniteMPS(eng, L), 4, seed=1)                     # api.sample works on a copy moved to site 0
    assert eng.centre() == 1 and s.multiplets.shape == (4, L)
    with pytest.raises(ValueError, match="spin independent"):
        s.sz
    other = build_engine(ops, "su2", "half")
    eng.move_centre(0)
    eng.set_orthogonal([other])
    with pytest.raises(abi.HtnError, match="attached orthogonal states"):
        eng.sample(u)
    eng.set_orthogonal([])
    hooked = make_hooked_ops()
    hooked.set_exchange(0, 1, lambda y: None)
    b4, t4 = mps.random_mps(4, (4, 0), 8, seed=2)
    e2 = engine.DMRG2(hooked, models.hamiltonian(models.OB_Sim([1.0], [4.0]), 4), b4, t4)
    with pytest.raises(abi.HtnError, match="communicator or an exchange hook"):
        e2.sample(uniforms(2, 1, 4))
    with pytest.raises(NotImplementedError, match="chain length"):
        api.sample(api.InfiniteMPS(8), 4)


def check_cache_hygiene(ops):
    def sweep_misses(measure):
        e2 = build_engine(ops, "su2", "half")
        if measure:
            e2.sample(uniforms(8, 2))
        m0 = e2.cache_misses
        E = e2.sweep()
        return e2.cache_misses - m0, E
    (m_plain, E_plain), (m_meas, E_meas) = sweep_misses(False), sweep_misses(True)
    print("cache misses of the following sweep", m_plain, m_meas, "energies", E_plain, E_meas)
    assert m_meas == m_plain and abs(E_plain - E_meas) <= 1e-12 * max(1.0, abs(E_plain))


def check_abi(lib_cpu, lib_hip):
    assert abi.SAMPLE_DT.itemsize == 64 and abi.SAMPLE_DT.fields["coef"][1] == 56 and abi.SAMPLE_DT.fields["n_l"][1] == 32
    assert hasattr(lib_cpu, "htn_mps_sample") and not hasattr(lib_cpu, "htn_sample_step_z")
    assert hasattr(lib_hip, "htn_mps_sample") and hasattr(lib_hip, "htn_sample_step_z")
    assert "htn_mps_sample" in abi.ENGINE_EXPORTS and "htn_sample_step_z" in abi.EXPORTS
