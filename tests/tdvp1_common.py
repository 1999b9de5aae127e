"""Shared by test_tdvp1_cpu.py / test_tdvp1_gpu.py: chains whose bonds two-site sweeps have grown and capped, the host side of
the identity H_eff0(C) = Q^H H_eff1(Q C), and the bodies of the one-site TDVP tests, which run on either library."""
import ctypes as C

import numpy as np

import tdvp_common as tc
from hubbardtn_amd import abi, engine, models, mps

SYMS = ["SU2U1", "U1U1", "SU2P"]
CASES = SYMS + ["range2"]


# ---- states ---------------------------------------------------------------------------------------------------------
def model(symname, L, t=(1.0,), U=4.0):
    """(MPO, total sector) of a half-filled chain in each of the three symmetry kinds"""
    t = list(t)
    if symname == "SU2U1":
        return models.hamiltonian(models.OB_Sim(t, [U]), L), (L, 0)
    if symname == "U1U1":
        return models.hamiltonian(models.OB_Sim(t, [U], 0.0, 1, 1, 2.0, 6, spin=True), L), (L, 0)
    return models.hamiltonian(models.OBC_Sim2(t, [U], 2.0), L), (0, 0)


def capped_state(ops, symname="SU2U1", L=10, chi=20, t=(1.0,), U=4.0, sweeps=3, seed=5):
    """an engine whose bonds `sweeps` two-site sweeps have grown under the cap truncdim(chi): the tables are not full and the
    sectors of a bond have different dimensions.  lanczos_tol = 1e-12, krylovdim = 30 afterwards."""
    H, target = model(symname, L, t, U)
    b, tn = mps.random_mps(L, target, 6, seed=seed, sym=H.sym)
    e = engine.DMRG2(ops, H, b, tn, chi_full=chi, krylovdim=20, lanczos_tol=1e-10, maxrestart=8)
    for _ in range(sweeps):
        e.sweep()
    e.krylovdim, e.lanczos_tol = 30, 1e-12
    return e


def tables(e):
    return [dict(x.dims) for x in e.bonds]


def sector_dims(e):
    """all n_c of the inner bonds"""
    return [n for b in tables(e)[1:-1] for n in b.values()]


def stored_energy(e):
    """<psi|H|psi> of the state as stored, from a copy (the pass moves the centre and, under a cap, could truncate)"""
    c = e.copy()
    c.chi_full, c.cutoff = None, 0.0
    return c.bond_energies()[0]


# ---- site vectors and bond vectors on the host ------------------------------------------------------------------------
def site_table(e, i):
    """[((l, s, r), off, ld, n_l, n_r)] of the stored layout of site i and the length of its flat vector"""
    nb = e.lib.htn_mps_get_site(e.handle, i, None, None)
    subs = np.zeros(max(nb, 1), dtype=abi.SUBBLOCK_DT)
    assert e.lib.htn_mps_get_site(e.handle, i, subs.ctypes.data, None) >= 0
    bl, br = e.bond(i).dims, e.bond(i + 1).dims
    out = []
    for sb in subs[:nb]:
        l, r = (int(sb["lN"]), int(sb["lj"])), (int(sb["rN"]), int(sb["rj"]))
        out.append(((l, int(sb["s"]), r), int(sb["off"]), int(sb["ld"]), bl[l], br[r]))
    return out, int(e.lib.htn_mps_site_size(e.handle, i, None))


def pack_site(table, size, blocks):
    flat = np.zeros(size, dtype=np.complex128)
    for key, off, ld, m, n in table:
        flat[off + np.arange(m)[:, None] + ld * np.arange(n)[None, :]] = blocks[key]
    return flat


def unpack_site(table, flat):
    return {key: flat[off + np.arange(m)[:, None] + ld * np.arange(n)[None, :]] for key, off, ld, m, n in table}


def bond_secs(e, b):
    return sorted(e.bond(b).dims.items())


def pack_bond(e, b, mats):
    """{sector: [n_c, n_c]} -> the flat vector in bond layout (sectors in order, column-major)"""
    return np.concatenate([np.asarray(mats[c], dtype=np.complex128).reshape(-1, order="F") for c, _ in bond_secs(e, b)])


def unpack_bond(e, b, flat):
    out, pos = {}, 0
    for c, n in bond_secs(e, b):
        out[c] = flat[pos:pos + n * n].reshape(n, n, order="F")
        pos += n * n
    assert pos == flat.size == e.bond_size(b)
    return out


def heff0_through_heff1(stay, Q, i, direction, Cm):
    """Q^H H_eff1(Q C) on site i of `stay` (centre on i), Q = the isometry blocks a gauge move left on site i of a second engine:
    direction +1: x[(l, s, r)] = Q[(l, s, r)] C_r and y_r = sum Q^H y[(l, s, r)]; -1: x = C_l Q and y_l = sum y Q^H"""
    tab, size = site_table(stay, i)
    x = {k: (Q[k] @ Cm[k[2]] if direction > 0 else Cm[k[0]] @ Q[k]) for k in Q}
    y = unpack_site(tab, stay.apply_heff1(i, pack_site(tab, size, x)))
    out = {c: np.zeros_like(m) for c, m in Cm.items()}
    for k in Q:
        if direction > 0:
            out[k[2]] += Q[k].conj().T @ y[k]
        else:
            out[k[0]] += y[k] @ Q[k].conj().T
    return out


# ---- test bodies ----------------------------------------------------------------------------------------------------
def body_heff0_identity(ops, case, L=10, chi=20, sweeps=3, wider_than=0):
    """test 1: for every bond and both gauge directions, apply_heff0(b, C) = Q^H H_eff1(Q C) to 1e-12 on a random C, <C|H_eff0|C>
    = <psi|H|psi> to 1e-12 for the state's own bond matrix, H_eff0 Hermitian on two random vectors to 1e-13.  Two engines walk
    the chain together by non-optimising one-site moves: `move` goes first, `stay` keeps the centre one site behind and supplies
    H_eff1 with the same outer environments."""
    e = capped_state(ops, "SU2U1", L, chi, t=(1.0, 0.3), sweeps=sweeps) if case == "range2" else capped_state(ops, case, L, chi, sweeps=sweeps)
    dims = sector_dims(e)
    print(case, "sector dimensions of the inner bonds:", sorted(set(dims)))
    assert 1 in dims and any(n % 16 for n in dims if n > 1) and len(set(dims)) > 2 and max(dims) > wider_than
    E = stored_energy(e)
    stay, move = e.copy(), e.copy()
    for x in (stay, move):
        x.chi_full, x.cutoff = None, 0.0
    rng = np.random.default_rng(11)
    worst = {"identity": 0.0, "energy": 0.0, "herm": 0.0}
    steps = [(i, +1) for i in range(L - 1)] + [(i, -1) for i in range(L - 1, 0, -1)]
    for i, d in steps:
        assert stay.centre() == i == move.centre()
        cen = stay.download_site(i)
        move.update_site(i, d, optimise=False, record=False)
        b = i + 1 if d > 0 else i
        Q = move.download_site(i)
        n0 = move.bond_size(b)
        secs = bond_secs(move, b)
        assert n0 == sum(n * n for _, n in secs)
        xr = unpack_bond(move, b, rng.normal(size=n0) + 1j * rng.normal(size=n0))
        got = move.apply_heff0(b, pack_bond(move, b, xr))
        ref = pack_bond(move, b, heff0_through_heff1(stay, Q, i, d, xr))
        worst["identity"] = max(worst["identity"], np.linalg.norm(got - ref) / np.linalg.norm(ref))
        # the state's own bond matrix: C = Q^H centre
        Cm = {c: np.zeros((n, n), dtype=np.complex128) for c, n in secs}
        for k in Q:
            if d > 0:
                Cm[k[2]] += Q[k].conj().T @ cen[k]
            else:
                Cm[k[0]] += cen[k] @ Q[k].conj().T
        cv = pack_bond(move, b, Cm)
        assert abs(np.linalg.norm(cv) - 1.0) <= 1e-12
        worst["energy"] = max(worst["energy"], abs(np.vdot(cv, move.apply_heff0(b, cv)) - E) / max(abs(E), 1.0))
        yv = rng.normal(size=n0) + 1j * rng.normal(size=n0)
        xv = pack_bond(move, b, xr)
        Hy = move.apply_heff0(b, yv)
        hnorm = max(np.linalg.norm(got) / np.linalg.norm(xv), np.linalg.norm(Hy) / np.linalg.norm(yv))
        worst["herm"] = max(worst["herm"], abs(np.vdot(xv, Hy) - np.conj(np.vdot(yv, got))) /
                            (hnorm * np.linalg.norm(xv) * np.linalg.norm(yv)))
        stay.update_site(i, d, optimise=False, record=False)
    print(case, "H_eff0: worst identity / energy / Hermiticity errors over", len(steps), "bond visits:", worst)
    assert worst["identity"] <= 1e-12 and worst["energy"] <= 1e-12 and worst["herm"] <= 1e-13
    return worst


def quenched(ops, L=10, chi=20, tol=1e-12):
    """the capped ground state of U = 4 under the Hamiltonian U = 1"""
    e = capped_state(ops, "SU2U1", L, chi)
    e.set_mpo(model("SU2U1", L, (1.0,), 1.0)[0])
    e.krylovdim, e.lanczos_tol = 30, tol
    return e


def body_conservation(ops, sweeps=20, dt=0.05):
    """test 2: 20 one-site sweeps after the quench at a cap of 20: energy, norm, bond tables; TDVP2 at the same cap is printed"""
    e = quenched(ops)
    two = e.copy()
    before = tables(e)
    E0 = stored_energy(e)
    drift = lognorm = 0.0
    for k in range(sweeps):
        n0 = len(e.stats)
        Es = e.tdvp1_sweep(dt)
        recs = e.stats[n0:]
        assert len(recs) == 2 * e.L - 2 and all(s.trunc_weight == 0.0 and s.jacobi_sweeps == 0 for s in recs)
        assert all(s.n_matvec >= 2 for s in recs)
        drift = max(drift, abs(Es - E0))
        lognorm = max(lognorm, abs(e.log_norm))
    drift = max(drift, abs(stored_energy(e) - E0))
    tw = 0.0
    for k in range(sweeps):
        n0 = len(two.stats)
        two.tdvp_sweep(dt)
        tw += sum(s.trunc_weight for s in two.stats[n0:])
    print("one-site: energy drift", drift, "max |log_norm|", lognorm, "| two-site at the same cap: drift",
          abs(stored_energy(two) - E0), "discarded weight", tw)
    assert drift <= 1e-9 and lognorm <= 1e-10
    assert tables(e) == before and e.centre() == 0
    return drift, lognorm


def body_reversibility(ops):
    """test 3: +dt then -dt on the capped chain returns the state"""
    e = quenched(ops)
    psi0 = e.copy()
    e.tdvp1_sweep(0.05)
    mid = abs(psi0.overlap(e))
    e.tdvp1_sweep(-0.05)
    ov = abs(psi0.overlap(e))
    print("reversibility: |<psi0|psi>| after +dt", mid, "after -dt", ov, "1 - ov", 1.0 - ov)
    assert mid < 1.0 - 1e-6                     # (the step did move the state)
    assert 1.0 - ov <= 1e-10
    return 1.0 - ov


# Errors of one-site TDVP against dense ED at T = 0.5 on the L = 6, N = 4 quench (U = 4 -> U = 1, t2 = 0.3) with full bond tables,
# measured on the CPU baseline library: max over the (n_i, d_i) profiles and the Loschmidt amplitude.  The gate of every library
# is 2 x the dt = 0.025 value (rounding and solver-path differences) and a ratio >= 3 between successive step sizes.
CPU_ED_ERRORS = {0.1: 4.54e-07, 0.05: 1.13e-07, 0.025: 2.83e-08}


class OracleED:
    """the quench in one (N_up, N_dn) sector on oracle/ed.py's sparse Hamiltonian, made dense: the ground state of (t0, U0) evolved
    by (t1, U1); profiles (n_i, d_i) and the Loschmidt amplitude at time T"""

    def __init__(self, L, n_up, n_dn, t0, U0, t1, U1):
        from oracle import ed
        s0, s1 = ed.SectorED(L, n_up, n_dn, t0, [U0]), ed.SectorED(L, n_up, n_dn, t1, [U1])
        self.psi0 = np.linalg.eigh(s0.hamiltonian().toarray())[1][:, 0].astype(np.complex128)
        self.w, self.v = np.linalg.eigh(s1.hamiltonian().toarray())
        ou = np.array([[(b >> i) & 1 for i in range(L)] for b in s1.up], dtype=float)
        od = np.array([[(b >> i) & 1 for i in range(L)] for b in s1.dn], dtype=float)
        self.n = (ou[:, None, :] + od[None, :, :]).reshape(-1, L)           # basis index = i_up * n_dn + i_dn (kron(H_up, 1))
        self.d = (ou[:, None, :] * od[None, :, :]).reshape(-1, L)

    def at(self, T):
        psi = self.v @ (np.exp(-1j * T * self.w) * (self.v.conj().T @ self.psi0))
        p = np.abs(psi) ** 2
        return p @ self.n, p @ self.d, np.vdot(self.psi0, psi)


def ed_errors(ops, T=0.5):
    """test 4's measurement: {dt: max error of the (n_i, d_i) profiles and of the Loschmidt amplitude at time T}"""
    n_ref, d_ref, echo = OracleED(6, 2, 2, [1.0], 4.0, [1.0, 0.3], 1.0).at(T)
    errs = {}
    for dt in (0.1, 0.05, 0.025):
        e = tc.quench_state(ops)
        e.tdvp_sweep(0.0)                   # the bond tables of the full space: one untruncated two-site sweep of length 0
        psi0 = e.copy()
        for _ in range(int(round(T / dt))):
            e.tdvp1_sweep(dt)
        n, d = e.site_occupations()
        errs[dt] = max(np.abs(n - n_ref).max(), np.abs(d - d_ref).max(), abs(psi0.overlap(e) - echo))
    return errs


def check_ed_errors(errs):
    """test 4's gate: the errors sit above the 1e-9 solver floor, so the splitting is second order -- err(dt) / err(dt / 2) >= 3
    for both pairs -- and the finest step is within 2 x the value measured on the CPU baseline library"""
    print("one-site TDVP against ED at T = 0.5:", {k: float(v) for k, v in errs.items()}, "| CPU baseline:", CPU_ED_ERRORS)
    assert all(v > 1e-9 for v in CPU_ED_ERRORS.values())
    assert errs[0.1] / errs[0.05] >= 3.0 and errs[0.05] / errs[0.025] >= 3.0, errs
    assert errs[0.025] <= 2.0 * CPU_ED_ERRORS[0.025], errs


def body_imaginary_time(ops):
    """test 5: 60 sweeps of dt = -0.2i on the capped chain from its grown state reach the energy sweep1() converges to on the
    same tables; the state stays normalised.  log_norm: d/d beta log |exp(-beta H) psi| = -<H>, so a sweep's log_norm has the
    sign of -E -- POSITIVE on this chain, whose energy is negative -- and at the fixed point, where every local solve acts on an
    eigenvector (L forward half steps of both kinds against L - 1 backward ones), it equals 0.2 x (-E): asserted to 1e-6."""
    e = capped_state(ops)
    ref = e.copy()
    ref.krylovdim, ref.lanczos_tol = 30, 1e-13
    E1 = None
    for _ in range(30):
        E = ref.sweep1()
        if E1 is not None and abs(E - E1) < 1e-12:
            break
        E1 = E
    E1 = E
    before = tables(e)
    total = 0.0
    for k in range(60):
        Es = e.tdvp1_sweep(-0.2j)
        assert np.isfinite(e.log_norm) and e.log_norm * Es < 0.0, (k, e.log_norm, Es)
        total += e.log_norm
    assert abs(e.log_norm + 0.2 * Es) <= 1e-6 * abs(0.2 * Es), (e.log_norm, Es)
    Ef = stored_energy(e)
    nrm = abs(e.copy().overlap(e))
    print("imaginary time: E", repr(Ef), "one-site DMRG on the same tables", repr(E1), "diff", Ef - E1, "norm", nrm, "log_norm sum", total)
    assert abs(Ef - E1) <= 1e-8
    assert abs(nrm - 1.0) <= 1e-12 and tables(e) == before
    return Ef - E1


def body_api(ops, ed_error):
    """test 6: the TDVP selector through timestep / time_evolve / greens_function, the hand-over from TDVP2, the refusals.
    ed_error: the dt = 0.05 error of test 4 on this library (the bar of the greens_function comparison)"""
    import pytest
    from hubbardtn_amd import api
    L = 10
    e = capped_state(ops)
    psi = api.FiniteMPS(e, L)
    H1 = model("SU2U1", L, (1.0,), 1.0)[0]
    times = [0.0, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3]
    a = api.time_evolve(psi, H1, times[:3], api.TDVP2(api.truncdim(20), tol=1e-12))
    tabs = tables(e)
    b = api.time_evolve(psi, H1, times[2:], api.TDVP(tol=1e-12))
    for out, n in ((a, 3), (b, 5)):
        assert set(out) == {"times", "energy", "density_state", "double_occupancy", "loschmidt", "trunc_weight"}
        assert out["energy"].shape == (n,) and out["density_state"].shape == (n, L) and out["trunc_weight"].shape == (n,)
    assert a["trunc_weight"][1:].min() > 0.0                                  # (the cap binds: the two-site part does truncate)
    assert np.all(b["trunc_weight"] == 0.0)
    print("hand-over: energies", a["energy"], b["energy"], "spread after the hand-over", np.ptp(b["energy"]))
    assert np.ptp(b["energy"]) <= 1e-9 and abs(b["energy"][0] - a["energy"][-1]) <= 1e-9
    assert tables(e) == tabs and e.mpo is H1 and e.krylovdim == 30 and e.maxrestart == 8 and e.chi_full == 20
    psi2, envs = api.timestep(psi, None, 0.05, api.TDVP())
    assert psi2 is psi and envs.engine is e and tables(e) == tabs and e.lanczos_tol == 1e-10
    seen = api.time_evolve(psi, None, [0.0, 0.05], api.TDVP(), observe=lambda p, t: (t, p is psi))
    assert seen == [(0.0, True), (0.05, True)]
    # G(x, t) at L = 6: one-site against two-site TDVP without truncation.  The operator is 1 + n_site: the applied state lives
    # in the sector of psi0 and keeps ALL of psi0's bond tables, which are full, so the one-site run differs from the exact
    # two-site one by its splitting error only.  apply_op drops the sectors an operator annihilates ("n": no electron left of
    # the bond) or moves the state to another sector ("c+"); the tables of such an applied state are not those of the full
    # space, one-site evolution stays inside them whatever the step, and the result carries that projection error: printed
    # (8.4e-3 and 8.9e-3 on the CPU baseline library), not asserted, stated in README "Limits".
    g = tc.ground_state(ops, 6, (4, 0), [1.0], 4.0)
    gpsi = api.FiniteMPS(g, 6)
    gt = [0.0, 0.05, 0.1, 0.15, 0.2]
    ident, dens, op1 = g._site_op("id"), g._site_op("n"), abi.SiteOp()
    op1.k, op1.dN = dens.k, dens.dN
    op1.red[:] = [a + b for a, b in zip(ident.red, dens.red)]
    two = api.greens_function(gpsi, None, gt, api.TDVP2(tol=1e-12), op=op1)
    one = api.greens_function(gpsi, None, gt, api.TDVP(tol=1e-12), op=op1)
    diff = np.abs(two["C"] - one["C"]).max()
    print("greens_function, op = 1 + n: max |C_TDVP - C_TDVP2|", diff, "bar", ed_error)
    assert set(one) == set(two) and np.all(one["trunc_weight"] == 0.0)
    assert np.abs(two["C"][1:] - two["C"][0]).max() > 1e-3 and diff <= ed_error
    for name in ("n", "c+"):
        p2 = api.greens_function(gpsi, None, gt, api.TDVP2(tol=1e-12), op=name)
        p1 = api.greens_function(gpsi, None, gt, api.TDVP(tol=1e-12), op=name)
        print("greens_function, op =", name, "(pruned tables, not asserted): max |C_TDVP - C_TDVP2|", np.abs(p2["C"] - p1["C"]).max())
    with pytest.raises(NotImplementedError):
        api.timestep(api.InfiniteMPS(8), None, 0.1, api.TDVP())
    with pytest.raises(TypeError):
        api.timestep(psi, None, 0.1, api.DMRG())
    other = e.copy()
    e.set_orthogonal([other])
    with pytest.raises(abi.HtnError, match="attached orthogonal states"):
        api.timestep(psi, None, 0.05, api.TDVP())
    e.set_orthogonal([])
    with pytest.raises(abi.HtnError, match="krylovdim"):
        api.timestep(psi, None, 0.05, api.TDVP(krylovdim=40))
    # a block with fewer rows than columns, built by hand: bond 1 wider than site 0 can support
    bonds = [{(0, 0): 1}, {(1, 1): 3}, {(2, 0): 1}]
    tens = [{((0, 0), 1, (1, 1)): np.ones((1, 3)) / np.sqrt(3)}, {((1, 1), 1, (2, 0)): np.eye(3, 1) * np.sqrt(1.0)}]
    wide = engine.DMRG2(ops, models.hamiltonian(models.OB_Sim([1.0], [4.0]), 2), bonds, tens)
    with pytest.raises(abi.HtnError, match="run a two-site sweep first"):
        api.timestep(api.FiniteMPS(wide, 2), None, 0.05, api.TDVP())


NEW_SYMBOLS = ["htn_mps_bond_size", "htn_heff0_apply", "htn_site_evolve_move", "htn_tdvp1_sweep"]


def body_abi(ops, lib):
    """test 7: the four entry points, the version both sides agree on, and a refused sweep that leaves the state alone"""
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in abi.ENGINE_EXPORTS, n
    assert lib.htn_abi_version() == abi.ABI_VERSION
    e = capped_state(ops, L=6, chi=12, sweeps=2)
    e.move_centre(2)
    sites = [e.site_vector(i).copy() for i in range(e.L)]
    E, lg = C.c_double(7.0), C.c_double(7.0)
    o = e._opts()
    assert lib.htn_tdvp1_sweep(e.handle, 0.05, 0.0, C.byref(o), None, C.byref(E), C.byref(lg)) != 0
    assert b"centre is on site 2" in lib.htn_last_error()
    assert e.centre() == 2 and all(np.array_equal(a, e.site_vector(i)) for i, a in enumerate(sites))
    assert lib.htn_mps_bond_size(e.handle, -1) == -1 and lib.htn_mps_bond_size(e.handle, 3) == sum(n * n for n in e.bond(3).dims.values())
    with np.testing.assert_raises(abi.HtnError):
        e.apply_heff0(5, np.zeros(e.bond_size(5), dtype=np.complex128))          # (the centre is not next to bond 5)
    e.move_centre(0)
    st = e.evolve_site_move(0, +1, 0.025, -0.025)
    assert e.centre() == 1 and st.bond == 1 and st.direction == 1 and st.trunc_weight == 0.0 and st.n_matvec >= 2
    with np.testing.assert_raises(abi.HtnError):
        e.evolve_site_move(1, 0, 0.025, -0.025)
