"""Shared by test_variance_cpu.py / test_variance_gpu.py: the two-site energy variance (htn_mps_variance) against the dense
||(H - E) psi||^2 of small chains, and the null-space projection kernel (htn_block_nullproj_z) against numpy.

Dense reference: psi from excited_common.dense_state (all 2J+1 components of the total multiplet, the norm the library
normalises to 1), H from oracle.ed.dense_hamiltonian with the parameters of excited_common.model; both use the Jordan-Wigner
product basis with site 1 most significant."""
import ctypes as C

import numpy as np
import pytest

import excited_common as xc
from hubbardtn_amd import abi, api, engine, models, mps
from oracle import ed

L = 6
KINDS = ("SU2U1", "U1U1", "SU2")
MU = {"SU2U1": 0.0, "U1U1": 0.0, "SU2": 2.0}          # chemical potential of excited_common.model per kind
# The cut of the exactness and lower-bound tests: truncdim(8) in one two-site sweep after the state has grown to full dimension.
# Chosen on the CPU baseline library: total = 5.1e-2 (SU2U1, SU2), 4.7e-2 (U1U1) for t = [1], and for t = [1, 0.5]
# dense - total = 2.2e-3 / 1.8e-3, i.e. > 1e6 x the bar.
CUT = 8
# max |total - dense| of the exactness test measured on the CPU baseline library: 1.3e-16.  The bar is
# max(10 x that, 1e-12 ||H||^2) = 1e-12 ||H||^2 on both libraries (||H||_2^2 is 2e2 .. 1e3 here).
EXACT_CPU_DEV = 1.3e-16
# HIP against CPU library from the same uploaded L = 16, chi = 64 state, entry by entry; measured 2.4e-15 (entries up to 2e-2 of a state that is 0.18 from an eigenstate)
HIP_CPU_DEV = 2.4e-15


def hamiltonian(kind, t):
    if kind == "SU2U1":
        return models.hamiltonian(models.OB_Sim(t, [4.0]), L)
    if kind == "U1U1":
        return models.hamiltonian(models.OB_Sim(t, [4.0], 0.0, 1, 1, 2.0, 6, spin=True), L)
    return models.hamiltonian(models.OBC_Sim2(t, [4.0], 2.0), L)


_DENSE = {}


def dense_h(kind, t):
    """(dense H, ||H||_2^2), computed once per (kind, hopping) and shared"""
    key = (MU[kind], tuple(t))
    if key not in _DENSE:
        Hd = ed.dense_hamiltonian(L, list(t), [4.0], MU[kind])
        _DENSE[key] = (Hd, float(np.abs(np.linalg.eigvalsh(Hd)).max()) ** 2)
    return _DENSE[key]


def bar_of(kind, t):
    return max(10.0 * EXACT_CPU_DEV, 1e-12 * dense_h(kind, t)[1])


def grown_state(ops, kind, t=(1.0,), cut=CUT, sweeps=3):
    """two-site sweeps at full dimension, then (cut) one sweep at truncdim(cut); centre on site 0"""
    sym, _, target = xc.model(kind, L)
    H = hamiltonian(kind, list(t))
    bonds, tens = mps.random_mps(L, target, 4000, seed=3, sym=H.sym)
    eng = engine.DMRG2(ops, H, bonds, tens, chi_full=None, lanczos_tol=1e-13)
    for _ in range(sweeps):
        eng.sweep()
    if cut:
        eng.chi_full = cut
        eng.sweep()
        eng.chi_full = None
    return eng, H.sym


def dense_variance(eng, sym, kind, t, centre=None):
    """(||(H - E) psi||^2 / <psi|psi>, E) of the state as stored"""
    c = eng.centre() if centre is None else centre
    bonds = [dict(b.dims) for b in eng.bonds]
    psi = xc.dense_state(bonds, [eng.download_site(i) for i in range(L)], sym, centre=c)
    Hd = dense_h(kind, t)[0]
    n2 = float(np.vdot(psi, psi).real)
    E = float(np.vdot(psi, Hd @ psi).real) / n2
    r = Hd @ psi - E * psi
    return float(np.vdot(r, r).real) / n2, E


# ---- 1. exactness for an MPO of range 1, any centre position --------------------------------------------------------------
def check_exact(ops, kind):
    t = (1.0,)
    eng, sym = grown_state(ops, kind, t)
    ref, E = dense_variance(eng, sym, kind, t)
    bar = bar_of(kind, t)
    assert ref >= 1e-3, ref
    devs = []
    for c in (0, L // 2, L - 1):
        eng.move_centre(c)
        v = eng.variance()
        dev, dE = abs(v.total - ref), abs(v.energy - E)
        print("variance", kind, "centre", c, "total", v.total, "dense", ref, "dev", dev, "energy dev", dE, "bar", bar)
        devs.append(dev)
        assert v.total >= 1e-3 and eng.centre() == c
        assert dev <= bar and dE <= bar, (kind, c, dev, dE, bar)
        assert abs(v.total - (v.site.sum() + v.bond.sum())) <= 1e-15 and len(v.site) == L and len(v.bond) == L - 1
        assert (v.site >= 0.0).all() and (v.bond >= 0.0).all()
    return max(devs)


# ---- 2. lower bound for an MPO of range 2 -----------------------------------------------------------------------------------
def check_lower_bound(ops, kind):
    t = (1.0, 0.5)
    eng, sym = grown_state(ops, kind, t)
    ref, E = dense_variance(eng, sym, kind, t)
    bar = bar_of(kind, t)
    v = eng.variance()
    print("variance, range 2", kind, "total", v.total, "dense", ref, "dense - total", ref - v.total, "bar", bar)
    assert v.total <= ref + bar
    assert ref - v.total > 100.0 * bar
    assert abs(v.energy - E) <= bar


# ---- 3. an eigenstate ---------------------------------------------------------------------------------------------------------
def check_eigenstate(ops, kind):
    t = (1.0,)
    eng, sym = grown_state(ops, kind, t, cut=None, sweeps=6)
    ref, _ = dense_variance(eng, sym, kind, t)
    v = eng.variance()
    print("variance, eigenstate", kind, "total", v.total, "dense", ref)
    assert abs(v.total - ref) <= bar_of(kind, t)
    assert (v.site >= 0.0).all() and (v.bond >= 0.0).all()


# ---- 4. the state is untouched ------------------------------------------------------------------------------------------------
def check_untouched(ops, kind="SU2U1"):
    """the call puts the state's own buffers back: measured change of energy and overlap 0.0 on both libraries, so the bar
    (10 x the measured change) is 0 and the tensors are compared bit for bit"""
    eng, _ = grown_state(ops, kind)
    ref = eng.copy()                  # (a copy is taken with the centre on site 0)
    eng.move_centre(2)
    before = [eng.site_vector(i).copy() for i in range(L)]
    E0, ov0 = eng.energy, ref.overlap(eng)
    n_stats = len(eng.stats)
    v1 = eng.variance()
    assert eng.centre() == 2 and eng.energy == E0 and len(eng.stats) == n_stats
    assert ref.overlap(eng) == ov0 and abs(abs(ov0) - 1.0) <= 1e-12
    for i in range(L):
        assert np.array_equal(eng.site_vector(i), before[i]), i
    v2 = eng.variance()               # the planned call: same bits
    assert v2.total == v1.total and np.array_equal(v1.site, v2.site) and np.array_equal(v1.bond, v2.bond) and v1.energy == v2.energy
    eng.move_centre(0)
    Es, _ = eng.bond_energies()
    print("untouched", kind, "energy by a pass", Es, "variance energy", v1.energy)
    assert abs(Es - v1.energy) <= 1e-12 * max(1.0, abs(Es))


def check_cache_hygiene(ops):
    def sweep_misses(measure):
        eng, _ = grown_state(ops, "SU2U1", cut=None, sweeps=6)
        if measure:
            eng.variance()
        m0 = eng.cache_misses
        E = eng.sweep()
        return eng.cache_misses - m0, E
    (m_plain, E_plain), (m_meas, E_meas) = sweep_misses(False), sweep_misses(True)
    print("cache misses of the following sweep", m_plain, m_meas, "energies", E_plain, E_meas)
    assert m_meas == m_plain and E_plain == E_meas


# ---- 5. other inputs ----------------------------------------------------------------------------------------------------------
def check_applied(ops, kind="SU2U1"):
    """c+ on site 2 of the grown state: the variance of the NORMALISED applied state, centre where apply_op left it and on 0"""
    t = (1.0,)
    eng, sym = grown_state(ops, kind, t)
    work = eng.copy()
    work.move_centre(2)
    a = work.apply_op(2, "c+_up" if kind == "U1U1" else "c+")
    if kind == "U1U1":                                        # (<c_up c+_up> = 1 - n_up = 1/2 at half filling: a state that really
        assert abs(a.applied_norm2 - 1.0) > 1e-3              #  carries a norm; both spins together give 2 - n = 1)
    ref, E = dense_variance(a, sym, kind, t, centre=2)
    bar = bar_of(kind, t)
    for c in (2, 0):
        a.move_centre(c)
        v = a.variance()
        print("variance, applied state", kind, "centre", c, "norm2", a.applied_norm2, "total", v.total, "dense", ref, "dev", abs(v.total - ref))
        assert abs(v.total - ref) <= bar and abs(v.energy - E) <= bar
    assert abs(a.overlap(a) - a.applied_norm2) <= 1e-12 * a.applied_norm2


def check_refusals(ops, make_hooked_ops):
    eng, _ = grown_state(ops, "SU2U1", cut=None, sweeps=1)
    with pytest.raises(NotImplementedError, match="chain length"):
        api.energy_variance(api.InfiniteMPS(8))
    hooked = make_hooked_ops()
    hooked.set_exchange(0, 1, lambda y: None)
    b4, t4 = mps.random_mps(4, (4, 0), 8, seed=2)
    e2 = engine.DMRG2(hooked, models.hamiltonian(models.OB_Sim([1.0], [4.0]), 4), b4, t4)
    with pytest.raises(abi.HtnError, match="communicator or an exchange hook"):
        e2.variance()
    other, _ = grown_state(ops, "SU2U1", cut=None, sweeps=1)
    eng.set_orthogonal([other])
    with pytest.raises(abi.HtnError, match="attached orthogonal states"):
        eng.variance()
    eng.set_orthogonal([])
    v = api.energy_variance(api.FiniteMPS(eng, L))
    assert v.total >= 0.0 and abs(v.energy - eng.bond_energies()[0]) <= 1e-12
    # another Hamiltonian under the same state goes through set_mpo
    H2 = models.hamiltonian(models.OB_Sim([1.0], [6.0]), L)
    v2 = api.energy_variance(api.FiniteMPS(eng, L), H2)
    bonds = [dict(b.dims) for b in eng.bonds]
    psi = xc.dense_state(bonds, [eng.download_site(i) for i in range(L)], eng.sym, centre=eng.centre())
    Hd = ed.dense_hamiltonian(L, [1.0], [6.0], 0.0)
    E2 = float(np.vdot(psi, Hd @ psi).real)
    r = Hd @ psi - E2 * psi
    print("another Hamiltonian: energy", v2.energy, "dense", E2, "variance", v2.total, "dense", float(np.vdot(r, r).real))
    assert abs(v2.energy - v.energy) > 1e-3 and abs(v2.energy - E2) <= 1e-11 and abs(v2.total - float(np.vdot(r, r).real)) <= 1e-9


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
EPS = float(np.finfo(float).eps)


def _orthonormal(rng, rows, k):
    """rows x k, orthonormal columns to rounding"""
    if k == 0:
        return np.zeros((rows, 0), dtype=np.complex128)
    q, _ = np.linalg.qr(rng.standard_normal((rows, k)) + 1j * rng.standard_normal((rows, k)))
    return np.ascontiguousarray(q[:, :k])


def two_pass(R, Q, side, dtype=np.complex128):
    """the kernel's formula: -> (R after two projections, |W|^2 of the first pass, |R|^2 at the end)"""
    R, Q = R.astype(dtype), Q.astype(dtype)
    w2 = None
    for _ in range(2):
        if side == 0:
            W = Q.conj().T @ R
            R = R - Q @ W
        else:
            W = R @ Q.conj().T
            R = R - W @ Q
        if w2 is None:
            w2 = (np.abs(W) ** 2).sum()
    return R, w2, (np.abs(R) ** 2).sum()


class Case:
    def __init__(self, side, m, n, k, R, Q, name=""):
        self.side, self.m, self.n, self.k, self.R, self.Q, self.name = side, m, n, k, R, Q, name


def kernel_cases():
    """the shape list: m, n in {1, 15, 16, 17, 33} x k in {0, 1, 16, 17, min(m, n)} on both sides (k limited to the
    length of Q's orthonormal direction), a 530 x 40 block with k = 20, a 40 x 600 block with k = 130 on side 1, k = m on side 0"""
    rng = np.random.default_rng(7)
    out = []

    def add(side, m, n, k, name=""):
        R = rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n))
        Q = _orthonormal(rng, m, k) if side == 0 else _orthonormal(rng, n, k).conj().T.copy()
        out.append(Case(side, m, n, k, R, Q, name))
    for side in (0, 1):
        for m in (1, 15, 16, 17, 33):
            for n in (1, 15, 16, 17, 33):
                for k in sorted({0, 1, 16, 17, min(m, n)}):
                    if k <= (m if side == 0 else n):
                        add(side, m, n, k)
    add(0, 530, 40, 20, "530 x 40")
    add(1, 40, 600, 130, "40 x 600, rounds over k")
    add(0, 33, 17, 33, "k = m")
    return out


def pack(cases, seed=1):
    """one launch: every case its own result, uneven items, padded leading dimensions, NaN everywhere outside the views"""
    rng = np.random.default_rng(seed)
    items = np.zeros(len(cases), dtype=abi.NULLPROJ_DT)
    r_pos = q_pos = 3
    for q, c in enumerate(cases):
        ldr = c.m + int(rng.integers(0, 4))
        qr = c.k if c.side else c.m
        qc = c.n if c.side else c.k
        ldq = max(qr, 1) + int(rng.integers(0, 4))
        items[q] = (r_pos, q_pos, c.m, c.n, c.k, ldr, ldq, c.side, q, (0,) * 5)
        r_pos += ldr * c.n + int(rng.integers(0, 5))
        q_pos += ldq * qc + int(rng.integers(0, 5))
    Rb = np.full(r_pos + 3, np.nan + 1j * np.nan, dtype=np.complex128)
    Qb = np.full(q_pos + 3, np.nan + 1j * np.nan, dtype=np.complex128)
    mask = np.zeros(Rb.shape, dtype=bool)
    for it, c in zip(items, cases):
        idx = int(it["r_off"]) + np.arange(c.m)[:, None] + int(it["ldr"]) * np.arange(c.n)[None, :]
        Rb[idx] = c.R
        mask[idx] = True
        if c.k:
            qr, qc = c.Q.shape
            Qb[int(it["q_off"]) + np.arange(qr)[:, None] + int(it["ldq"]) * np.arange(qc)[None, :]] = c.Q
    return items, Rb, Qb, mask


def unpack(items, Rb, cases):
    return [Rb[int(it["r_off"]) + np.arange(c.m)[:, None] + int(it["ldr"]) * np.arange(c.n)[None, :]] for it, c in zip(items, cases)]


def check_kernel(run):
    """run(items, Rb, Qb, n_out) -> (Rb after, out[n_out, 2]).  Bar after qr_cases.py: max(10 x numpy's own deviation from a
    longdouble evaluation of the same formula, 256 eps), relative to |R| for R and to the value for the two norms.  Where Q spans
    the whole space (k = the length of its orthonormal direction) nothing is left: there the remainder and the square root of the
    emitted |R|^2 are bounded by bar x |R| instead."""
    cases = kernel_cases()
    items, Rb, Qb, mask = pack(cases)
    R1, out1 = run(items, Rb.copy(), Qb.copy(), len(cases))
    R2, out2 = run(items, Rb.copy(), Qb.copy(), len(cases))
    assert R1.tobytes() == R2.tobytes() and np.asarray(out1).tobytes() == np.asarray(out2).tobytes()      # two calls: the same bits
    assert np.isnan(R1[~mask]).all() and not np.isnan(R1[mask]).any()                                      # NaN outside the views untouched
    worst = 0.0
    for c, got, o in zip(cases, unpack(items, R1, cases), np.asarray(out1)):
        ref, w2, r2 = two_pass(c.R, c.Q, c.side)
        hi, w2h, r2h = two_pass(c.R, c.Q, c.side, np.clongdouble)
        nR = float(np.linalg.norm(c.R))
        own = float(np.linalg.norm((ref - hi).astype(np.complex128))) / nR
        bar = max(10.0 * own, 256 * EPS)
        dR = float(np.linalg.norm(got - hi.astype(np.complex128))) / nR
        worst = max(worst, dR / bar)
        assert dR <= bar, (c.name, c.side, c.m, c.n, c.k, dR, bar)
        full = c.k == (c.m if c.side == 0 else c.n)
        bw = max(10.0 * abs(w2 - float(w2h)) / max(float(w2h), 1e-300), 256 * EPS)
        assert abs(o[0] - float(w2h)) <= bw * float(w2h), (c.name, c.side, c.m, c.n, c.k, o[0], float(w2h))
        if full:
            assert np.sqrt(o[1]) <= bar * nR and float(np.linalg.norm(got)) <= bar * nR, (c.name, c.side, c.m, c.n, c.k, o[1])
        else:
            br = max(10.0 * abs(r2 - float(r2h)) / float(r2h), 256 * EPS)
            assert abs(o[1] - float(r2h)) <= br * float(r2h), (c.name, c.side, c.m, c.n, c.k, o[1], float(r2h))
        if c.k == 0:
            assert np.array_equal(got, c.R)
    print("nullproj: worst |R - R_longdouble| / bar over", len(cases), "cases:", worst)


def check_kernel_leak(run):
    """Q orthonormal only to 1e-12, R's component outside range(Q) = 1e-7 |R|: the emitted |R|^2 within 1e-6 of the exact
    remainder's (longdouble, projected until nothing moves).  One pass leaves about 1e-11 |R| of the removed part behind, 1e-4 of
    the remainder in norm; it lies inside range(Q), at right angles to the remainder, so it enters the squared norm squared:
    measured 2.3e-8 relative for one pass (printed below), 4e-12 for the two passes of the kernel."""
    rng = np.random.default_rng(11)
    for side, m, n, k in ((0, 200, 24, 60), (1, 24, 200, 60)):
        long_dim = m if side == 0 else n
        B = _orthonormal(rng, long_dim, k + 1)
        Qx, perp = B[:, :k], B[:, k:]                        # exact isometry and a unit vector outside its range
        Qp = Qx + 1e-12 * (rng.standard_normal(Qx.shape) + 1j * rng.standard_normal(Qx.shape))
        other = n if side == 0 else m
        coef = rng.standard_normal((k, other)) + 1j * rng.standard_normal((k, other))
        inside = Qx @ coef
        out_part = perp @ (rng.standard_normal((1, other)) + 1j * rng.standard_normal((1, other)))
        out_part *= 1e-7 * np.linalg.norm(inside) / np.linalg.norm(out_part)
        Rl = inside + out_part                               # long dimension first
        R = Rl if side == 0 else Rl.conj().T.copy()
        Q = Qp if side == 0 else Qp.conj().T.copy()
        hi = R.astype(np.clongdouble)
        Qh = Q.astype(np.clongdouble)
        for _ in range(4):
            hi = hi - Qh @ (Qh.conj().T @ hi) if side == 0 else hi - (hi @ Qh.conj().T) @ Qh
        exact = float((np.abs(hi) ** 2).sum())
        one = R - Q @ (Q.conj().T @ R) if side == 0 else R - (R @ Q.conj().T) @ Q
        one_pass = float((np.abs(one) ** 2).sum())
        c = Case(side, m, n, k, R, Q)
        items, Rb, Qb, _ = pack([c], seed=2)
        _, out = run(items, Rb, Qb, 1)
        rel = abs(out[0][1] - exact) / exact
        print("nullproj leak, side", side, "emitted", out[0][1], "exact", exact, "rel", rel, "one pass would give rel", abs(one_pass - exact) / exact)
        assert rel <= 1e-6, (side, rel)


def cpu_run(lib):
    def run(items, Rb, Qb, n_out):
        out = np.zeros((n_out, 2))
        rc = lib.htn_block_nullproj_z(Rb.ctypes.data, Qb.ctypes.data, items.ctypes.data, items.ctypes.data, len(items), out.ctypes.data,
                                      n_out, None, None)
        abi.check(lib, rc, "htn_block_nullproj_z")
        return Rb, out
    return run


def hip_run(ops):
    def run(items, Rb, Qb, n_out):
        Rd, Qd = ops.to_device(Rb), ops.to_device(Qb)
        out = ops.block_nullproj(Rd, Qd, items, n_out)
        ops.sync()
        return ops.to_host(Rd), ops.to_host(out)
    return run


def check_extrapolate():
    v = np.array([1e-3, 4e-4, 1e-4, 2e-5])
    r = api.extrapolate_energy(-3.5 + 2.0 * v, v)
    assert abs(r.E0 + 3.5) <= 1e-14 and abs(r.slope - 2.0) <= 1e-11 and r.residual <= 1e-14
    E0, slope, res = api.extrapolate_energy([1.0, 2.0, 2.0], [0.0, 1.0, 2.0])       # line 7/6 + x / 2, misfit (1, -2, 1) / 6
    assert abs(E0 - 7.0 / 6.0) <= 1e-15 and abs(slope - 0.5) <= 1e-15 and abs(res - np.sqrt(6.0) / 6.0) <= 1e-15
    with pytest.raises(ValueError):
        api.extrapolate_energy([1.0], [0.1])
    with pytest.raises(ValueError):
        api.extrapolate_energy([1.0, 2.0], [0.1, 0.1])
