"""Shared by test_tdvp_cpu.py / test_tdvp_gpu.py: dense exact diagonalisation of small Hubbard chains (numpy.kron, 4^L
states, L <= 6), exp(-i H t) by eigh, and the bodies of the two-site TDVP tests, which run on either library."""
import functools

import numpy as np

from hubbardtn_amd import abi, engine, models, mps

# ---- dense ED -------------------------------------------------------------------------------------------------------
_A = np.array([[0, 1], [0, 0]], dtype=np.int8)    # annihilator of one mode in the basis (empty, occupied)
_Z = np.array([[1, 0], [0, -1]], dtype=np.int8)
_I = np.eye(2, dtype=np.int8)


def _mode_op(L, k, a):
    """the operator `a` on mode k of 2L modes (site i: modes 2i = up, 2i + 1 = down) behind its Jordan-Wigner string"""
    out = np.ones((1, 1), dtype=np.int8)
    for q in range(2 * L):
        out = np.kron(out, _Z if q < k else (a if q == k else _I))
    return out


@functools.lru_cache(maxsize=None)
def operators(L):
    """(c[i][spin] as dense 4^L matrices of small integers, diagonals of n_up[i], n_dn[i])"""
    c = [[_mode_op(L, 2 * i + s, _A) for s in (0, 1)] for i in range(L)]
    nu = [np.abs(c[i][0]).sum(axis=0).astype(float) for i in range(L)]     # column j of c holds one entry iff the mode is occupied in j
    nd = [np.abs(c[i][1]).sum(axis=0).astype(float) for i in range(L)]
    return c, nu, nd


def sector(L, n_up, n_dn):
    """indices of the basis states with the given particle numbers"""
    _, nu, nd = operators(L)
    return np.where((np.abs(sum(nu) - n_up) < 0.5) & (np.abs(sum(nd) - n_dn) < 0.5))[0]


def dense_hubbard(L, t, U, idx=None):
    """H = - sum_r t[r-1] sum_{i, s} (c+_{i s} c_{i+r s} + h.c.) + U sum_i n_up n_dn on the open chain, restricted to the basis
    states idx (every term conserves both particle numbers; None: all 4^L states)"""
    c, nu, nd = operators(L)
    idx = np.arange(4 ** L) if idx is None else idx
    cols = {(i, s): c[i][s][:, idx].astype(float) for i in range(L) for s in (0, 1)}
    H = np.zeros((len(idx), len(idx)))
    for r, tr in enumerate(t, start=1):
        for i in range(L - r):
            for s in (0, 1):
                h = cols[(i, s)].T @ cols[(i + r, s)]
                H -= tr * (h + h.T)
    H += U * np.diag(sum(a[idx] * b[idx] for a, b in zip(nu, nd)))
    return H


class ED:
    """one (n_up, n_dn) sector: H0 prepares the state (its ground state), H1 evolves it"""

    def __init__(self, L, n_up, n_dn, t0, U0, t1=None, U1=None):
        self.L, self.idx = L, sector(L, n_up, n_dn)
        self.w0, v0 = np.linalg.eigh(dense_hubbard(L, t0, U0, self.idx))
        self.psi0 = v0[:, 0].astype(np.complex128)
        self.H1 = dense_hubbard(L, t0 if t1 is None else t1, U0 if U1 is None else U1, self.idx)
        self.w1, self.v1 = np.linalg.eigh(self.H1)
        _, nu, nd = operators(L)
        self.nu = [x[self.idx] for x in nu]
        self.nd = [x[self.idx] for x in nd]

    def evolve(self, T, psi=None):
        """exp(-i H1 T) psi (T complex: -i beta is imaginary time), not normalised"""
        psi = self.psi0 if psi is None else psi
        return self.v1 @ (np.exp(-1j * complex(T) * self.w1) * (self.v1.conj().T @ psi))

    def observe(self, psi):
        p = np.abs(psi) ** 2 / np.vdot(psi, psi).real
        n_up = np.array([p @ x for x in self.nu])
        n_dn = np.array([p @ x for x in self.nd])
        d = np.array([p @ (a * b) for a, b in zip(self.nu, self.nd)])
        E = (np.vdot(psi, self.H1 @ psi) / np.vdot(psi, psi)).real
        return E, n_up, n_dn, d


def singlet_levels(L, N, t, U):
    """ascending S = 0 levels at N electrons: the Sz = 0 spectrum with the Sz = 1 spectrum removed as a multiset"""
    def spec(a, b):
        return np.linalg.eigvalsh(dense_hubbard(L, t, U, sector(L, a, b)))
    lo, hi = list(spec(N // 2, N // 2)), list(spec(N // 2 + 1, N // 2 - 1))
    out, j = [], 0
    for x in lo:
        if j < len(hi) and abs(x - hi[j]) < 1e-9:
            j += 1
        else:
            out.append(x)
    assert j == len(hi)
    return np.array(out)


# ---- engines --------------------------------------------------------------------------------------------------------
def ham(L, t, U, spin=False):
    if spin:
        return models.hamiltonian(models.OB_Sim(list(t), [U], 0.0, 1, 1, 2.0, 6, spin=True), L)
    return models.hamiltonian(models.OB_Sim(list(t), [U]), L)


def ground_state(ops, L, target, t, U, sweeps=6, spin=False, seed=5, cap=64):
    """an untruncated engine converged by sweep(): the bond tables are full"""
    H = ham(L, t, U, spin)
    b, tn = mps.random_mps(L, target, cap, seed=seed, sym=H.sym)
    e = engine.DMRG2(ops, H, b, tn, krylovdim=20, lanczos_tol=1e-13, maxrestart=8)
    E_prev = None
    for _ in range(sweeps):
        E = e.sweep()
        if E_prev is not None and abs(E - E_prev) < 1e-13:
            break
        E_prev = E
    return e


def quench_state(ops, L=6, N=4, spin=False, target=None):
    """test 2's state: the ground state of U = 4, then the Hamiltonian U = 1, t2 = 0.3 under it; lanczos_tol = 1e-12"""
    e = ground_state(ops, L, (N, 0) if target is None else target, [1.0], 4.0, spin=spin)
    e.set_mpo(ham(L, [1.0, 0.3], 1.0, spin))
    e.krylovdim, e.lanczos_tol = 30, 1e-12
    return e


def stored_energy(e):
    """<psi|H|psi> of the state as stored (a non-optimising pass)"""
    return e.bond_energies()[0]


# ---- test bodies ----------------------------------------------------------------------------------------------------
def body_l2_exact(ops):
    """L = 2: one bond, no splitting error.  Quench U = 4 -> 8, ten sweeps of dt = 0.1: energy, double occupancy and the complex
    echo against dense ED to 1e-10"""
    ref = ED(2, 1, 1, [1.0], 4.0, U1=8.0)
    e = ground_state(ops, 2, (2, 0), [1.0], 4.0)
    psi0 = e.copy()
    e.set_mpo(ham(2, [1.0], 8.0))
    e.lanczos_tol = 1e-13
    worst = 0.0
    for k in range(1, 11):
        e.tdvp_sweep(0.1)
        E, _, _, d = ref.observe(ref.evolve(0.1 * k))
        echo = np.vdot(ref.psi0, ref.evolve(0.1 * k))
        n_got, d_got = e.site_occupations()
        errs = (abs(stored_energy(e) - E), np.abs(d_got - d).max(), abs(psi0.overlap(e) - echo), np.abs(n_got - 1.0).max())
        print("L=2 sweep", k, "errors E, d, echo, n:", errs)
        worst = max(worst, *errs)
    assert worst <= 1e-10
    return worst


def body_conservation(ops, L=6, N=4, spin=False, target=None, sweeps=20, dt=0.05):
    """quench at L = 6, N = 4: |E(t) - E(0)| <= 1e-8 over 20 untruncated sweeps, the density sums to N to 1e-12.
    -> (drift, trajectory of (energy, d_i, echo) per sweep)"""
    e = quench_state(ops, L, N, spin, target)
    psi0 = e.copy()
    E0 = stored_energy(e)
    drift, traj = 0.0, []
    for k in range(sweeps):
        Es = e.tdvp_sweep(dt)
        n, d = e.site_occupations()
        drift = max(drift, abs(Es - E0))
        traj.append((Es, d, psi0.overlap(e)))
        assert abs(n.sum() - (N if target is None else target[0])) <= 1e-12, n.sum()
        assert e.log_norm == 0.0 or abs(e.log_norm) <= 1e-10
    drift = max(drift, abs(stored_energy(e) - E0))
    print("energy drift over", sweeps, "sweeps:", drift)
    assert drift <= 1e-8
    return drift, traj


def body_reversibility(ops):
    """tdvp_sweep(+dt) then tdvp_sweep(-dt) returns the state of test 2 (nothing truncated: the composition is self-adjoint)"""
    e = quench_state(ops)
    psi0 = e.copy()
    E0 = stored_energy(e)
    e.tdvp_sweep(0.05)
    mid = abs(psi0.overlap(e))
    e.tdvp_sweep(-0.05)
    ov, E1 = abs(psi0.overlap(e)), stored_energy(e)
    print("reversibility: |<psi0|psi>| after +dt", mid, "after -dt", ov, "1 - ov", 1.0 - ov, "dE", abs(E1 - E0))
    assert mid < 1.0 - 1e-6                     # (the step did move the state)
    assert ov >= 1.0 - 1e-9 and abs(E1 - E0) <= 1e-9


def profile_error(e, ref, T, spin=False):
    psi = ref.evolve(T)
    _, nu, nd, d = ref.observe(psi)
    if spin:
        gu, gd = e.spin_occupations()
        return max(np.abs(gu - nu).max(), np.abs(gd - nd).max())
    n_got, d_got = e.site_occupations()
    return max(np.abs(n_got - (nu + nd)).max(), np.abs(d_got - d).max())


FLOOR = 1e-9        # what the solves (lanczos_tol = 1e-12 per exponential, some hundred of them) leave in a profile


def exact_check(errs):
    """Both step sizes must reproduce ED to the floor.  Why not a ratio: without truncation the bond tables of these chains are
    full after the first sweep, the two-site and the following one-site projector then act on the same space, the forward and
    backward steps cancel and two-site TDVP has NO step-size error -- measured on the CPU baseline library 3.4e-13 (dt = 0.1),
    2.7e-14 (0.05), 4.8e-14 (0.25), 2.0e-14 (0.125); with a bond cap (20, 12) the discarded weight (1e-5 .. 1e-3) swamps the
    splitting error instead.  A ratio of rounding errors says nothing, so the ORDER of the splitting is not tested anywhere
    (DESIGN.md section 4b); a wrong factor, sign or site in the sweep still shows here as an error of order dt."""
    print("step-size errors against ED:", errs)
    assert all(v <= FLOOR for v in errs.values()), errs


def body_second_order(ops):
    """same quench to T = 0.5 with dt = 0.1 and dt = 0.05 (and the coarser pair 0.25 / 0.125): the (n_i, d_i) profiles against ED"""
    ref = ED(6, 2, 2, [1.0], 4.0, t1=[1.0, 0.3], U1=1.0)
    errs = {}
    for dt, steps in ((0.25, 2), (0.125, 4), (0.1, 5), (0.05, 10)):
        e = quench_state(ops)
        for _ in range(steps):
            e.tdvp_sweep(dt)
        errs[dt] = profile_error(e, ref, 0.5)
    exact_check(errs)
    return errs


def body_imaginary_time(ops):
    """L = 6, random (N = 6, S = 0) state shaped by one sweep(), dt = -0.2i: E never rises, 60 sweeps reach the ED ground energy"""
    lv = singlet_levels(6, 6, [1.0], 4.0)
    gap = lv[1] - lv[0]
    beta = 0.2 * 60
    print("ED singlet levels", lv[:3], "gap", gap, "bound on the excited admixture", (lv[-1] - lv[0]) * np.exp(-2.0 * beta * gap))
    assert (lv[-1] - lv[0]) * np.exp(-2.0 * beta * gap) * 1e3 < 1e-6      # (1e3: a start with 0.1 % ground-state weight)
    H = ham(6, [1.0], 4.0)
    b, tn = mps.random_mps(6, (6, 0), 64, seed=11)
    e = engine.DMRG2(ops, H, b, tn, krylovdim=3, lanczos_tol=1e-1, maxrestart=0)
    e.sweep()
    e.krylovdim, e.lanczos_tol, e.maxrestart = 30, 1e-12, 8
    E_prev = stored_energy(e)
    assert E_prev > lv[0] + 1e-3                # (the start is not the answer)
    for k in range(60):
        E = e.tdvp_sweep(-0.2j)
        assert E <= E_prev + 1e-10, (k, E, E_prev)
        E_prev = E
    Ef = stored_energy(e)
    print("imaginary time: E", Ef, "ED", lv[0], "diff", Ef - lv[0])
    assert abs(Ef - lv[0]) <= 1e-6


def heff_matrix(e, i=0):
    """the two-site effective Hamiltonian of bond i as a dense matrix through apply_heff (L = 2: H in the state's sector)"""
    n = e.theta(i).shape[0]
    return np.stack([e.apply_heff(i, np.eye(n, dtype=np.complex128)[k]) for k in range(n)], axis=1)


def body_log_norm_l2(ops):
    """L = 2 is exact: the summed log_norm of imaginary-time sweeps against log |exp(-beta H) psi0|.  The sector's H comes from
    apply_heff on unit vectors; its spectrum is checked against the dense ED matrix first."""
    H = ham(2, [1.0], 4.0)
    b, tn = mps.random_mps(2, (2, 0), 8, seed=3)
    e = engine.DMRG2(ops, H, b, tn, krylovdim=8, lanczos_tol=1e-13, maxrestart=8)
    th0 = e.theta(0)
    Hm = heff_matrix(e)
    assert np.abs(Hm - Hm.conj().T).max() <= 1e-13
    w, v = np.linalg.eigh(Hm)
    full = np.linalg.eigvalsh(dense_hubbard(2, [1.0], 4.0))
    assert all(np.abs(full - x).min() <= 1e-12 for x in w) and len(w) == 3
    th0 = th0 / np.linalg.norm(th0)
    total = 0.0
    for k in range(1, 6):
        e.tdvp_sweep(-0.2j)
        total += e.log_norm
        ref = np.log(np.linalg.norm(v @ (np.exp(-0.2 * k * w) * (v.conj().T @ th0))))
        print("log norm after", k, "sweeps:", total, "ED", ref, "diff", abs(total - ref))
        assert abs(total - ref) <= 1e-6


def body_truncation(ops):
    """L = 8, chi_full = 40, real time: the discarded weight is reported and positive from some sweep on, the cap holds, and the
    energy drift stays below (sum of discarded weights) x scale.  Scale: the spectral width of H is at most twice
    sum_r |t_r| x 2 (spins) x (bonds of range r) x |c+c + h.c.| <= 2 + U L, which bounds |<a|H|b>| for normalised a, b."""
    L = 8
    e = ground_state(ops, L, (8, 0), [1.0], 4.0, sweeps=4)
    e.set_mpo(ham(L, [1.0, 0.3], 1.0))
    e.krylovdim, e.lanczos_tol, e.chi_full = 30, 1e-10, 40
    e.svd_cut(40)
    E0 = stored_energy(e)
    scale = 2.0 * (2 * 2 * (1.0 * (L - 1) + 0.3 * (L - 2)) + 1.0 * L)
    tw_sum, seen = 0.0, False
    for k in range(8):
        n0 = len(e.stats)
        e.tdvp_sweep(0.1)
        tw = sum(s.trunc_weight for s in e.stats[n0:])
        assert all(s.trunc_weight >= -1e-14 for s in e.stats[n0:])
        seen = seen or tw > 1e-12
        if seen:
            assert tw > 1e-12
        tw_sum += tw
        assert max(e.bond_dims()) <= 40
        drift = abs(stored_energy(e) - E0)
        print("truncation sweep", k, "discarded", tw, "sum", tw_sum, "drift", drift, "bound", tw_sum * scale)
        assert drift <= tw_sum * scale + 1e-8
    assert seen


def body_spinful(ops):
    """U(1) x U(1) mode, L = 4, N_up = 2, N_dn = 1: conservation as in test 2, the (n_up, n_dn) profile against ED"""
    drift, _ = body_conservation(ops, L=4, N=3, spin=True, target=(3, 1), sweeps=20)
    ref = ED(4, 2, 1, [1.0], 4.0, t1=[1.0, 0.3], U1=1.0)
    errs = {}
    for dt, steps in ((0.1, 5), (0.05, 10)):
        e = quench_state(ops, 4, 3, True, (3, 1))
        for _ in range(steps):
            e.tdvp_sweep(dt)
        errs[dt] = profile_error(e, ref, 0.5, spin=True)
    print("spinful: drift", drift)
    exact_check(errs)
    return errs


def body_refusals(ops, with_exchange=True):
    e = ground_state(ops, 4, (4, 0), [1.0], 4.0, sweeps=2)
    other = e.copy()

    def refused(fn, word):
        try:
            fn()
        except abi.HtnError as ex:
            assert word in str(ex), str(ex)
        else:
            raise AssertionError("not refused: " + word)
    e.set_orthogonal([other])
    refused(lambda: e.tdvp_sweep(0.1), "attached")
    refused(lambda: e.evolve_bond(0, +1, "right", 0.1), "attached")
    e.set_orthogonal([])
    refused(lambda: e.set_mpo(ham(6, [1.0], 4.0)), "sites")
    e.krylovdim = 40
    refused(lambda: e.tdvp_sweep(0.1), "krylovdim")
    refused(lambda: e.evolve_site(0, 0.1), "krylovdim")
    e.krylovdim = 20
    refused(lambda: e.evolve_site(2, 0.1), "centre")
    E = e.tdvp_sweep(0.1)                       # and after all refusals the state still evolves
    assert np.isfinite(E) and e.centre() == 0
    if with_exchange:
        ops.set_exchange(0, 1, lambda *a: None)          # (an exchange hook makes the context a sharded one)
        try:
            refused(lambda: e.tdvp_sweep(0.1), "communicator")
        finally:
            ops.set_exchange(0, 1, None)


def body_api_time_evolve(ops):
    """api.time_evolve / api.timestep on the L = 2 quench (exact): the default record against ED at every time, observe= gets
    every time, a truncating scheme reports its discarded weight, and H = the current Hamiltonian does not quench again"""
    import pytest
    from hubbardtn_amd import api
    ref = ED(2, 1, 1, [1.0], 4.0, U1=8.0)
    e = ground_state(ops, 2, (2, 0), [1.0], 4.0)
    psi = api.FiniteMPS(e, 2)
    H1 = ham(2, [1.0], 8.0)
    times = [0.0, 0.1, 0.2, 0.3]
    out = api.time_evolve(psi, H1, times, api.TDVP2(tol=1e-13))
    assert e.mpo is H1 and e.krylovdim == 30 and e.maxrestart == 8
    for k, t in enumerate(times):
        E, nu, nd, d = ref.observe(ref.evolve(t))
        assert abs(out["energy"][k] - E) <= 1e-10 and np.abs(out["double_occupancy"][k] - d).max() <= 1e-10
        assert abs(out["loschmidt"][k] - np.vdot(ref.psi0, ref.evolve(t))) <= 1e-10
        assert np.abs(out["density_state"][k] - (nu + nd)).max() <= 1e-10
    assert out["trunc_weight"].shape == (4,) and np.abs(out["trunc_weight"]).max() <= 1e-14
    handle = e.cmpo
    seen = api.time_evolve(psi, H1, [0.3, 0.4], api.TDVP2(), observe=lambda p, t: (t, p is psi))
    assert seen == [(0.3, True), (0.4, True)] and e.cmpo is handle          # same H: no second quench
    psi2, envs = api.timestep(psi, None, 0.1, api.TDVP2(trscheme=api.truncdim(2)))
    assert psi2 is psi and envs.engine is e and max(e.bond_dims()) <= 2
    assert sum(s.trunc_weight for s in e.stats[-2:]) > 1e-6                  # (dimension 3 cut to 2: something is discarded)
    with pytest.raises(NotImplementedError):
        api.timestep(api.InfiniteMPS(8), None, 0.1, api.TDVP2())
    with pytest.raises(TypeError):
        api.timestep(psi, None, 0.1, api.DMRG2())
