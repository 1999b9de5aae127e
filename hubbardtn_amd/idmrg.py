"""Infinite-chain two-site DMRG (the `IDMRG2` the reference calls at src/HubbardFunctions.jl:1010), SURVEY 8f.1.

MPSKit's IDMRG2 sweeps the sites of ONE unit cell with environments that grow by transfer at every pass
(no linear solve inside the loop) and stops on ||C_old - C_new|| < tol.  The same fixed point is reached here in
McCulloch's original formulation, which needs nothing but the finite-chain engine:

    system_n = [left block] + window of 2 T sites + [right block]              (T = unit cell, src:408-412)
    optimise the window by ordinary two-site sweeps (engine.DMRG2 with the blocks' environments as boundaries),
    absorb its left half into the left block, its right half into the right block  (= the environments at
    the window's centre bond, which the sweep has just produced), insert a fresh window, repeat.

Every step adds 2 T sites, so  e = (E_n - E_{n-1}) / (2 T)  is the energy per site and the change of the centre
Schmidt spectrum is the convergence measure (the ||dC|| of MPSKit; C is diagonal after the SVD).  All arithmetic
is the finite sweep's: H_eff apply, Lanczos, per-sector SVD, environment transfer -- the library's hot path.

Sector labels stay absolute (N = particles to the left of the bond): the left block's labels simply grow; the
right block's environment is re-keyed by the window's particle content 2 T P/Q when a window is inserted in front
of it (sorted block order, hence the flat buffer, is invariant under that shift).  The reference's shifted charge
k = N Q - P sites (src:251) is this relabelling done once and for all.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import abi
from . import engine as _engine
from . import models, mps


def unit_cell(P: int, Q: int) -> int:
    """T = Q if P even else 2 Q (src:408-412)"""
    return Q if P % 2 == 0 else 2 * Q


def cell_sites(sim) -> int:
    """sites per unit cell of the infinite chain: T B with T = Q or 2Q for the fixed-filling models (src:408-412,
    832-836); the chemical-potential models have T = 1 (src:417, 841) -- a one-band cell of ONE site is doubled here,
    because the growing window needs a bond inside each half"""
    B = int(sim.bands)
    if models.symmetry_of(sim).kind == 2:
        return max(B, 2)
    return unit_cell(int(sim.P), int(sim.Q)) * B


def reference_cell_sites(sim) -> int:
    """length(H) of the reference: T B with T = 1 for the chemical-potential models (src:417, 841)"""
    B = int(sim.bands)
    if models.symmetry_of(sim).kind == 2:
        return B
    return unit_cell(int(sim.P), int(sim.Q)) * B


def schmidt_cut_scale(sim) -> float:
    """factor between a Schmidt-value cut applied to the reference's state and the same cut applied here.
    Only the one-site unit cell of the chemical-potential one-band model differs (the branch src:1012-1022, VUMPS +
    SvdCut(truncbelow)): its uniform MPS carries BOTH sector families on every bond -- (even parity, integer spin) and
    (odd parity, half-integer spin), which one site translation maps onto each other -- as two blocks of equal weight 1/2,
    so its normalised Schmidt values are the family's values divided by sqrt 2.  The doubled cell used here (cell_sites)
    keeps ONE family per bond with weight 1: truncbelow(eta) on the reference's state keeps exactly the multiplets
    truncbelow(sqrt 2 eta) keeps here.  Inferred from the structure of the state, not verifiable without MPSKit; what can be
    checked is the reference's own constant: test/OBC.jl:20 (-1.03541433, atol 1e-3) is met at 7e-4 with the factor and
    missed (1.1e-3) without it (tests/test_nou1_cpu.py)."""
    return float(np.sqrt(2.0)) if cell_sites(sim) == 2 * reference_cell_sites(sim) else 1.0


def _spectrum_distance(a: dict, b: dict, dN: int, sym=models.SU2U1) -> float:
    """|| S_a - S_b || over sectors, b's labels shifted back by dN, shorter spectra zero padded"""
    keys = set(a) | {(N - dN, j) for (N, j) in b}
    d2 = 0.0
    for k in keys:
        x = np.asarray(a.get(k, []), dtype=float)
        y = np.asarray(b.get((k[0] + dN, k[1]), []), dtype=float)
        n = max(len(x), len(y))
        x = np.pad(x, (0, n - len(x)))
        y = np.pad(y, (0, n - len(y)))
        d2 += sym.qdim(k) * float(np.sum((x - y) ** 2))
    return float(np.sqrt(d2))


@dataclass
class IDMRGResult:
    energy_per_site: float
    delta: float                 # change of the centre Schmidt spectrum in the last step
    iterations: int
    unit_cell: int
    bond_dims: list              # TensorKit dims of the bonds inside the last window
    spectrum: dict               # centre Schmidt spectrum {sector: values} (absolute labels of the last window)
    history: list = field(default_factory=list)     # (energy per site, delta) per growth step
    engine: object = None        # the last window's engine (device-resident tensors of two unit cells)
    boundary: dict = field(default_factory=dict)    # bL, bR, Lenv, Renv of the last window (what storage needs to re-create it)
    sweeps: int = 0              # window sweeps run in total


def idmrg2(ops, sim, chi_full=None, cutoff=0.0, tol=1e-6, maxiter=100, sweeps_per_step=6, init_dimension=8,
           krylovdim=30, lanczos_tol=1e-10, seed=1234, verbosity=0, min_steps=3, warm_start=None, driver="python"):
    """-> IDMRGResult.  `sim` is an OB_Sim / MB_Sim (filling P/Q); truncation by truncdim(chi_full) and/or
    truncbelow(cutoff) exactly as in the finite engine.  warm_start: every window after the second starts from McCulloch's
    prediction built out of the previous window's halves (`_absorb`) instead of a random state.  Default: on for the
    SU(2)-symmetric modes; off for the spinful U(1) x U(1) mode, whose growth under a crude Schmidt cut has several
    self-consistent fixed points (symmetry-broken windows whose multiplets the cut has split) -- random restarts wander
    between them and find lower ones than a prediction that hands one of them on (two-band test/Spin.jl case: -0.61 against
    -0.55).
    driver: "python" runs the growth loop below over the finite engine; "native" runs the same rules inside the library
    (htn_idmrg_*: boundary environments and window tensors stay on the device between steps, `_native_idmrg2`)."""
    if driver not in ("python", "native"):
        raise ValueError(f"idmrg2: driver must be 'python' or 'native', not {driver!r}")
    P, Q = int(sim.P), int(sim.Q)
    B = int(sim.bands)
    sym = models.symmetry_of(sim)
    if warm_start is None:
        warm_start = sym.kind != 1
    T = cell_sites(sim)                      # sites per unit cell
    W = 2 * T
    dNw = (W * P) // Q                       # particles in a window (integer: the cell length is a multiple of Q)
    assert (W * P) % Q == 0
    # translation-invariant MPO sites from the bulk of a long open chain
    ncells = 8 * max(T // B, 1)
    big = models.hamiltonian(sim, ncells)
    m0 = 3 * T
    sites = [big[m0 + i] for i in range(W)]
    key = lambda w: (tuple(w.left), tuple(w.right), tuple(w.entries))
    assert key(big[m0]) == key(big[m0 + T]) == key(big[m0 + W]), "MPO is not periodic with the unit cell"
    cmpo = _engine.CMpo(ops, models.MPO(sites, sym))
    if driver == "native":
        return _native_idmrg2(ops, cmpo, sym, T, dNw, chi_full, cutoff, tol, maxiter, sweeps_per_step, init_dimension,
                              krylovdim, lanczos_tol, seed, verbosity, min_steps, warm_start)
    # step 0: the window alone.  Its MPO bonds are the bulk's (full width), so "open ends" are explicit boundary
    # environments: an empty chain to the left (only the implicit identity level is non-zero) and to the right
    bL = {(0, 0): 1}
    bR = {(sym.wrap(dNw), 0): 1}
    Lenv = _zero_env(bL, sites[0].left, "L", sym)
    Renv = _zero_env(bR, sites[W - 1].right, "R", sym)
    E_prev, spec_prev, e_site, delta = None, None, float("nan"), float("inf")
    history = []
    eng = None
    carry = {"sigma": {c: np.ones(n) for c, n in bL.items()}, "Ddag": {c: np.eye(n) for c, n in bL.items()}}
    guess = None
    n_sweeps = stall = 0
    for it in range(maxiter):
        warm = guess is not None
        if warm:
            bonds, tensors = guess
        else:
            bonds, tensors = mps.random_window(W, bL, bR, init_dimension, seed=seed + it, sym=sym)
        eng = _engine.DMRG2(ops, cmpo, bonds, tensors, chi_full=chi_full, cutoff=cutoff, krylovdim=krylovdim,
                            lanczos_tol=lanczos_tol, left_env=Lenv, right_env=Renv)
        boundary = {"bL": dict(bL), "bR": dict(bR), "Lenv": Lenv, "Renv": Renv}
        # the window starts from a random state: sweep until its energy has settled (at least twice, at most
        # sweeps_per_step times); a window that has not found its ground state poisons the blocks it is absorbed into
        E_sw = None
        for k in range(sweeps_per_step):
            E_new = eng.sweep()
            n_sweeps += 1
            # (a predicted window is 1e-6 from its ground state after one sweep and 1e-9 after two; the growth steps, not the
            # window sweeps, set the accuracy of the fixed point)
            if k >= 1 and E_sw is not None and abs(E_new - E_sw) <= (1e-8 if warm else 1e-11) * max(abs(E_new), 1.0):
                break
            E_sw = E_new
        # energy of system_n: <psi|H|psi> of the window state AS STORED (after the truncations of the last sweep),
        # evaluated at bond 0 without moving the centre -- not the pre-truncation Ritz value of an eigensolve, which is
        # biased low by the discarded weight (visible at the reference's truncbelow(1e-2))
        E = eng.update_bond(0, +1, "left", optimise=False, record=False, cutoff=0.0)
        spec = eng.spectrum(T)
        if E_prev is not None:
            e_site = (E - E_prev) / W
            delta = _spectrum_distance(spec_prev, spec, 0 if sym.kind == 2 else dNw // 2, sym)
        history.append((e_site, delta))
        if verbosity:
            print(f"IDMRG2 step {it + 1}: sites {W * (it + 1)}  E/site = {e_site:.10f}  delta = {delta:.3e}  "
                  f"chi = {eng.bond(T).dim_full}")
        E_prev, spec_prev = E, spec
        if (it + 1 >= min_steps and delta < tol) or it + 1 == maxiter:
            break                                    # (the last window stays as the sweeps left it: centre on site 0)
        # absorb the halves: environments at the centre bond become the new boundaries; the right block's bond is
        # relabelled N -> N + dNw (block order, hence the flat data, unchanged)
        # (each environment carries the bond table it was built on: the left one dates from the rightward pass, the
        # right one from the leftward pass, and truncdim may have kept different counts in between)
        if warm_start:
            Lenv, Renv, bL, bR, guess, carry = _absorb(eng, T, sym, dNw, carry)
            # a growth that neither converges nor moves (the spinful two-band model with the crude Schmidt cut can lock into
            # a poor, symmetry-broken window that the prediction then hands on unchanged) gets a random window again
            if len(history) >= 2 and delta > 10.0 * tol and abs(delta - history[-2][1]) <= 0.05 * delta:
                stall += 1
            else:
                stall = 0
            if it == 0 or stall >= 2:
                guess = None     # (it == 0: the isolated first window predicts a product of isolated windows: a two-site
                stall = 0        # sweep with a Schmidt cut can stay on it -- seen for two decoupled chains snaked onto one --
                                 # so the second window starts at random as well, prediction from the third on)
        else:
            Lenv, Renv = eng.env_data("L", T), eng.env_data("R", T)
            bL = dict(eng.env_bond("L", T).dims)
            bR = {(sym.wrap(N + dNw), j): n for (N, j), n in eng.env_bond("R", T).dims.items()}
    return IDMRGResult(energy_per_site=e_site, delta=delta, iterations=len(history), unit_cell=T,
                       bond_dims=eng.bond_dims(), spectrum=spec_prev, history=history, engine=eng, boundary=boundary,
                       sweeps=n_sweeps)


def _native_idmrg2(ops, cmpo, sym, T, dNw, chi_full, cutoff, tol, maxiter, sweeps_per_step, init_dimension, krylovdim,
                   lanczos_tol, seed, verbosity, min_steps, warm_start):
    """idmrg2's loop driven through the library's step-wise driver (htn_idmrg_*): the host only supplies the random
    windows the driver asks for (same seeds as the Python loop: seed + step) and reads the scalars of every step"""
    lib = ops.lib
    W = 2 * T
    kw = dict(chi_full=chi_full, cutoff=cutoff, krylovdim=krylovdim, lanczos_tol=lanczos_tol)
    o = abi.IdmrgOpts()
    o.sweep = _engine.sweep_opts(**kw)
    o.cell_sites, o.window_dN, o.tol = T, dNw, float(tol)
    o.min_steps, o.maxiter, o.sweeps_per_step, o.warm_start = int(min_steps), int(maxiter), int(sweeps_per_step), int(bool(warm_start))
    h = C.c_void_p()
    abi.check(lib, lib.htn_idmrg_create(ops.ctx, cmpo.handle, C.byref(o), C.byref(h)), "htn_idmrg_create")
    history, n_sweeps = [], 0
    try:
        st = abi.IdmrgStats()
        needs = True
        while True:
            it = len(history)
            if needs:
                bL, bR = boundary_table(lib, h, 0), boundary_table(lib, h, 1)
                bonds, tensors = mps.random_window(W, bL, bR, init_dimension, seed=seed + it, sym=sym)
                tab = _engine.state_tables(bonds, tensors)
                rc = lib.htn_idmrg_step(h, *tab.pointers(), C.byref(st))
            else:
                rc = lib.htn_idmrg_step(h, None, None, None, None, None, None, C.byref(st))
            chk = getattr(ops, "check_exchange", None)
            if chk is not None:
                chk()
            abi.check(lib, rc, "htn_idmrg_step")
            history.append((st.energy_per_site, st.delta))
            n_sweeps += st.sweeps
            if verbosity:
                print(f"IDMRG2 step {it + 1}: sites {W * (it + 1)}  E/site = {st.energy_per_site:.10f}  delta = {st.delta:.3e}  "
                      f"chi = {st.chi_full}")
            if st.finished:
                break
            needs = bool(st.needs_window)
        win = C.c_void_p()
        abi.check(lib, lib.htn_idmrg_window(h, C.byref(win)), "htn_idmrg_window")
    finally:
        lib.htn_idmrg_destroy(h)
    eng = _engine.DMRG2.wrap(ops, cmpo, win, **kw)
    eng.energy = st.energy
    boundary = {"bL": dict(eng.bond(0).dims), "bR": dict(eng.bond(W).dims), "Lenv": eng.env_data("L", 0),
                "Renv": eng.env_data("R", W)}
    return IDMRGResult(energy_per_site=st.energy_per_site, delta=st.delta, iterations=len(history), unit_cell=T,
                       bond_dims=eng.bond_dims(), spectrum=eng.spectrum(T), history=history, engine=eng, boundary=boundary,
                       sweeps=n_sweeps)


def boundary_table(lib, handle, side) -> dict:
    """{sector: count} the next window of an htn_idmrg driver must have at its left (0) / right (1) end"""
    n = lib.htn_idmrg_boundary(handle, side, None)
    if n < 0:
        raise abi.HtnError("htn_idmrg_boundary: bad argument")
    arr = np.zeros(max(n, 1), dtype=abi.SECTOR_DT)
    lib.htn_idmrg_boundary(handle, side, arr.ctypes.data)
    return {(int(r["N"]), int(r["j"])): int(r["count"]) for r in arr[:n]}


def _absorb(eng, T, sym, dNw, carry):
    """Absorb the halves of a converged window and predict the next one (McCulloch, arXiv:0804.2509 sec. II.C).

    The window (sites 0 .. 2T-1, centre on site 0) is brought ONCE into the mixed form  A_0 .. A_{T-1} sigma B'_T .. B_{2T-1}
    by non-optimising moves: rightwards to the centre bond T (fresh left environment, A's and B'_T = the PAIRED Schmidt
    bases of bond T), one move back ('left' placement: fresh right environment; its SVD re-chooses the basis, B''_T =
    D^H B'_T with a unitary D per sector, recovered from the two tensors).  Boundaries of the next window: the left
    environment in the paired gauge, the right one in the B'' gauge.  Its trial state

        [sigma B'_T] B_{T+1} .. B_{2T-1}  .  [D_prev^H sigma_0^-1 A_0 sigma_1] .. [sigma_{T-1}^-1 A_{T-1} sigma_T D]

    reuses the right half as the new left half and the left half, turned into right-canonical form by the Schmidt values
    of its own bonds (sigma_0 = the previous step's centre values), as the new right half; labels of the latter move by
    one window (dNw particles).  All sigma are singular values in the library's Euclidean normalisation (Schmidt value
    times sqrt(2S+1)).  -> (Lenv, Renv, bL, bR, (bonds, tensors) or None, carry for the next call)."""
    W = 2 * T
    kw = dict(optimise=False, record=False)              # (the run's own truncation: the state already satisfies it)
    tilde = lambda spec: {c: np.asarray(v, dtype=float) * np.sqrt(sym.qdim(c)) for c, v in spec.items()}
    sh = lambda c: (sym.wrap(c[0] + dNw), c[1])
    for i in range(T):                                   # centre 0 -> T
        eng.update_bond(i, +1, "right", **kw)
    A = [eng.download_site(k) for k in range(T)]
    sig = [carry["sigma"] if carry else None] + [tilde(eng.spectrum(k)) for k in range(1, T + 1)]
    CT = eng.download_site(T)                            # sigma_T B'_T
    Bs = {k: eng.download_site(k) for k in range(T + 1, W)}
    Lenv, bL = eng.env_data("L", T), dict(eng.env_bond("L", T).dims)
    ob = [dict(b.dims) for b in eng.bonds]
    eng.update_bond(T - 1, +1, "left", **kw)             # centre back to T-1: B''_T and the right environment on bond T
    B2 = eng.download_site(T)
    Renv, bRt = eng.env_data("R", T), dict(eng.env_bond("R", T).dims)
    bR = {sh(c): n for c, n in bRt.items()}
    if bRt != bL or any(len(sig[T].get(c, ())) != n for c, n in bL.items()):
        return Lenv, Renv, bL, bR, None, None
    # D^H = B''_T B'_T^H per left sector, B'_T = sigma_T^-1 C_T; made exactly unitary by its polar factor
    inv = lambda v: np.where(v > 1e-13 * max(float(np.max(v)), 1e-300), 1.0 / np.maximum(v, 1e-300), 0.0)
    acc = {c: np.zeros((n, n), dtype=np.complex128) for c, n in bL.items()}
    for (l, s_, r), b2 in B2.items():
        c1 = CT.get((l, s_, r))
        if c1 is not None:
            acc[l] += b2 @ (inv(sig[T][l])[:, None] * c1).conj().T
    Ddag = {}
    for c, m in acc.items():                             # (directions of numerically zero weight get an arbitrary completion)
        u, _, vh = np.linalg.svd(m)
        Ddag[c] = u @ vh
    new_carry = {"sigma": sig[T], "Ddag": Ddag}
    if carry is None:
        return Lenv, Renv, bL, bR, None, new_carry
    bonds = [None] * (W + 1)
    bonds[0] = bL
    for k in range(1, T + 1):
        bonds[k] = ob[T + k]
        bonds[T + k] = {sh(c): n for c, n in ob[k].items()}
    if bonds[T] != {sh(c): n for c, n in ob[0].items()} or bonds[W] != bR:
        return (Lenv, Renv, bL, bR, None, new_carry)
    if any(len(sig[0].get(c, ())) != n for c, n in ob[0].items()):
        return (Lenv, Renv, bL, bR, None, new_carry)
    tensors = [None] * W
    tensors[0] = CT
    for k in range(1, T):
        tensors[k] = Bs[T + k]
    for k in range(T):
        blk = {}
        for (l, s_, r), a in A[k].items():
            if l not in sig[k] or r not in sig[k + 1]:
                return (Lenv, Renv, bL, bR, None, new_carry)
            x = (inv(sig[k][l])[:, None] * a) * sig[k + 1][r][None, :]
            if k == 0:
                x = carry["Ddag"][l] @ x
            if k == T - 1:
                x = x @ Ddag[r].conj().T
            blk[(sh(l), s_, sh(r))] = x
        tensors[T + k] = blk
    return Lenv, Renv, bL, bR, (bonds, tensors), new_carry


def _zero_env(bond: dict, levels, side: str, sym=models.SU2U1) -> np.ndarray:
    """environment of an EMPTY block beyond an open end, for a full-width MPO bond: every explicit level is zero
    (the identity level -- 'nothing applied yet' on the left, 'complete' on the right -- is implicit).  Size = sum over
    non-identity levels and connected (ket, bra) pairs of n_bra n_ket; for the one-sector boundary bonds used here:"""
    ident = 0 if side == "L" else len(levels) - 1
    size = 0
    for w, (dN, k) in enumerate(levels):
        if w == ident:
            continue
        for ket, nk in bond.items():
            for bra, nb in bond.items():
                if sym.connects(ket, dN, k, bra):
                    size += nb * nk
    return np.zeros(max(size, 1), dtype=np.complex128)
