"""What moves a finite state (host API, re-exported by api.py): TDVP time steps in real and imaginary time, cooling of a purified
thermal state, local operators applied to a state, Green's functions in time (greens_function, thermal_greens_function) and in
frequency (correction_vector), and the host transforms that turn them into spectral functions.  The sweeps are methods of
engine.DMRG2; this module sets the engine up from the algorithm selector and keeps the books (times, phases, discarded weight).
"""
from __future__ import annotations

import numpy as np

from . import engine as _engine
from . import models
from .observables import _fourier_phases, _other_mpo, density_state, double_occupancy
from .states import (SEED_STEPS, TDVP, TDVP2, CorrectionVector, Environments, FiniteMPS, InfiniteHamiltonian, InfiniteMPS, ThermalMPS,
                     _needs_chain, _no_thermal, _NO_TRUNCATION, _refuse_sharded, _truncation)


# ---- time evolution: TDVP steps of a finite MPS ------------------------------------------------------------------------------
def _tdvp_setup(psi, H, alg):
    if isinstance(psi, InfiniteMPS) or isinstance(H, InfiniteHamiltonian):
        raise NotImplementedError("time evolution of the infinite chain is not available: give a chain length L")
    if not isinstance(alg, (TDVP2, TDVP)):
        raise TypeError("timestep / time_evolve take alg = TDVP2(...)")
    eng = psi.engine
    if not isinstance(alg, TDVP):       # (one-site: the bond tables stay, the truncation settings of the state are not touched)
        eng.chi_full, eng.cutoff = _truncation(alg.trscheme, none=_NO_TRUNCATION)
    eng.krylovdim, eng.lanczos_tol, eng.maxrestart = int(alg.krylovdim), float(alg.tol), int(alg.maxrestart)
    if _other_mpo(eng, H):
        eng.set_mpo(H)          # the quench: another Hamiltonian under the same state
    return eng


def _stepped(eng, step, dts):
    """run step(dt) for every dt on the engine -> the discarded weight of the records those steps added to its stats"""
    k0 = len(eng.stats)
    for dt in dts:
        step(dt)
    return float(sum(s.trunc_weight for s in eng.stats[k0:]))


def _tdvp_step(eng, alg):
    """the sweep of the selector: TDVP2 -> tdvp_sweep (two-site), TDVP -> tdvp1_sweep (one-site, fixed bond tables)"""
    return eng.tdvp1_sweep if isinstance(alg, TDVP) else eng.tdvp_sweep


def timestep(psi: FiniteMPS, H, dt, alg, envs=None):
    """one TDVP step psi <- exp(-i dt H) psi in place (MPSKit.timestep; dt complex, -i beta is imaginary time and the state stays
    normalised): two-site with alg = TDVP2(...), one-site at the current bond tables with alg = TDVP(...).  H other than the
    state's current MPO replaces it first (engine.DMRG2.set_mpo).  -> (psi, envs)"""
    eng = _tdvp_setup(psi, H, alg)
    _tdvp_step(eng, alg)(dt)
    return psi, Environments(eng)


def time_evolve(psi: FiniteMPS, H, times, alg, observe=None):
    """evolve psi through the increasing list `times` (MPSKit.time_evolve; the state is at times[0] on entry), one TDVP step per
    interval (alg = TDVP2(...) or TDVP(...), as for timestep; with TDVP "trunc_weight" is all zeros).  A hybrid run calls this
    twice on one handle: times[:k] with TDVP2(truncdim(D)), then times[k-1:] with TDVP().
    With observe: the list of observe(psi, t) for every t of `times`.  Without: a dict of arrays over the times -- "times", "energy" (<psi|H|psi>), "density_state" and "double_occupancy" ([len(times), L]), "loschmidt" (<psi(t0)|psi(t)>,
    complex) and "trunc_weight" (discarded weight of the step that led to each time, 0 for the first)."""
    eng = _tdvp_setup(psi, H, alg)
    step = _tdvp_step(eng, alg)
    times = [complex(t) if isinstance(t, complex) else float(t) for t in times]
    out = []
    psi0 = None
    if observe is None:
        psi0 = eng.copy()       # the echo needs the initial state: one copy before the first step

    def record(t, tw):
        if observe is not None:
            return observe(psi, t)
        n, d = eng.site_occupations()
        E, _ = eng.bond_energies()
        return {"t": t, "energy": E, "n": n, "d": d, "echo": psi0.overlap(eng), "tw": tw}
    out.append(record(times[0], 0.0))
    for t0, t1 in zip(times[:-1], times[1:]):
        out.append(record(t1, _stepped(eng, step, [t1 - t0])))
    if observe is not None:
        return out
    return {"times": np.array(times), "energy": np.array([r["energy"] for r in out]),
            "density_state": np.array([r["n"] for r in out]), "double_occupancy": np.array([r["d"] for r in out]),
            "loschmidt": np.array([r["echo"] for r in out]), "trunc_weight": np.array([r["tw"] for r in out])}


# ---- finite temperature: a purified thermal state (api.thermal_state) cooled by two-site TDVP in imaginary time ---------------
def cool(psi: ThermalMPS, betas, alg, dbeta: float = 0.05, observe=None):
    """cool a ThermalMPS through the increasing list `betas` (the first not below psi.beta) by two-site TDVP steps in imaginary
    time, alg = TDVP2(trscheme, ...): one tdvp_sweep(-i h / 2) per step of h = min(dbeta, gap to the next requested beta), so
    every requested beta is hit exactly.  psi is advanced in place to betas[-1]; a second call continues from there.
    With observe: the list of observe(psi, beta).  Without: a dict of arrays over the betas -- "betas", "energy" (<H'> of the
    state at beta: one H_eff2 apply on bond 0), "log_z" (n_phys ln 4 + 2 sum of the sweeps' log_norm), "grand_potential"
    (-log_z / beta; nan at beta = 0), "entropy" (beta (E - Omega); log_z at beta = 0), "density" and "double_occupancy"
    ([len(betas), n_phys], one correlator pass each) and "trunc_weight" (discarded weight of the steps that led to each beta).
    The first step from beta = 0 begins with the two sweeps of SEED_STEPS (each at most a quarter of that step), which open the
    bond tables; they count in beta, so the step sizes above hold for their sum with the rest of the first step.
    One-site TDVP() is refused: the bond tables of the beta = 0 state have dimension 1 and one-site steps never grow them."""
    if not isinstance(psi, ThermalMPS):
        raise TypeError("cool takes the ThermalMPS of thermal_state (an InfiniteMPS or a ground state has no temperature to lower)")
    if isinstance(alg, TDVP):
        raise TypeError("cool takes alg = TDVP2(...): the bond tables of the beta = 0 state have dimension 1, and one-site TDVP "
                        "never grows them")
    if not isinstance(alg, TDVP2):
        raise TypeError("cool takes alg = TDVP2(...)")
    _refuse_sharded(psi.engine.ops, "cool")
    betas = [float(b) for b in np.atleast_1d(betas)]
    dbeta = float(dbeta)
    if dbeta <= 0.0:
        raise ValueError("cool: dbeta must be positive")
    if any(b1 <= b0 for b0, b1 in zip(betas[:-1], betas[1:])) or betas[0] < psi.beta:
        raise ValueError(f"cool: betas must increase and start at or above the state's beta = {psi.beta}")
    eng = _tdvp_setup(psi, None, alg)
    out = []

    def step(h):
        tw = _stepped(eng, eng.tdvp_sweep, [-0.5j * h])
        psi.log_z += 2.0 * eng.log_norm
        return tw
    for b in betas:
        tw, seeded = 0.0, 0.0
        if not psi.seeded and b - psi.beta > 1e-12:
            # the beta = 0 tables have dimension 1 between rungs: a term that crosses two such bonds is invisible to every
            # two-site projection there, and the first step would lose it -- an error of first order in dbeta.  Two
            # sweeps of negligible length put the bond directions of H'|I> and H'^2|I> into the tables first; they count as
            # imaginary time, and the first regular step is shorter by their length.  Neither is ever left out: where the first
            # step is itself that short, each takes a quarter of it at the most
            first = min(dbeta, b - psi.beta)
            for eps in SEED_STEPS:
                eps = min(eps, 0.25 * first)
                tw += step(eps)
                seeded += eps
            psi.beta += seeded
            psi.seeded = True
        while b - psi.beta > 1e-12:
            gap = b - psi.beta
            last = gap <= (dbeta - seeded) * (1.0 + 1e-9)   # (the sum of the steps so far carries rounding: the last one closes the gap)
            h = gap if last else dbeta - seeded
            seeded = 0.0
            tw += step(h)
            psi.beta = b if last else psi.beta + h
        psi.beta = b
        if observe is not None:
            out.append(observe(psi, b))
            continue
        E = eng.centre_energy()
        omega = -psi.log_z / b if b > 0.0 else float("nan")
        out.append({"E": E, "lz": psi.log_z, "om": omega, "S": b * (E - omega) if b > 0.0 else psi.log_z,
                    "n": density_state(psi), "d": double_occupancy(psi), "tw": tw})
    if observe is not None:
        return out
    return {"betas": np.array(betas), "energy": np.array([r["E"] for r in out]), "grand_potential": np.array([r["om"] for r in out]),
            "entropy": np.array([r["S"] for r in out]), "log_z": np.array([r["lz"] for r in out]),
            "density": np.array([r["n"] for r in out]), "double_occupancy": np.array([r["d"] for r in out]),
            "trunc_weight": np.array([r["tw"] for r in out])}


# ---- local operators on a finite MPS: G(x, t) and spectral functions ------------------------------------------------
def apply_operator(psi, name, site):
    """a new FiniteMPS holding O_site |psi> for the site operator `name` of the state's symmetry ("c", "c+" = "cdag", "n", "S";
    spinful mode "c_up", "c+_up", ...; or an abi.SiteOp).  psi (centre on site 0, as after a sweep) is copied, the copy's centre
    is carried to `site` without optimisation and the operator applied there on the device (engine.DMRG2.apply_op); psi itself
    is untouched.  The result is not normalised: <O_x psi|O_y psi> = sum over the operator's components of <psi|O+_xq O_yq|psi>,
    so for "c" the overlap matrix of the applied states is correlation_function(psi, "hop").  In the SU(2) modes psi must have
    total spin 0 unless the operator is a scalar."""
    return _applied(psi, name, site)


def _apply_at(eng, op, site, home=None):
    """a new engine holding O_site |eng>: a copy of eng (centre on site 0) with its centre carried to chain site `site`, the
    operator applied there (engine.DMRG2.apply_op), and the centre of the result carried to `home` (None: it stays on `site`)"""
    work = eng.copy()
    work.move_centre(site)
    new = work.apply_op(site, op)
    if home is not None:
        new.move_centre(home)           # (its norm now sits beside normalised tensors: the amplitude, applied by `transition`)
    return new


def _applied(psi, op, site, home=None):
    """apply_operator with its refusals; home as in _apply_at (greens_function and correction_vector want the centre on site 0)"""
    _needs_chain(psi, None, "apply_operator needs", "operators are applied to a finite chain (pass L= / use a FiniteMPS), not to "
                                                    "an InfiniteMPS")
    _no_thermal(psi, "apply_operator")
    if not 0 <= int(site) < psi.L:
        raise ValueError(f"apply_operator: site {site} out of range (the chain has {psi.L} sites)")
    return FiniteMPS(_apply_at(psi.engine, op, int(site), home), psi.L)


def _reference_energy(psi0, H, also=()):
    """E0 = <psi0|H|psi0> on a copy of psi0 (bond_energies moves the centre through the chain: not on the caller's state).  H
    other than the state's MPO is attached to the copy first, and then to the engines of `also`"""
    ref = psi0.engine.copy()
    if _other_mpo(ref, H):
        ref.set_mpo(H)
        for eng in also:
            eng.set_mpo(H)
    return ref.bond_energies()[0]


def greens_function(psi0, H, times, alg, op="c+", site=None):
    """C[t, x] = exp(+i E0 t) <O_x psi0| exp(-i H t) O_site psi0> for all sites x and the increasing list `times` (the first entry
    is the time of the applied state itself, normally 0), E0 = <psi0|H|psi0>, site = L // 2 by default.  One TDVP sweep (alg =
    TDVP2(...), or TDVP(...): one-site at the bond tables of the applied state, trunc_weight all zeros) and one
    `transition` pass per interval.  -> {"times", "C": [len(times), L], "E0", "trunc_weight", "site"}.
    The overlaps carry the sum over the components of the operator's multiplet (apply_operator), e.g. both spins for "c+" in
    the SU(2) modes.  The factor -i, the step function and the combination of the particle part (op = "c+") with the hole part
    (op = "c", evolved with exp(+i H t): conjugate the result) into the retarded function are left to the caller:
    G^R(x, t) = -i theta(t) (C_particle(t, x) + conj(C_hole(t, x))).  The evolved state is renormalised after every truncation
    (TDVP2 of this library), so a truncating trscheme shows up in trunc_weight, not as a loss of norm."""
    _needs_chain(psi0, H, "greens_function needs", "it is measured on a finite chain, not on an InfiniteMPS")
    _no_thermal(psi0, "greens_function")
    L = psi0.L
    site = L // 2 if site is None else int(site)
    times = [float(t) for t in times]
    eng = _tdvp_setup(_applied(psi0, op, site, home=0), H, alg)
    step = _tdvp_step(eng, alg)
    E0 = _reference_energy(psi0, H)
    Cm = np.zeros((len(times), L), dtype=np.complex128)
    tw = np.zeros(len(times))
    Cm[0] = psi0.engine.transition(op, eng)
    for k in range(1, len(times)):
        tw[k] = _stepped(eng, step, [times[k] - times[k - 1]])
        Cm[k] = np.exp(1j * E0 * (times[k] - times[0])) * psi0.engine.transition(op, eng)
    return {"times": np.array(times), "C": Cm, "E0": E0, "trunc_weight": tw, "site": site}


def spectral_function(res, q, omegas, eta):
    """A(q, omega) = -Im G(q, omega) / pi from a greens_function result, on the host: for t >= 0
    G(q, omega) = -i sum_x exp(-i q (x - site)) int dt exp(i omega t) W(t) C[t, x], with the Gaussian window
    W(t) = exp(-(eta t)^2 / 2) (a broadening of width eta in omega) and the trapezoidal rule over res["times"].  q (radians per
    site) and omegas are scalars or arrays -> array [len(q), len(omegas)] (scalars are squeezed out).  omega is measured from
    E0: the particle part (op = "c+") has its weight at omega = E_n(N+1) - E0.  As for momentum_distribution, an open chain has
    no momentum eigenstates: this is the Fourier transform in the distance from `site`, not a momentum-resolved quantity of a
    translation-invariant system, and it is not normalised over a q grid."""
    t = np.asarray(res["times"], dtype=float) - float(res["times"][0])
    Cm = np.asarray(res["C"])
    L = Cm.shape[1]
    ws = np.atleast_1d(np.asarray(omegas, dtype=float))
    Cq = _fourier_phases(q, np.arange(L) - res["site"], -1) @ Cm.T                                                              # [q, t]
    wt = np.zeros_like(t)                                                         # trapezoidal weights
    if len(t) > 1:
        dt = np.diff(t)
        wt[:-1] += 0.5 * dt
        wt[1:] += 0.5 * dt
    kern = np.exp(1j * ws[:, None] * t[None, :]) * (wt * np.exp(-0.5 * (float(eta) * t) ** 2))[None, :]      # [w, t]
    G = -1j * Cq @ kern.T                                                         # [q, w]
    A = -G.imag / np.pi
    if not np.ndim(q):
        A = A[0]
    if not np.ndim(omegas):
        A = A[..., 0]
    return A


def correction_vector(psi0, H, omegas, eta, alg, op="c+", site=None, part="particle"):
    """frequency-space Green's function by correction-vector sweeps:
    G[w, x] = <O_x psi0| (omega + i eta -+ (H - E0))^-1 O_site psi0> for all sites x and every omega of `omegas`, eta > 0 the
    Lorentzian broadening, E0 = <psi0|H|psi0>, site = L // 2 by default.  part = "particle" (sign -, op normally "c+"): the
    solve is (z - H) x = b with z = E0 + omega + i eta; part = "hole" (sign +, op normally "c"): z = E0 - omega - i eta and the
    overall sign flips.  b = O_site psi0 (apply_operator), x an MPS of its own: per omega `cv_sweep`s (engine.DMRG2) until
    |delta <b|x>| <= sweep_tol |<b|x>| or alg.maxsweeps, then G[w] = psi0.engine.transition(op, x) -- the amplitude of x (the
    norm of the solution; the stored tensors stay normalised) is applied inside the library, as for every applied state.  The
    next omega starts from the previous x.  As for greens_function the overlaps carry the sum over the components of the
    operator's multiplet.  Resolution is eta by construction and no time evolution is involved; real z (eta = 0) is not
    guaranteed to converge.  -> {"omegas", "G": [len(omegas), L] complex, "E0", "sweeps" (per omega), "residual" (largest relative
    residual of the last sweep's solves), "trunc_weight" (largest discarded weight of the last sweep), "site", "eta"}"""
    _needs_chain(psi0, H, "correction_vector needs", "it is solved on a finite chain, not on an InfiniteMPS")
    _no_thermal(psi0, "correction_vector")
    if not isinstance(alg, CorrectionVector):
        raise TypeError("correction_vector takes alg = CorrectionVector(...)")
    if part not in ("particle", "hole"):
        raise ValueError("part must be 'particle' or 'hole'")
    L = psi0.L
    site = L // 2 if site is None else int(site)
    omegas = [float(w) for w in np.atleast_1d(omegas)]
    eta = float(eta)
    b = _applied(psi0, op, site, home=0)
    E0 = _reference_energy(psi0, H, also=(b.engine,))
    x = b.engine.copy()                 # start value: b itself, normalised
    x.chi_full, x.cutoff = _truncation(alg.trscheme, none=_NO_TRUNCATION)
    x.krylovdim, x.lanczos_tol, x.maxrestart = int(alg.krylovdim), float(alg.tol), int(alg.maxrestart)
    x.set_orthogonal([b.engine])
    sign = 1.0 if part == "particle" else -1.0
    G = np.zeros((len(omegas), L), dtype=np.complex128)
    sweeps = np.zeros(len(omegas), dtype=int)
    resid, tw = np.zeros(len(omegas)), np.zeros(len(omegas))
    try:
        for k, w in enumerate(omegas):
            z = E0 + sign * (w + 1j * eta)
            last = None
            for it in range(max(int(alg.maxsweeps), 1)):
                k0 = len(x.stats)
                bx, _ = x.cv_sweep(z)
                sweeps[k] = it + 1
                if last is not None and abs(bx - last) <= alg.sweep_tol * abs(bx):
                    break
                last = bx
            resid[k] = max(s.residual for s in x.stats[k0:])
            tw[k] = max(s.trunc_weight for s in x.stats[k0:])
            G[k] = sign * psi0.engine.transition(op, x)
    finally:
        x.set_orthogonal([])
    return {"omegas": np.array(omegas), "G": G, "E0": E0, "sweeps": sweeps, "residual": resid, "trunc_weight": tw, "site": site,
            "eta": eta}


def spectral_function_cv(res, q):
    """A(q, omega) = -Im sum_x exp(-i q (x - site)) G[w, x] / pi from a correction_vector result; q (radians per site) a scalar
    or an array -> array [len(q), len(omegas)] (a scalar q is squeezed out).  As for spectral_function, an open chain has no
    momentum eigenstates: this is the Fourier transform in the distance from `site`."""
    G = np.asarray(res["G"])
    L = G.shape[1]
    A = -(_fourier_phases(q, np.arange(L) - res["site"], -1) @ G.T).imag / np.pi
    return A if np.ndim(q) else A[0]


# ---- finite-temperature dynamics: both states of the purification evolved, or the ket alone under the mirrored generator -----
def _mirror_mpo(psi):
    """the MPO of G = K x 1 - 1 x K~ of a ThermalMPS on its context (models.purified_hamiltonian, ancilla="mirror"), built once"""
    if psi.mirror is None:
        if psi.simul is None:
            raise ValueError("this ThermalMPS does not know its model (it was not made by thermal_state): no mirrored generator")
        psi.mirror = _engine.CMpo(psi.engine.ops, models.purified_hamiltonian(psi.simul, psi.n_phys // psi.simul.bands, "mirror"))
    return psi.mirror


def thermal_greens_function(psi, times, alg, op="c+", site=None, ancilla="idle"):
    """C[t, x] = <psi_beta| exp(+i K t) O+_x exp(-i K t) O_site |psi_beta> = Tr[rho_beta O+_x(t) O_site] of a ThermalMPS at its
    current beta, for all n_phys physical sites x and the increasing list `times` (the first entry is the time of the applied
    state itself, normally 0); site is a physical index, n_phys // 2 by default.  K is the Hamiltonian attached to the state
    (models.purified_hamiltonian): the model including its -mu N, so ensemble and dynamics are grand canonical.  op: any name
    engine.DMRG2.apply_op takes in the state's symmetry ("c+", "c", "n", "S", spinful mode "c+_up", ...); as in greens_function
    the overlaps carry the sum over the components of the operator's multiplet: both spins for "c+" in the SU(2) modes,
    <S_x(t) . S_site> for "S".
    Method: the ancillas stay idle, so psi_beta is no eigenstate of K and the bra is evolved as well -- per interval one
    tdvp_sweep on a copy of psi (the bra) and one on O_site psi (the ket; the operator is applied on chain site 2 site), alg =
    TDVP2(...) for both, then one `transition` pass, of which the physical sublattice is kept.  The bra carries the phase that
    greens_function removes with exp(+i E0 t): there is none here.  One-site TDVP() is refused.  psi itself is not touched.
    -> {"times", "C": [len(times), n_phys] complex, "trunc_weight": [len(times), 2] (discarded weight of the step that led to each
    time, bra and ket), "site", "beta", "op"}; spectral_function takes the result as it is, thermal_spectral_function a particle
    and a hole result.  The factor -i and the step function are left to the caller, as for greens_function.
    ancilla="mirror" (DESIGN 4i): the ancillas are evolved backwards with the mirrored Hamiltonian, the generator is G = K x 1 -
    1 x K~ (models.purified_hamiltonian(..., "mirror")): K~ acts on the ancillas alone, so it commutes with every physical
    operator, and G annihilates psi_beta.  The bra is psi itself, read only and never evolved; per interval one tdvp_sweep of the ket under G and
    one `transition` pass.  No phase is owed: the eigenvalue of psi_beta under G is 0.  That holds as well as `cool` made
    psi_beta (purification_defect measures it).  The result has the same keys, "ancilla" in both schemes; the bra column of
    "trunc_weight" is all zeros.  A state that was never cooled gets the seed sweeps on the ket, under G."""
    _needs_chain(psi, None, "thermal_greens_function needs", "thermal states live on a finite chain, not on an InfiniteMPS")
    if not isinstance(psi, ThermalMPS):
        raise TypeError("thermal_greens_function takes the ThermalMPS of thermal_state / cool; the Green's function of a ground "
                        "state is greens_function")
    if isinstance(alg, TDVP):
        raise TypeError("thermal_greens_function takes alg = TDVP2(...): one-site TDVP never leaves the bond tables of the applied "
                        "state, and those do not hold the dynamics (a projection error that no step size removes)")
    if not isinstance(alg, TDVP2):
        raise TypeError("thermal_greens_function takes alg = TDVP2(...)")
    if ancilla not in ("idle", "mirror"):
        raise ValueError(f"thermal_greens_function: ancilla must be 'idle' or 'mirror', not {ancilla!r}")
    _refuse_sharded(psi.engine.ops, "thermal_greens_function")
    site = psi.n_phys // 2 if site is None else int(site)
    if not 0 <= site < psi.n_phys:
        raise ValueError(f"thermal_greens_function: site {site} out of range (the state has {psi.n_phys} physical sites)")
    times = [float(t) for t in times]
    mirror = ancilla == "mirror"
    bra = psi.engine if mirror else psi.engine.copy()      # (mirror: read only -- `transition` does not modify its bra)
    ket = _apply_at(psi.engine, op, 2 * site, home=0)      # (on the chain site of the physical one; no refusal of thermal states here)
    evolved = (ket,) if mirror else (bra, ket)
    for eng in evolved:
        _tdvp_setup(FiniteMPS(eng, psi.L), None, alg)
    if mirror:
        ket.set_mpo(_mirror_mpo(psi))
    Cm = np.zeros((len(times), psi.n_phys), dtype=np.complex128)
    tw = np.zeros((len(times), 2))
    Cm[0] = bra.transition(op, ket)[::2]
    for k in range(1, len(times)):
        h = times[k] - times[k - 1]
        # a state `cool` has never stepped has the beta = 0 tables, dimension 1 between rungs, and so has the state applied to it:
        # the first interval opens them with the sweeps of SEED_STEPS, as the first step of `cool` does (in real time here, and
        # counted in that interval)
        seeds = [min(eps, 0.25 * h) for eps in SEED_STEPS] if k == 1 and not psi.seeded else []
        for j, eng in enumerate(evolved, start=2 - len(evolved)):
            tw[k, j] = _stepped(eng, eng.tdvp_sweep, seeds + [h - sum(seeds)])
        Cm[k] = bra.transition(op, ket)[::2]
    return {"times": np.array(times), "C": Cm, "trunc_weight": tw, "site": site, "beta": psi.beta, "op": op, "ancilla": ancilla}


def purification_defect(psi):
    """two-site variance of the mirrored generator G = K x 1 - 1 x K~ on a ThermalMPS -> the result type of
    energy_variance: .total, .site [L], .bond [L - 1] over the 2 n_phys chain sites, .energy = <psi|G|psi>.  G annihilates the exact
    psi_beta, so this is 0 for it and measures what truncation and the step error of `cool` left: the quality figure of a cooled
    state for thermal_greens_function(..., ancilla="mirror"), whose bra is taken to be stationary.  On the interleaved chain every
    pair term of G spans at least one site in between (range >= 2), so the figure is a lower bound of <G^2> - <G>^2, as
    energy_variance is for longer-range Hamiltonians.  Measured on a copy with G attached (engine.DMRG2.variance); psi is not
    touched."""
    if not isinstance(psi, ThermalMPS):
        raise TypeError("purification_defect takes the ThermalMPS of thermal_state / cool")
    _refuse_sharded(psi.engine.ops, "purification_defect")
    work = psi.engine.copy()
    work.set_mpo(_mirror_mpo(psi))
    return work.variance()


def _adjoint_pair(part_op, hole_op):
    """True if the two operator names are a creator and the annihilator of the same orbital ("c+" / "c", "c+_up" / "c_up", ...)"""
    alias = _engine.DMRG2.OP_ALIASES
    p, h = alias.get(part_op, part_op), alias.get(hole_op, hole_op)
    return p.startswith("cdag") and h == "c" + p[len("cdag"):]


def thermal_spectral_function(part, hole, q, omegas, eta):
    """A(q, omega) = -Im G^R(q, omega) / pi at finite temperature from two thermal_greens_function results of the same state, times
    and site: `part` for a creator (op = "c+") and `hole` for its annihilator (op = "c"), combined into the retarded function
    G^R(x, t) = -i theta(t) (C_part(t, x) + conj(C_hole(t, x))) = -i theta(t) Tr[rho_beta {c_x(t), c+_site}] and transformed by
    spectral_function: its Gaussian window of width eta, its trapezoidal rule over the times, its Fourier transform in x - site;
    q and omegas scalars or arrays -> [len(q), len(omegas)].  Host only.  Conventions: the anticommutator sums over the components
    of the operator's multiplet, so in the SU(2) modes A is the sum of both spins and integrates to 2 over omega at q = 0 (to 1 for
    "c+_up" / "c_up" in the spinful mode); omega is measured from the chemical potential, since K = H - mu N drives the dynamics;
    as for spectral_function, an open chain has no momentum eigenstates and q is the variable conjugate to the distance from
    `site`.  Results that do not belong together raise ValueError."""
    for key in ("site", "beta", "times", "C", "op"):
        if key not in part or key not in hole:
            raise ValueError(f"thermal_spectral_function takes two thermal_greens_function results ('{key}' is missing)")
    tp, th = np.asarray(part["times"], dtype=float), np.asarray(hole["times"], dtype=float)
    if part["site"] != hole["site"] or part["beta"] != hole["beta"]:
        raise ValueError("thermal_spectral_function: the particle and the hole part differ in site or beta")
    if tp.shape != th.shape or not np.array_equal(tp, th) or np.shape(part["C"]) != np.shape(hole["C"]):
        raise ValueError("thermal_spectral_function: the particle and the hole part differ in their times or their sites")
    if isinstance(part["op"], str) and isinstance(hole["op"], str) and not _adjoint_pair(part["op"], hole["op"]):
        raise ValueError(f"thermal_spectral_function: op '{part['op']}' (particle) and '{hole['op']}' (hole) are not a creator and "
                         "its annihilator")
    both = dict(part, C=np.asarray(part["C"]) + np.conj(np.asarray(hole["C"])))
    return spectral_function(both, q, omegas, eta)


