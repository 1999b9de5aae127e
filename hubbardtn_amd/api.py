"""Host API mirroring the reference's call sequence on the hot path:

    model = OB_Sim(t, u, mu, P, Q, svalue, bond_dim; spin=false)         src/HubbardFunctions.jl:76-93
    dictionary = produce_groundstate(model)                              src:1145-1166
    psi, H = dictionary["groundstate"], dictionary["ham"]
    E = sum(real(expectation_value(psi, H))) / length(H)                 examples/One_band.jl:42-43
    dim_state(psi)                                                       src:1399-1405

and the plugin boundary MPSKit exposes to it,

    find_groundstate(psi0, H, alg) -> (psi, envs, delta)                 src:1010

with `alg = DMRG2(trscheme=truncdim(D) | truncbelow(eta), tol, maxiter, verbosity)`.

Two drivers share the hot path: with a chain length (`L=` keyword / `simul.kwargs["L"]`) the
finite two-site sweep DMRG2 that BASELINE.json's L=... configs name; without one the infinite-chain IDMRG2 the
reference itself calls (src:1010), here in McCulloch's growing-window form (hubbardtn_amd/idmrg.py) with the
reference's truncation default truncbelow(10^-svalue).  All compute goes through the HIP library; there is no CPU
path.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import engine as _engine
from . import idmrg as _idmrg
from . import models, mps
from .models import MB_Sim, MBC_Sim, OB_Sim, OBC_Sim, OBC_Sim2, Simulation


# ---- truncation schemes (TensorKit names; App. A.6) --------------------------------------------
@dataclass
class truncdim:
    """keep at most D in TensorKit `dim` units (sum (2S+1) n); used at src:1363-1365"""
    D: int


@dataclass
class truncbelow:
    """keep Schmidt values > eta; used at src:1010 with eta = 10^-svalue"""
    eta: float


@dataclass
class DMRG2:
    """two-site DMRG algorithm selector (MPSKit.DMRG2 / IDMRG2 keyword names)"""
    trscheme: object = None
    tol: float = 1e-6              # src:993 default of compute_groundstate
    maxiter: int = 100
    verbosity: int = 0
    krylovdim: int = 30            # KrylovKit / MPSKit defaults (App. A.4)
    eigsolve_tol: float = 1e-10


@dataclass
class DMRG:
    """one-site DMRG at the state's current bond tables (MPSKit.DMRG keyword names): converge or polish a state whose
    bonds two-site sweeps have grown.  tol: on the energy change per site between two sweeps."""
    tol: float = 1e-6
    maxiter: int = 100
    krylovdim: int = 30
    verbosity: int = 0
    eigsolve_tol: float = 1e-10


@dataclass
class IDMRG2:
    """infinite two-site DMRG selector (MPSKit.IDMRG2 keyword names; the call at src:1010)"""
    trscheme: object = None
    tol: float = 1e-6              # on the change of the centre Schmidt spectrum (MPSKit: ||C_old - C_new||)
    maxiter: int = 100
    verbosity: int = 0
    krylovdim: int = 30
    eigsolve_tol: float = 1e-10
    sweeps_per_step: int = 6       # at most this many finite sweeps of the 2-cell window per growth step
    driver: str = "python"         # growth loop: "python" (idmrg.idmrg2's loop) or "native" (htn_idmrg_* inside the library)


@dataclass
class TDVP2:
    """two-site TDVP selector (MPSKit.TDVP2 keyword names): trscheme truncates every bond step, tol is the tolerance of the
    Krylov exponential, maxrestart the number of sub-steps a solve may take when krylovdim vectors do not reach it"""
    trscheme: object = None
    krylovdim: int = 30
    tol: float = 1e-10
    maxrestart: int = 8


@dataclass
class TDVP:
    """one-site TDVP selector (MPSKit.TDVP keyword names): time evolution at the state's current bond tables, nothing is
    truncated (hence no trscheme).  Grow the bonds first -- two-site DMRG sweeps, or TDVP2 steps until the cap is reached -- then
    switch to this on the same handle.  tol is the tolerance of the Krylov exponential, maxrestart the number of sub-steps a
    solve may take when krylovdim vectors do not reach it."""
    krylovdim: int = 30
    tol: float = 1e-10
    maxrestart: int = 8


@dataclass
class CorrectionVector:
    """correction-vector (DDMRG) selector: trscheme truncates every bond step, tol is the relative residual of the local solves
    (krylovdim vectors per cycle, at most maxrestart restarts), sweeps per frequency run until <b|x> changes by less than
    sweep_tol relative, at most maxsweeps"""
    trscheme: object = None
    krylovdim: int = 30
    tol: float = 1e-8
    maxrestart: int = 50
    sweep_tol: float = 1e-6
    maxsweeps: int = 10


@dataclass
class InfiniteHamiltonian:
    """the model of a translation-invariant chain; len() = sites per unit cell (length(H) in the reference)"""
    simul: Simulation

    def __len__(self):
        return _idmrg.cell_sites(self.simul)


@dataclass
class InfiniteMPS:
    """handle of an infinite MPS: before optimisation only the start parameters, afterwards the IDMRGResult"""
    max_dimension: int
    seed: int = 1234
    ops: object = None
    result: object = None

    def bond_dimensions(self):
        if self.result is None:
            raise RuntimeError("run find_groundstate first")
        T = self.result.unit_cell
        return list(self.result.bond_dims[T // 2 + 1:T // 2 + 1 + T])     # the central unit cell of the last window


@dataclass
class FiniteMPS:
    """device-resident finite MPS handle (wraps the sweep engine's state)"""
    engine: object
    L: int

    def bond_dimensions(self):
        return self.engine.bond_dims()


@dataclass
class ThermalMPS(FiniteMPS):
    """purified thermal state of n_phys physical sites on a chain of L = 2 n_phys sites (physical site i at 2 i, its ancilla at
    2 i + 1; `thermal_state`, `cool`): |psi_beta> ~ exp(-beta H' / 2)|I>, normalised; log_z = ln Z(beta) of the grand-canonical
    ensemble H - mu N the model defines.  The observables of this module report its physical sites only."""
    n_phys: int = 0
    beta: float = 0.0
    log_z: float = 0.0
    seeded: bool = False        # cool() has put the first bond directions into the beta = 0 tables (SEED_STEPS)
    simul: object = None        # the model: the mirror scheme builds its generator from it
    mirror: object = None       # engine.CMpo of models.purified_hamiltonian(simul, n_phys, "mirror"), built on first use


SEED_STEPS = (1e-10, 1e-5)      # imaginary-time lengths of the two sweeps that open the bond tables of the beta = 0 state


def _phys(psi, x):
    """the physical sublattice of a per-site vector or a site x site matrix of a ThermalMPS; anything else unchanged"""
    if not isinstance(psi, ThermalMPS):
        return x
    if isinstance(x, tuple):
        return tuple(_phys(psi, v) for v in x)
    return x[::2] if np.ndim(x) == 1 else x[::2, ::2]


def _no_thermal(psi, what):
    if isinstance(psi, ThermalMPS):
        raise NotImplementedError(f"{what} of a ThermalMPS is not available: dynamics at finite temperature needs the bra of the "
                                  "purification evolved as well (thermal_greens_function evolves both)")


@dataclass
class Environments:
    engine: object


_OPS = None


def _ops(device=0):
    global _OPS
    if _OPS is None:
        from .device import HipOps        # raises if libhubbardtn_hip.so or the GPU is missing
        _OPS = HipOps(device)
    return _OPS


def hamiltonian(simul: Simulation, L: int | None = None):
    """finite open chain of L unit cells -> list of MPO sites; no L -> the infinite chain (src:386-472, 811-910)"""
    L = L or simul.kwargs.get("L")
    if L is None:
        return InfiniteHamiltonian(simul)
    return models.hamiltonian(simul, int(L))


def target_sector(sym, nsites: int, P: int = 1, Q: int = 1, charges=None):
    """total sector (N, j) of a finite chain for the reference's `charges = [parity, spin, dN]` (src:1174, 1185), relative to
    the filling P/Q: (N0 + dN, 2 spin) in the SU(2) x U(1) mode, (N0 + dN, 2 Sz) with spin=true, (parity, 2 spin) without
    U(1).  None = the ground-state sector (N0, 0)."""
    if sym.kind == 2:
        if charges is None:
            return (0, 0)
        parity, j2 = int(charges[0]), 2.0 * float(charges[1])
        if parity not in (0, 1) or j2 != int(j2) or j2 < 0:
            raise ValueError("charges = [parity, spin]: parity is 0 or 1 and spin a non-negative multiple of 1/2")
        if (parity + int(j2)) % 2:
            raise ValueError("charges: fermion parity and spin do not match (a half-integer spin needs odd parity)")
        if int(j2) > nsites:
            raise ValueError(f"charges: a chain of {nsites} sites cannot hold spin {charges[1]}")
        return (parity, int(j2))
    if (nsites * P) % Q:
        raise ValueError("filling P/Q incompatible with the chain length")
    N0 = nsites * P // Q
    if charges is None:
        return (N0, 0)
    if len(charges) != 3:
        raise ValueError("charges = [parity, spin, dN]")
    parity, j2, dN = int(charges[0]), 2.0 * float(charges[1]), int(charges[2])
    if parity not in (0, 1) or parity != dN % 2:
        raise ValueError(f"charges: fermion parity {charges[0]} contradicts dN = {dN} (parity = dN mod 2)")
    if j2 != int(j2) or (sym.su2 and j2 < 0):
        raise ValueError("charges: spin must be a multiple of 1/2" + (" and non-negative" if sym.su2 else ""))
    N, j2 = N0 + dN, int(j2)
    if (N + j2) % 2:
        raise ValueError(f"charges: spin {charges[1]} with N = {N} electrons (half-integer spin needs odd N, integer spin even N)")
    if not 0 <= N <= 2 * nsites or abs(j2) > min(N, 2 * nsites - N):
        raise ValueError(f"charges: a chain of {nsites} sites cannot hold the sector N = {N}, 2S = {j2}")
    return (N, j2)


def initialize_mps(H, P: int, max_dimension: int | None = None, spin: bool = False, Q: int = 1, seed: int = 1234, ops=None,
                   charges=None):
    """random right-canonical start with per-sector cap `max_dimension` (src:917-959); the symmetry mode (SU(2) x U(1),
    or U(1) x U(1) for `spin=true`) is the Hamiltonian's.  The chemical-potential models use the reference's two-argument
    form `initialize_mps(operator, max_dimension)` (src:961-991).  charges = [parity, spin, dN] (finite chains): the total
    sector of the state, see target_sector; None = the ground-state sector."""
    if charges is not None and isinstance(H, InfiniteHamiltonian):
        raise NotImplementedError("initialize_mps: charges need a finite chain")
    if charges is not None and getattr(H, "sym", None) is models.SU2P:
        max_dimension = P if max_dimension is None else max_dimension
        bonds, tensors = mps.random_mps(len(H), target_sector(models.SU2P, len(H), charges=charges), int(max_dimension), seed=seed,
                                        sym=models.SU2P)
        return FiniteMPS(_engine.DMRG2(ops or _ops(), H, bonds, tensors), len(H))
    if isinstance(H, InfiniteHamiltonian) and models.symmetry_of(H.simul).kind == 2 or getattr(H, "sym", None) is models.SU2P:
        # (parity 0, S = 0) total sector on a finite chain: an even number of electrons in a singlet
        max_dimension = P if max_dimension is None else max_dimension
        if isinstance(H, InfiniteHamiltonian):
            return InfiniteMPS(int(max_dimension), seed, ops)
        bonds, tensors = mps.random_mps(len(H), (0, 0), int(max_dimension), seed=seed, sym=models.SU2P)
        return FiniteMPS(_engine.DMRG2(ops or _ops(), H, bonds, tensors), len(H))
    if isinstance(H, InfiniteHamiltonian):
        if bool(spin) != (not models.symmetry_of(H.simul).su2):
            raise ValueError("initialize_mps: `spin` does not match the Hamiltonian's symmetry mode")
        return InfiniteMPS(int(max_dimension), seed, ops)
    if max_dimension is None:
        raise TypeError("initialize_mps(H, P, max_dimension, spin, Q): max_dimension is required for the fixed-filling models")
    nsites = len(H)
    sym = getattr(H, "sym", models.SU2U1)
    if bool(spin) != (not sym.su2):
        raise ValueError("initialize_mps: `spin` does not match the Hamiltonian's symmetry mode")
    target = target_sector(sym, nsites, P, Q, charges)  # charges None: total spin 0 / total Sz 0 at filling P/Q
    bonds, tensors = mps.random_mps(nsites, target, max_dimension, seed=seed, sym=sym)
    eng = _engine.DMRG2(ops or _ops(), H, bonds, tensors)
    return FiniteMPS(eng, nsites)


def find_groundstate(psi: FiniteMPS, H, alg: DMRG2, envs=None):
    """-> (psi, envs, delta); delta = |E_sweep - E_previous sweep| / L at exit (MPSKit returns the
    last convergence error).  Sweeps until delta < alg.tol or maxiter.  With an InfiniteMPS / IDMRG2: growth steps
    until the centre Schmidt spectrum changes by less than alg.tol.  With alg = DMRG(...) on a FiniteMPS: one-site sweeps at
    the state's current bond tables (engine.DMRG2.sweep1), same return values."""
    if isinstance(psi, InfiniteMPS):
        if not isinstance(alg, IDMRG2) or not isinstance(H, InfiniteHamiltonian):
            raise TypeError("an InfiniteMPS is optimised with IDMRG2 on hamiltonian(simul) without a chain length")
        chi, cut = None, 0.0
        if isinstance(alg.trscheme, truncdim):
            chi = int(alg.trscheme.D)
        elif isinstance(alg.trscheme, truncbelow):
            cut = float(alg.trscheme.eta)
        elif alg.trscheme is not None:
            raise TypeError("trscheme must be truncdim(D) or truncbelow(eta)")
        psi.result = _idmrg.idmrg2(psi.ops or _ops(), H.simul, chi_full=chi, cutoff=cut, tol=alg.tol,
                                   maxiter=alg.maxiter, sweeps_per_step=alg.sweeps_per_step,
                                   init_dimension=psi.max_dimension, krylovdim=alg.krylovdim,
                                   lanczos_tol=alg.eigsolve_tol, seed=psi.seed, verbosity=alg.verbosity,
                                   driver=alg.driver)
        return psi, Environments(psi.result.engine), psi.result.delta
    eng = psi.engine
    if isinstance(alg, DMRG):
        # one-site sweeps: the bond tables stay as they are, nothing is truncated
        eng.krylovdim, eng.lanczos_tol = alg.krylovdim, alg.eigsolve_tol
        E_prev, delta = None, float("inf")
        for it in range(alg.maxiter):
            E = eng.sweep1()
            if E_prev is not None:
                delta = abs(E - E_prev) / psi.L
            if alg.verbosity:
                print(f"DMRG sweep {it + 1}: E/L = {E / psi.L:.12f}  delta = {delta:.3e}  chi = {max(eng.bond_dims())}")
            E_prev = E
            if delta < alg.tol:
                break
        return psi, Environments(eng), delta
    if isinstance(alg.trscheme, truncdim):
        eng.chi_full, eng.cutoff = int(alg.trscheme.D), 0.0
    elif isinstance(alg.trscheme, truncbelow):
        eng.chi_full, eng.cutoff = None, float(alg.trscheme.eta)
    elif alg.trscheme is not None:
        raise TypeError("trscheme must be truncdim(D) or truncbelow(eta)")
    eng.krylovdim, eng.lanczos_tol = alg.krylovdim, alg.eigsolve_tol
    E_prev, delta = None, float("inf")
    for it in range(alg.maxiter):
        E = eng.sweep()
        if E_prev is not None:
            delta = abs(E - E_prev) / psi.L
        if alg.verbosity:
            print(f"DMRG2 sweep {it + 1}: E/L = {E / psi.L:.12f}  delta = {delta:.3e}  chi = {max(eng.bond_dims())}")
        E_prev = E
        if delta < alg.tol:
            break
    return psi, Environments(eng), delta


def _tdvp_setup(psi, H, alg):
    if isinstance(psi, InfiniteMPS) or isinstance(H, InfiniteHamiltonian):
        raise NotImplementedError("time evolution of the infinite chain is not available: give a chain length L")
    if not isinstance(alg, (TDVP2, TDVP)):
        raise TypeError("timestep / time_evolve take alg = TDVP2(...)")
    eng = psi.engine
    if isinstance(alg, TDVP):           # one-site: the bond tables stay, the truncation settings of the state are not touched
        pass
    elif isinstance(alg.trscheme, truncdim):
        eng.chi_full, eng.cutoff = int(alg.trscheme.D), 0.0
    elif isinstance(alg.trscheme, truncbelow):
        eng.chi_full, eng.cutoff = None, float(alg.trscheme.eta)
    elif alg.trscheme is None:
        eng.chi_full, eng.cutoff = None, 0.0
    else:
        raise TypeError("trscheme must be truncdim(D) or truncbelow(eta)")
    eng.krylovdim, eng.lanczos_tol, eng.maxrestart = int(alg.krylovdim), float(alg.tol), int(alg.maxrestart)
    if H is not None and H is not eng.mpo and H is not eng.cmpo:
        eng.set_mpo(H)          # the quench: another Hamiltonian under the same state
    return eng


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
        k0 = len(eng.stats)
        step(t1 - t0)
        out.append(record(t1, float(sum(s.trunc_weight for s in eng.stats[k0:]))))
    if observe is not None:
        return out
    return {"times": np.array(times), "energy": np.array([r["energy"] for r in out]),
            "density_state": np.array([r["n"] for r in out]), "double_occupancy": np.array([r["d"] for r in out]),
            "loschmidt": np.array([r["echo"] for r in out]), "trunc_weight": np.array([r["tw"] for r in out])}


# ---- finite temperature: purified thermal states cooled by two-site TDVP -----------------------------------------------
def _refuse_sharded(ops, what):
    if bool(getattr(ops, "_cb", None)) or int(getattr(ops, "comm_world", 1)) > 1:
        raise NotImplementedError(f"{what}: thermal states are not available in a context with a communicator or an exchange "
                                  "hook")


def thermal_state(simul: Simulation, L: int | None = None, ops=None):
    """the infinite-temperature state of `simul` on L unit cells as a ThermalMPS at beta = 0: the purified chain of
    mps.infinite_temperature_mps with models.purified_hamiltonian attached.  The ancillas carry the complementary
    charge, so the physical particle number fluctuates at fixed chain charge: the ensemble is grand canonical and `mu` of the
    model (the diagonal of t for MB_Sim) sets the filling; P / Q are not used."""
    L = L or simul.kwargs.get("L")
    if L is None:
        raise NotImplementedError("thermal_state needs a chain length: thermal states live on a finite chain (pass L=)")
    ops = ops or _ops()
    _refuse_sharded(ops, "thermal_state")
    H = models.purified_hamiltonian(simul, int(L))
    n_phys = len(H) // 2
    bonds, tensors = mps.infinite_temperature_mps(n_phys, H.sym)
    eng = _engine.DMRG2(ops, H, bonds, tensors)
    return ThermalMPS(eng, len(H), n_phys, 0.0, n_phys * float(np.log(4.0)), simul=simul)


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
        k0 = len(eng.stats)
        eng.tdvp_sweep(-0.5j * h)
        psi.log_z += 2.0 * eng.log_norm
        return float(sum(s.trunc_weight for s in eng.stats[k0:]))
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


def compute_groundstate(simul: Simulation, L: int | None = None, tol: float = 1e-6, verbosity: int = 0,
                        maxiter: int = 100, init_state=None, chi: int | None = None, driver: str = "python"):
    """src:993-1030 restated for the finite chain: H = hamiltonian(simul); psi0 = initialize_mps(...);
    find_groundstate(psi0, H, DMRG2(trscheme = truncbelow(10^-svalue))) -- or truncdim(chi) when a
    fixed bond dimension is requested (the configs of BASELINE.json).  driver: growth loop of the infinite chain
    (IDMRG2.driver)."""
    H = hamiltonian(simul, L)
    spin = bool(simul.kwargs.get("spin", False))
    psi0 = init_state if init_state is not None else initialize_mps(H, simul.P, simul.bond_dim, spin, simul.Q)
    scheme = truncdim(chi) if chi is not None else truncbelow(10.0 ** (-simul.svalue))
    if isinstance(H, InfiniteHamiltonian):       # src:1010; the VUMPS / GradientGrassmann polish (src:1025-1027) is out of scope
        if chi is None and _idmrg.reference_cell_sites(simul) == 1:
            # the reference's branch for length(H) == 1 (src:1012-1022): VUMPS at fixed space, the space grown by VUMPSSvdCut and
            # cut by SvdCut(truncbelow(10^-svalue)) until it stops changing.  VUMPS-free route: the same self-consistent space is
            # the fixed point of two-site updates with that Schmidt cut -- IDMRG2 -- once the cut is expressed for the doubled cell
            # this library uses (idmrg.schmidt_cut_scale: one sector family per bond instead of both at half weight)
            scheme = truncbelow(_idmrg.schmidt_cut_scale(simul) * 10.0 ** (-simul.svalue))
        alg = IDMRG2(trscheme=scheme, tol=tol, verbosity=verbosity, maxiter=maxiter, driver=driver)
    else:
        alg = DMRG2(trscheme=scheme, tol=tol, verbosity=verbosity, maxiter=maxiter)
    psi, envs, delta = find_groundstate(psi0, H, alg)
    return {"groundstate": psi, "environments": envs, "ham": H, "delta": delta, "config": simul}


def produce_groundstate(simul: Simulation, force: bool = False, **kw):
    """src:1145-1166: computes, or loads the result saved under the reference's cache name (storage.produce_or_load)"""
    from . import storage
    return storage.produce_or_load(compute_groundstate, simul, force=force, **kw)


def _exc_setup(simul, momenta, nums, charges, L):
    L = L or simul.kwargs.get("L")
    if L is None:
        raise NotImplementedError("excitations of the infinite chain need the quasiparticle ansatz on a uniform MPS "
                                  "(src:1173-1209), which this library does not have: give a chain length L")
    if momenta is not None:
        raise ValueError("an open finite chain has no momentum: momenta must be None")
    charges = [0, 0.0, 0] if charges is None else list(charges)
    trivial = not any(float(c) for c in charges)
    if nums < 1 or nums - (0 if trivial else 1) > 8:
        raise ValueError("nums: at least 1, and at most 8 states can be attached to a sweep (8 excited states of the ground-state "
                         "sector, 9 states of any other)")
    return int(L), charges, trivial


def compute_excitations(simul: Simulation, momenta, nums: int, charges=None, L: int | None = None, tol: float = 1e-10,
                        maxiter: int = 40, chi: int | None = None, seed: int = 4321, verbosity: int = 0, **kw):
    """finite-chain counterpart of src:1173-1209: the lowest `nums` states of the sector `charges = [parity, spin, dN]` by
    two-site DMRG in the orthogonal complement of the states found before (engine.DMRG2.set_orthogonal).  -> {"Es", "states",
    "E0", "charges"}: Es[k] = energy of the k-th state minus the ground-state energy E0 of the sector [0, 0, 0] (the
    reference measures its Es from its ground state, too); for charges [0, 0, 0] the ground state is the first attached state
    and Es are the excited states above it.  momenta must be None (no momentum on an open chain)."""
    L, charges, trivial = _exc_setup(simul, momenta, nums, charges, L)
    d = produce_groundstate(simul, L=L, chi=chi, tol=min(tol, 1e-6), maxiter=maxiter, **kw)
    g = d["groundstate"].engine
    H = d["ham"]
    E0 = float(g.energy)
    spin = bool(simul.kwargs.get("spin", False))
    found, states, Es = ([g] if trivial else []), [], []
    for k in range(nums):
        psi = initialize_mps(H, getattr(simul, "P", 1), simul.bond_dim, spin, getattr(simul, "Q", 1), seed=seed + k, ops=g.ops,
                             charges=charges)
        eng = psi.engine
        eng.chi_full, eng.cutoff = g.chi_full, g.cutoff
        eng.krylovdim = min(g.krylovdim, 31 - len(found))          # row limit of the projected Lanczos step
        eng.set_orthogonal(found)
        E_prev = None
        for it in range(maxiter):
            E = eng.sweep()
            if verbosity:
                print(f"state {k} sweep {it + 1}: E = {E:.12f}")
            if E_prev is not None and abs(E - E_prev) / L < tol:
                break
            E_prev = E
        found.append(eng)
        states.append(psi)
        Es.append(E - E0)
    return {"Es": np.array(Es), "states": states, "E0": E0, "charges": charges}


def produce_excitations(simul: Simulation, momenta, nums: int, force: bool = False, charges=None, L: int | None = None, **kw):
    """src:1211-1265: compute_excitations, or the entry saved under the reference's prefix rule (storage.excitations_name):
    the energies as JSON, the states in storage.save_state format"""
    import json
    import os
    from . import storage
    L, charges, _ = _exc_setup(simul, momenta, nums, charges, L)
    simul.kwargs.setdefault("L", L)
    sub, stem = storage.excitations_name(simul, nums, charges)
    if kw.get("chi"):
        stem += f"_chi={int(kw['chi'])}"
    directory = storage.datadir("sims", sub)
    entry = os.path.join(directory, stem)
    if os.path.isdir(entry) and not force:
        meta = json.load(open(os.path.join(entry, "excitations.json")))
        H = hamiltonian(simul, L)
        states = []
        for k in range(nums):
            bonds, sites = storage.load_state(os.path.join(entry, f"state_{k}"))
            eng = _engine.DMRG2(_ops(), H, bonds, [s["blocks"] for s in sites], chi_full=meta["chi_full"], cutoff=meta["cutoff"])
            eng.energy = meta["E0"] + meta["Es"][k]
            states.append(FiniteMPS(eng, L))
        return {"Es": np.array(meta["Es"]), "states": states, "E0": meta["E0"], "charges": meta["charges"]}
    res = compute_excitations(simul, None, nums, charges=charges, L=L, **kw)
    try:
        os.makedirs(directory, exist_ok=True)
        if os.path.isdir(entry):
            import shutil
            shutil.rmtree(entry)
        os.makedirs(entry)
        for k, psi in enumerate(res["states"]):
            storage.save_state(psi, entry, f"state_{k}")
        e0 = res["states"][0].engine
        with open(os.path.join(entry, "excitations.json"), "w") as f:
            json.dump({"Es": [float(x) for x in res["Es"]], "E0": res["E0"], "charges": [float(c) for c in res["charges"]],
                       "chi_full": e0.chi_full, "cutoff": e0.cutoff}, f)
    except OSError:
        pass
    return res


def produce_bandgap(simul: Simulation, L: int | None = None, force: bool = False, **kw):
    """src:1267-1299 on an open chain: the charge gap E0(N+1, 1/2) + E0(N-1, 1/2) - 2 E0(N, 0) as Es_hole[0] + Es_elec[0]
    with charges [1, 1/2, -1] and [1, 1/2, +1] (src:1284-1285)"""
    if bool(simul.kwargs.get("spin", False)):
        raise NotImplementedError("Band gap for spin systems not implemented.")
    hole = produce_excitations(simul, None, 1, force=force, charges=[1, 0.5, -1], L=L, **kw)
    elec = produce_excitations(simul, None, 1, force=force, charges=[1, 0.5, 1], L=L, **kw)
    return float(hole["Es"][0] + elec["Es"][0])


def spin_gap(simul: Simulation, L: int | None = None, force: bool = False, **kw):
    """E0(N, S = 1) - E0(N, 0): the lowest state of charges [0, 1, 0] above the ground state"""
    return float(produce_excitations(simul, None, 1, force=force, charges=[0, 1.0, 0], L=L, **kw)["Es"][0])


def expectation_value(psi: FiniteMPS, H):
    """<psi|H|psi> per site as a vector whose sum / length(H) is the energy per site (examples/One_band.jl:42-43 take
    sum(real(E0)) / length(H); test/OB.jl:28-29).  Finite chain: a genuine expectation value of the state AS STORED
    (after truncation), evaluated by a non-optimising pass through the library; entry i = energy of the terms ending on
    site i (engine.DMRG2.site_energies).  Infinite chain: the energy density of the converged window, the same for
    every site of the unit cell: differences of <psi_n|H_n|psi_n> of successive (truncated) window states."""
    if isinstance(psi, InfiniteMPS):
        if psi.result is None:
            raise RuntimeError("run find_groundstate first")
        return np.full(len(H), psi.result.energy_per_site)
    if psi.engine.energy is None:
        raise RuntimeError("run find_groundstate first")
    return psi.engine.site_energies()


def _save_result(res, entry):
    """cache entry of produce_groundstate: the site tensors (storage.save_state format) + what re-creates the handle"""
    import json
    import os
    from . import storage
    psi = res["groundstate"]
    storage.save_state(psi, os.path.dirname(entry), os.path.basename(entry))
    meta = {"delta": float(res["delta"])}
    if isinstance(psi, InfiniteMPS):
        r = psi.result
        meta.update(kind="infinite", energy_per_site=r.energy_per_site, iterations=r.iterations, unit_cell=r.unit_cell,
                    history=[list(h) for h in r.history], max_dimension=psi.max_dimension, seed=psi.seed,
                    spectrum=[[N, j, [float(x) for x in v]] for (N, j), v in sorted(r.spectrum.items())],
                    bL=[[N, j, n] for (N, j), n in sorted(r.boundary["bL"].items())],
                    bR=[[N, j, n] for (N, j), n in sorted(r.boundary["bR"].items())],
                    chi_full=r.engine.chi_full, cutoff=r.engine.cutoff)
        np.save(os.path.join(entry, "left_env.npy"), r.boundary["Lenv"])
        np.save(os.path.join(entry, "right_env.npy"), r.boundary["Renv"])
    else:
        eng = psi.engine
        meta.update(kind="finite", L=psi.L, energy=eng.energy, chi_full=eng.chi_full, cutoff=eng.cutoff)
    with open(os.path.join(entry, "result.json"), "w") as f:
        json.dump(meta, f)


def _load_result(simul, entry, L=None, ops=None, **kw):
    """the result dictionary of compute_groundstate re-created from a cache entry: the state is uploaded, nothing is
    recomputed"""
    import json
    import os
    from . import storage
    meta = json.load(open(os.path.join(entry, "result.json")))
    bonds, sites = storage.load_state(entry)
    tensors = [s["blocks"] for s in sites]
    H = hamiltonian(simul, L)
    ops = ops or _ops()
    if meta["kind"] == "infinite":
        T = meta["unit_cell"]
        big = models.hamiltonian(simul, 8 * max(meta["unit_cell"] // simul.bands, 1))
        window = [big[3 * T + i] for i in range(2 * T)]
        eng = _engine.DMRG2(ops, window, bonds, tensors, chi_full=meta["chi_full"], cutoff=meta["cutoff"],
                            left_env=np.load(os.path.join(entry, "left_env.npy")),
                            right_env=np.load(os.path.join(entry, "right_env.npy")))
        spec = {(N, j): np.asarray(v) for N, j, v in meta["spectrum"]}
        res = _idmrg.IDMRGResult(energy_per_site=meta["energy_per_site"], delta=meta["delta"], iterations=meta["iterations"],
                                 unit_cell=T, bond_dims=eng.bond_dims(), spectrum=spec,
                                 history=[tuple(h) for h in meta["history"]], engine=eng,
                                 boundary={"bL": {(N, j): n for N, j, n in meta["bL"]}, "bR": {(N, j): n for N, j, n in meta["bR"]},
                                           "Lenv": np.load(os.path.join(entry, "left_env.npy")),
                                           "Renv": np.load(os.path.join(entry, "right_env.npy"))})
        psi = InfiniteMPS(meta["max_dimension"], meta["seed"], ops, res)
        return {"groundstate": psi, "environments": Environments(eng), "ham": H, "delta": meta["delta"], "config": simul}
    eng = _engine.DMRG2(ops, H, bonds, tensors, chi_full=meta["chi_full"], cutoff=meta["cutoff"])
    eng.energy = meta["energy"]
    psi = FiniteMPS(eng, meta["L"])
    return {"groundstate": psi, "environments": Environments(eng), "ham": H, "delta": meta["delta"], "config": simul}


def dim_state(psi: FiniteMPS):
    """bond dimensions in TensorKit `dim` units (src:1399-1405)"""
    if isinstance(psi, InfiniteMPS):
        return psi.bond_dimensions()
    return psi.engine.bond_dims()[1:]


def density_state(psi):
    """electrons per site <n_i> (src:1475-1523): all L sites of a finite chain, the unit cell of an infinite one
    (its sum / len equals the filling P/Q, the check at test/OB.jl:97-99)"""
    if isinstance(psi, InfiniteMPS):
        if psi.result is None:
            raise RuntimeError("run find_groundstate first")
        T = psi.result.unit_cell
        n, _ = psi.result.engine.site_occupations()
        return n[T // 2:T // 2 + T]
    if isinstance(psi, ThermalMPS):
        return _phys(psi, psi.engine.site_expectation("n"))
    return psi.engine.site_occupations()[0]


def density_spin(psi):
    """(n_up, n_dn) per site (src:1412-1456): spinful U(1) x U(1) mode only -- the SU(2) mode raises the reference's
    "This system is spin independent." -- finite chain: all sites, infinite chain: the unit cell"""
    if isinstance(psi, InfiniteMPS):
        if psi.result is None:
            raise RuntimeError("run find_groundstate first")
        T = psi.result.unit_cell
        up, dn = psi.result.engine.spin_occupations()
        return up[T // 2:T // 2 + T], dn[T // 2:T // 2 + T]
    if isinstance(psi, ThermalMPS):
        if psi.engine.sym.su2:
            raise ValueError("This system is spin independent.")                # the reference's error text (src:1424)
        return _phys(psi, (psi.engine.site_expectation("n_up"), psi.engine.site_expectation("n_dn")))
    return psi.engine.spin_occupations()


def calc_ms(psi):
    """staggered magnetisation |<n_up - n_dn>| of the first site (src:1458-1473; warns like the reference when the
    magnitude is not uniform)"""
    import warnings
    up, dn = density_spin(psi)
    mag = up - dn
    if not np.allclose(np.abs(mag), abs(mag[0]), rtol=1e-6, atol=1e-12):
        warnings.warn("Spin-density wave?")
    return float(abs(mag[0]))


def double_occupancy(psi):
    """<n_up n_dn> per site, same conventions as density_state"""
    if isinstance(psi, InfiniteMPS):
        T = psi.result.unit_cell
        return psi.result.engine.site_occupations()[1][T // 2:T // 2 + T]
    if isinstance(psi, ThermalMPS):
        return _phys(psi, psi.engine.site_expectation("docc"))
    return psi.engine.site_occupations()[1]


def correlation_function(psi, kind, connected=False):
    """Hermitian L x L matrix of two-point functions of a finite chain, measured on the device without moving the state:
    kind "hop": sum_s <c+_is c_js>, "nn": <n_i n_j>, "ss": <S_i . S_j>, "pair": <D+_i D_j>; spinful mode also "hop_up", "hop_dn",
    "szsz", "s+-", "s-+".  connected=True subtracts <n_i><n_j> ("nn") or <sz_i><sz_j> ("szsz")."""
    if isinstance(psi, InfiniteMPS):
        raise NotImplementedError("correlation functions need a chain length: they are measured on a finite chain "
                                  "(pass L= / use a FiniteMPS), not on an InfiniteMPS")
    return _phys(psi, psi.engine.correlator(kind, connected=connected))


def structure_factor(psi, kind, q, connected=True):
    """S(q) = (1 / L) sum_ij exp(i q (i - j)) C_ij of correlation_function(psi, kind); q scalar or array (radians per site).
    connected applies to the kinds that have a connected form ("nn", "szsz")."""
    Cm = correlation_function(psi, kind, connected=connected and kind in ("nn", "szsz"))
    L = Cm.shape[0]
    qs = np.atleast_1d(np.asarray(q, dtype=float))
    ph = np.exp(1j * qs[:, None] * np.arange(L)[None, :])                      # [q, i]
    S = np.einsum("qi,ij,qj->q", ph, Cm, ph.conj()) / L
    return S if np.ndim(q) else S[0]


def momentum_distribution(psi, q):
    """n(q) per spin: the "hop" structure factor halved (sum over q on the open-chain grid is not normalised: an open chain
    has no momentum eigenstates, this is the Fourier transform of the one-particle density matrix)"""
    return np.real(structure_factor(psi, "hop", q, connected=False)) / 2.0


def bond_correlation_function(psi, kind, connected=False):
    """Hermitian (L-1) x (L-1) matrix of correlation functions of nearest-neighbour bond operators of a finite chain, indexed by
    each bond's left site and measured on the device without moving the state: kind "bond": <B_i B_j> with the bond order
    B_i = sum_s (c+_{i s} c_{i+1 s} + h.c.), "dimer": <(S_i . S_{i+1}) (S_j . S_{j+1})>, "spair": <Delta+_i Delta_j> with the
    singlet bond pair Delta_i = (c_{i up} c_{i+1 dn} - c_{i dn} c_{i+1 up}) / sqrt 2 (not in the no-U(1) mode); spinful mode also
    "bond_up", "bond_dn", "dimer_zz", "dimer_xy".  connected=True ("bond", "dimer" and their components) subtracts <O_i><O_j>."""
    if isinstance(psi, InfiniteMPS):
        raise NotImplementedError("correlation functions need a chain length: they are measured on a finite chain "
                                  "(pass L= / use a FiniteMPS), not on an InfiniteMPS")
    if isinstance(psi, ThermalMPS):
        raise NotImplementedError("bond correlators of a ThermalMPS: physical neighbours are two chain sites apart in a purified "
                                  "state, the bond operators of this entry act on adjacent chain sites")
    return psi.engine.bond_correlator(kind, connected=connected)


def bond_structure_factor(psi, kind, q, connected=True):
    """S(q) = (1 / (L-1)) sum_ij exp(i q (i - j)) C_ij of bond_correlation_function(psi, kind) over the L - 1 bonds; q scalar or
    array (radians per site).  connected applies to the kinds that have a connected form (all but "spair")."""
    Cm = bond_correlation_function(psi, kind, connected=connected and kind != "spair")
    n = Cm.shape[0]
    qs = np.atleast_1d(np.asarray(q, dtype=float))
    ph = np.exp(1j * qs[:, None] * np.arange(n)[None, :])                      # [q, i]
    S = np.einsum("qi,ij,qj->q", ph, Cm, ph.conj()) / n
    return S if np.ndim(q) else S[0]


# ---- perfect sampling: occupation snapshots, full counting statistics ---------------------------------------------------
class Samples:
    """result of sample: .multiplets int32[n, L] (indices into the symmetry's site multiplets: empty / singly / doubly occupied in
    the SU(2) kinds, empty / up / dn / up dn in the spinful kind), .log_prob [n] (logarithm of the exact probability of each drawn
    configuration), .sites (the chain sites behind the columns); .electrons and .sz are derived from the multiplets"""

    def __init__(self, multiplets, log_prob, sites, sym):
        self.multiplets, self.log_prob, self.sites, self.sym = multiplets, log_prob, sites, sym

    @property
    def electrons(self):
        """n_i of every snapshot: int[n, L]"""
        return np.asarray(self.sym.site_electrons, dtype=np.int64)[self.multiplets]

    @property
    def sz(self):
        """S^z_i of every snapshot (spinful U(1) x U(1) kind only: an SU(2) multiplet leaves the spin of a singly occupied site
        unmeasured)"""
        if self.sym.su2:
            raise ValueError("This system is spin independent.")                # the reference's error text (src:1424)
        return np.array([0.0, 0.5, -0.5, 0.0])[self.multiplets]

    def __len__(self):
        return len(self.log_prob)


def sample(psi, n_samples, seed=0, batch=None):
    """n_samples independent snapshots of the site occupations of a finite chain, each drawn with its exact probability
    <psi|prod_i P_{s_i}|psi> by perfect sampling on the device (engine.DMRG2.sample) -> Samples.  The uniforms are
    numpy.random.default_rng(seed).random((n_samples, chain sites)), so a seed names its snapshots.  Any diagonal n-point
    function -- full counting statistics, string correlations, n-point density correlations -- is a mean over the snapshots.
    psi with its centre on site 0 (as after a sweep) is only read; otherwise a copy() with the centre on site 0 is sampled, for which
    psi's centre is carried to site 0 and back by exact moves (the same state to rounding).  A ThermalMPS is sampled with its
    ancillas traced out and reports its physical sites: finite-temperature snapshots."""
    if isinstance(psi, InfiniteMPS):
        raise NotImplementedError("sampling needs a chain length: snapshots are drawn on a finite chain "
                                  "(pass L= / use a FiniteMPS), not on an InfiniteMPS")
    eng = psi.engine
    if eng.centre() != 0:
        c = eng.centre()
        eng.move_centre(0)              # (copy() goes through the tensors with the centre on site 0; the moves are exact)
        work = eng.copy()
        eng.move_centre(c)
        eng = work
    u = np.random.default_rng(seed).random((int(n_samples), eng.L))
    thermal = isinstance(psi, ThermalMPS)
    measure = (np.arange(eng.L) % 2 == 0) if thermal else None
    occ, logp = eng.sample(u, measure=measure, batch=batch)
    sites = np.arange(0, eng.L, 2) if thermal else np.arange(eng.L)
    return Samples(np.ascontiguousarray(occ[:, sites]), logp, sites, eng.sym)


def full_counting_statistics(samples, region):
    """histogram of the particle number in `region` (indices into the columns of samples) -> (N values 0 .. 2 |region|, their
    relative frequencies, binomial standard errors sqrt(f (1 - f) / n)).  Host only."""
    region = np.atleast_1d(np.asarray(region, dtype=np.int64))
    N = samples.electrons[:, region].sum(axis=1)
    values = np.arange(2 * len(region) + 1)
    n = len(N)
    f = np.bincount(N, minlength=len(values))[:len(values)] / max(n, 1)
    return values, f, np.sqrt(f * (1.0 - f) / max(n, 1))


# ---- local operators on a finite MPS: G(x, t) and spectral functions ------------------------------------------------
def apply_operator(psi, name, site):
    """a new FiniteMPS holding O_site |psi> for the site operator `name` of the state's symmetry ("c", "c+" = "cdag", "n", "S";
    spinful mode "c_up", "c+_up", ...; or an abi.SiteOp).  psi (centre on site 0, as after a sweep) is copied, the copy's centre
    is carried to `site` without optimisation and the operator applied there on the device (engine.DMRG2.apply_op); psi itself
    is untouched.  The result is not normalised: <O_x psi|O_y psi> = sum over the operator's components of <psi|O+_xq O_yq|psi>,
    so for "c" the overlap matrix of the applied states is correlation_function(psi, "hop").  In the SU(2) modes psi must have
    total spin 0 unless the operator is a scalar."""
    if isinstance(psi, InfiniteMPS):
        raise NotImplementedError("apply_operator needs a chain length: operators are applied to a finite chain "
                                  "(pass L= / use a FiniteMPS), not to an InfiniteMPS")
    _no_thermal(psi, "apply_operator")
    if not 0 <= int(site) < psi.L:
        raise ValueError(f"apply_operator: site {site} out of range (the chain has {psi.L} sites)")
    work = psi.engine.copy()
    work.move_centre(int(site))
    return FiniteMPS(work.apply_op(int(site), name), psi.L)


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
    if isinstance(psi0, InfiniteMPS) or isinstance(H, InfiniteHamiltonian):
        raise NotImplementedError("greens_function needs a chain length: it is measured on a finite chain, not on an InfiniteMPS")
    _no_thermal(psi0, "greens_function")
    L = psi0.L
    site = L // 2 if site is None else int(site)
    times = [float(t) for t in times]
    phi = apply_operator(psi0, op, site)
    phi.engine.move_centre(0)
    eng = _tdvp_setup(phi, H, alg)
    step = _tdvp_step(eng, alg)
    ref = psi0.engine.copy()            # (bond_energies moves the centre through the chain: not on the caller's state)
    if H is not None and H is not ref.mpo and H is not ref.cmpo:
        ref.set_mpo(H)
    E0, _ = ref.bond_energies()
    Cm = np.zeros((len(times), L), dtype=np.complex128)
    tw = np.zeros(len(times))
    Cm[0] = psi0.engine.transition(op, eng)
    for k in range(1, len(times)):
        k0 = len(eng.stats)
        step(times[k] - times[k - 1])
        tw[k] = float(sum(s.trunc_weight for s in eng.stats[k0:]))
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
    qs, ws = np.atleast_1d(np.asarray(q, dtype=float)), np.atleast_1d(np.asarray(omegas, dtype=float))
    ph = np.exp(-1j * qs[:, None] * (np.arange(L) - res["site"])[None, :])        # [q, x]
    Cq = ph @ Cm.T                                                                # [q, t]
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
    if isinstance(psi0, InfiniteMPS) or isinstance(H, InfiniteHamiltonian):
        raise NotImplementedError("correction_vector needs a chain length: it is solved on a finite chain, not on an InfiniteMPS")
    _no_thermal(psi0, "correction_vector")
    if not isinstance(alg, CorrectionVector):
        raise TypeError("correction_vector takes alg = CorrectionVector(...)")
    if part not in ("particle", "hole"):
        raise ValueError("part must be 'particle' or 'hole'")
    L = psi0.L
    site = L // 2 if site is None else int(site)
    omegas = [float(w) for w in np.atleast_1d(omegas)]
    eta = float(eta)
    b = apply_operator(psi0, op, site)
    b.engine.move_centre(0)             # (its norm now sits beside normalised tensors: the amplitude of b)
    ref = psi0.engine.copy()            # (bond_energies moves the centre through the chain: not on the caller's state)
    if H is not None and H is not ref.mpo and H is not ref.cmpo:
        ref.set_mpo(H)
        b.engine.set_mpo(H)
    E0, _ = ref.bond_energies()
    x = b.engine.copy()                 # start value: b itself, normalised
    if isinstance(alg.trscheme, truncdim):
        x.chi_full, x.cutoff = int(alg.trscheme.D), 0.0
    elif isinstance(alg.trscheme, truncbelow):
        x.chi_full, x.cutoff = None, float(alg.trscheme.eta)
    elif alg.trscheme is None:
        x.chi_full, x.cutoff = None, 0.0
    else:
        raise TypeError("trscheme must be truncdim(D) or truncbelow(eta)")
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
    qs = np.atleast_1d(np.asarray(q, dtype=float))
    ph = np.exp(-1j * qs[:, None] * (np.arange(L) - res["site"])[None, :])        # [q, x]
    A = -(ph @ G.T).imag / np.pi
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
    if isinstance(psi, InfiniteMPS):
        raise NotImplementedError("thermal_greens_function needs a chain length: thermal states live on a finite chain, not on an "
                                  "InfiniteMPS")
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
    work = psi.engine.copy()
    work.move_centre(2 * site)
    ket = work.apply_op(2 * site, op)
    ket.move_centre(0)                  # (its norm now sits beside normalised tensors: the amplitude, applied by `transition`)
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
            k0 = len(eng.stats)
            for dt in seeds + [h - sum(seeds)]:
                eng.tdvp_sweep(dt)
            tw[k, j] = float(sum(s.trunc_weight for s in eng.stats[k0:]))
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


# ---- energy variance and extrapolation ---------------------------------------------------------------------------------
def energy_variance(psi, H=None):
    """two-site energy variance of a FiniteMPS (Hubig, Haegeman, Schollwoeck, PRB 97, 045125) -> result with .total, .site [L],
    .bond [L - 1] and .energy = <psi|H|psi>; total = sum(site) + sum(bond) is <H^2> - <H>^2 of the normalised state exactly for an
    MPO of range 1 (nearest-neighbour terms) and a lower bound for longer range.  It is the convergence measure of a state that
    was never truncated (one-site sweeps, applied and evolved states) and the abscissa of `extrapolate_energy`.  Measured on the
    device by engine.DMRG2.variance; psi is the same state afterwards, in the same gauge position.  H other than the state's
    current MPO replaces it first (engine.DMRG2.set_mpo: centre on site 0), as in time_evolve."""
    if isinstance(psi, InfiniteMPS) or isinstance(H, InfiniteHamiltonian):
        raise NotImplementedError("energy_variance needs a chain length: it is measured on a finite chain "
                                  "(pass L= / use a FiniteMPS), not on an InfiniteMPS")
    _no_thermal(psi, "energy_variance")
    eng = psi.engine
    if H is not None and H is not eng.mpo and H is not eng.cmpo:
        eng.set_mpo(H)
    return eng.variance()


class Extrapolation:
    """result of extrapolate_energy: the line E = E0 + slope * variance"""

    def __init__(self, E0, slope, residual):
        self.E0, self.slope, self.residual = E0, slope, residual

    def __iter__(self):
        return iter((self.E0, self.slope, self.residual))

    def __repr__(self):
        return f"Extrapolation(E0={self.E0:.12g}, slope={self.slope:.6g}, residual={self.residual:.3e})"


def extrapolate_energy(energies, variances):
    """least-squares line through (variance, energy) pairs of states of growing bond dimension: -> Extrapolation with .E0 (the
    intercept, E at variance 0), .slope and .residual (the 2-norm of the misfit; 0 for two points).  Host only.  The energy
    error of a variational state is linear in its variance to leading order, which makes the variance the abscissa of choice."""
    E, v = np.asarray(energies, dtype=float).ravel(), np.asarray(variances, dtype=float).ravel()
    if E.shape != v.shape or E.size < 2:
        raise ValueError("extrapolate_energy: needs at least two (energy, variance) pairs of equal number")
    if np.ptp(v) == 0.0:
        raise ValueError("extrapolate_energy: all variances are equal, the line is not determined")
    vm, Em = v.mean(), E.mean()
    slope = float(np.sum((v - vm) * (E - Em)) / np.sum((v - vm) ** 2))
    E0 = float(Em - slope * vm)
    return Extrapolation(E0, slope, float(np.linalg.norm(E - (E0 + slope * v))))


def TruncState(simul: Simulation, trunc_dim: int, trunc_scheme: int = 0, L: int | None = None, polish: str = "twosite", **kw):
    """truncated approximation of the ground state at bond dimension `trunc_dim` (TensorKit dim units), src:1351-1367.
    trunc_scheme 1 = SvdCut (truncate by SVD only); 0 = VUMPSSvdCut (truncate, then re-optimise variationally at
    that dimension -- here: further two-site sweeps with truncdim(trunc_dim), or, on a finite chain with
    polish="onesite", one-site sweeps at the bond tables the cut left).  Finite chains (L given) and the infinite
    chain: scheme 1 cuts the bonds of the converged window, scheme 0 = IDMRG2 at truncdim(trunc_dim)."""
    if polish not in ("twosite", "onesite"):
        raise ValueError('polish should be either "twosite" or "onesite".')
    if trunc_dim <= 0:
        raise ValueError("trunc_dim should be a positive integer.")
    if trunc_scheme not in (0, 1):
        raise ValueError("trunc_scheme should be either 0 (VUMPSSvdCut) or 1 (SvdCut).")
    L = L or simul.kwargs.get("L")
    if L is None:
        if trunc_scheme == 1:
            # SvdCut of the infinite state (test/MB.jl:95-103): every bond inside the converged window -- two unit cells between
            # the environments of the half-infinite blocks -- is cut to truncdim(trunc_dim) by its own Schmidt decomposition,
            # without re-optimisation; the energy density moves by the window's energy change per site
            d = compute_groundstate(simul, **kw)
            psi = d["groundstate"]
            r, eng = psi.result, psi.result.engine
            E_before, _ = eng.bond_energies()
            E_after = eng.svd_cut(trunc_dim)
            r.bond_dims = eng.bond_dims()
            r.energy_per_site += (E_after - E_before) / eng.L
            r.spectrum = eng.spectrum(r.unit_cell)
            return {"ψ_trunc": psi, "envs_trunc": Environments(eng)}
        d = compute_groundstate(simul, chi=trunc_dim, **kw)
        return {"ψ_trunc": d["groundstate"], "envs_trunc": d["environments"]}
    d = produce_groundstate(simul, L=L, **kw)
    psi = d["groundstate"]
    eng = psi.engine
    eng.svd_cut(trunc_dim)
    if trunc_scheme == 0:
        E_prev = None
        for _ in range(kw.get("maxiter", 20)):
            E = eng.sweep1() if polish == "onesite" else eng.sweep()
            if E_prev is not None and abs(E - E_prev) / psi.L < kw.get("tol", 1e-6):
                break
            E_prev = E
    return {"ψ_trunc": psi, "envs_trunc": Environments(eng)}


def produce_TruncState(simul: Simulation, trunc_dim: int, trunc_scheme: int = 0, force: bool = False, **kw):
    """src:1378-1385 without the DrWatson disk cache"""
    return TruncState(simul, trunc_dim, trunc_scheme=trunc_scheme, **kw)
