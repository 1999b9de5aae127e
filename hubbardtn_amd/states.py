"""What the host API (api.py) passes around: the truncation schemes and algorithm selectors (TensorKit / MPSKit names), the state
handles, and the decisions every entry makes the same way -- how a truncation scheme becomes (chi_full, cutoff), which states an
entry refuses.  observables.py and dynamics.py build on this module and on engine.py; api.py re-exports all of it.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import idmrg as _idmrg
from .models import Simulation


# ---- truncation schemes (TensorKit names; App. A.6) --------------------------------------------
@dataclass
class truncdim:
    """keep at most D in TensorKit `dim` units (sum (2S+1) n); used at src:1363-1365"""
    D: int


@dataclass
class truncbelow:
    """keep Schmidt values > eta; used at src:1010 with eta = 10^-svalue"""
    eta: float


_NO_TRUNCATION = (None, 0.0)


def _truncation(trscheme, none):
    """(chi_full, cutoff) of a truncation scheme, as the engine takes them.  none: what trscheme=None decodes to -- _NO_TRUNCATION
    where the selector's scheme is the whole truth (IDMRG2, TDVP2, CorrectionVector), None where the caller leaves the engine's
    settings alone then (DMRG2 on a finite chain)"""
    if isinstance(trscheme, truncdim):
        return int(trscheme.D), 0.0
    if isinstance(trscheme, truncbelow):
        return None, float(trscheme.eta)
    if trscheme is None:
        return none
    raise TypeError("trscheme must be truncdim(D) or truncbelow(eta)")


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


# ---- states ------------------------------------------------------------------------------------------------------------
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
    ensemble H - mu N the model defines.  The observables (observables.py) report its physical sites only."""
    n_phys: int = 0
    beta: float = 0.0
    log_z: float = 0.0
    seeded: bool = False        # cool() has put the first bond directions into the beta = 0 tables (SEED_STEPS)
    simul: object = None        # the model: the mirror scheme builds its generator from it
    mirror: object = None       # engine.CMpo of models.purified_hamiltonian(simul, n_phys, "mirror"), built on first use


@dataclass
class Environments:
    engine: object


SEED_STEPS = (1e-10, 1e-5)      # imaginary-time lengths of the two sweeps that open the bond tables of the beta = 0 state


def _phys(psi, x):
    """the physical sublattice of a per-site vector or a site x site matrix of a ThermalMPS; anything else unchanged"""
    if not isinstance(psi, ThermalMPS):
        return x
    if isinstance(x, tuple):
        return tuple(_phys(psi, v) for v in x)
    return x[::2] if np.ndim(x) == 1 else x[::2, ::2]


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _needs_chain(psi, H, what, tail):
    """the refusal of the entries that work on a finite chain only, for an InfiniteMPS or the Hamiltonian of the infinite chain (H
    None where the entry takes none).  what: the entry with its verb ("sampling needs"), tail: the rest of its sentence"""
    if isinstance(psi, InfiniteMPS) or isinstance(H, InfiniteHamiltonian):
        raise NotImplementedError(f"{what} a chain length: {tail}")


_ON_A_FINITE_CHAIN = "on a finite chain (pass L= / use a FiniteMPS), not on an InfiniteMPS"


def _no_thermal(psi, what):
    if isinstance(psi, ThermalMPS):
        raise NotImplementedError(f"{what} of a ThermalMPS is not available: dynamics at finite temperature needs the bra of the "
                                  "purification evolved as well (thermal_greens_function evolves both)")


def _refuse_sharded(ops, what):
    if bool(getattr(ops, "_cb", None)) or int(getattr(ops, "comm_world", 1)) > 1:
        raise NotImplementedError(f"{what}: thermal states are not available in a context with a communicator or an exchange "
                                  "hook")
