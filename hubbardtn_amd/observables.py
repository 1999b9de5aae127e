"""What is measured on a state without changing it (host API, re-exported by api.py): bond dimensions, densities, two-point and
bond-operator correlation functions and their structure factors, perfect sampling, the energy variance and the extrapolation in it.
Every device pass is a method of engine.DMRG2; this module picks the physical sites of a ThermalMPS, the unit cell of an InfiniteMPS,
and does the Fourier sums on the host.
"""
from __future__ import annotations

import numpy as np

from .states import FiniteMPS, InfiniteMPS, ThermalMPS, _needs_chain, _no_thermal, _ON_A_FINITE_CHAIN, _phys


def _other_mpo(eng, H):
    """True if H is a Hamiltonian other than the one attached to the engine (None: keep what is attached)"""
    return H is not None and H is not eng.mpo and H is not eng.cmpo


def _fourier_phases(q, x, sign):
    """exp(sign i q x) as an array [q, x] for q a scalar or an array (radians per site) and the positions x"""
    qs = np.atleast_1d(np.asarray(q, dtype=float))
    return np.exp((1j if sign > 0 else -1j) * qs[:, None] * x[None, :])


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
    _needs_chain(psi, None, "correlation functions need", "they are measured " + _ON_A_FINITE_CHAIN)
    return _phys(psi, psi.engine.correlator(kind, connected=connected))


def _structure(Cm, q):
    """(1 / n) sum_ij exp(i q (i - j)) C_ij of an n x n matrix; q scalar or array"""
    n = Cm.shape[0]
    ph = _fourier_phases(q, np.arange(n), +1)                                   # [q, i]
    S = np.einsum("qi,ij,qj->q", ph, Cm, ph.conj()) / n
    return S if np.ndim(q) else S[0]


def structure_factor(psi, kind, q, connected=True):
    """S(q) = (1 / L) sum_ij exp(i q (i - j)) C_ij of correlation_function(psi, kind); q scalar or array (radians per site).
    connected applies to the kinds that have a connected form ("nn", "szsz")."""
    return _structure(correlation_function(psi, kind, connected=connected and kind in ("nn", "szsz")), q)


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
    _needs_chain(psi, None, "correlation functions need", "they are measured " + _ON_A_FINITE_CHAIN)
    if isinstance(psi, ThermalMPS):
        raise NotImplementedError("bond correlators of a ThermalMPS: physical neighbours are two chain sites apart in a purified "
                                  "state, the bond operators of this entry act on adjacent chain sites")
    return psi.engine.bond_correlator(kind, connected=connected)


def bond_structure_factor(psi, kind, q, connected=True):
    """S(q) = (1 / (L-1)) sum_ij exp(i q (i - j)) C_ij of bond_correlation_function(psi, kind) over the L - 1 bonds; q scalar or
    array (radians per site).  connected applies to the kinds that have a connected form (all but "spair")."""
    return _structure(bond_correlation_function(psi, kind, connected=connected and kind != "spair"), q)


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
    _needs_chain(psi, None, "sampling needs", "snapshots are drawn " + _ON_A_FINITE_CHAIN)
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


# ---- energy variance and extrapolation ---------------------------------------------------------------------------------
def energy_variance(psi, H=None):
    """two-site energy variance of a FiniteMPS (Hubig, Haegeman, Schollwoeck, PRB 97, 045125) -> result with .total, .site [L],
    .bond [L - 1] and .energy = <psi|H|psi>; total = sum(site) + sum(bond) is <H^2> - <H>^2 of the normalised state exactly for an
    MPO of range 1 (nearest-neighbour terms) and a lower bound for longer range.  It is the convergence measure of a state that
    was never truncated (one-site sweeps, applied and evolved states) and the abscissa of `extrapolate_energy`.  Measured on the
    device by engine.DMRG2.variance; psi is the same state afterwards, in the same gauge position.  H other than the state's
    current MPO replaces it first (engine.DMRG2.set_mpo: centre on site 0), as in time_evolve."""
    _needs_chain(psi, H, "energy_variance needs", "it is measured " + _ON_A_FINITE_CHAIN)
    _no_thermal(psi, "energy_variance")
    eng = psi.engine
    if _other_mpo(eng, H):
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

