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

This module is the face: it holds what builds a state or reaches for the default context (`_ops`) -- Hamiltonians, initial states,
ground states, excitations, thermal states, the result cache's two ends -- and re-exports the rest under the names it always had:
states.py (truncation schemes, algorithm selectors, state handles), observables.py (what is measured on a state), dynamics.py
(what moves one: TDVP, cooling, applied operators, Green's and spectral functions).
"""
from __future__ import annotations

from dataclasses import dataclass, field  # noqa: F401  (api.dataclass / api.field were reachable before the split)

import numpy as np

from . import engine as _engine
from . import idmrg as _idmrg
from . import models, mps
from .dynamics import (_adjoint_pair, _mirror_mpo, _tdvp_setup, _tdvp_step, apply_operator, cool, correction_vector,  # noqa: F401
                       greens_function, purification_defect, spectral_function, spectral_function_cv, thermal_greens_function,
                       thermal_spectral_function, time_evolve, timestep)
from .models import MB_Sim, MBC_Sim, OB_Sim, OBC_Sim, OBC_Sim2, Simulation  # noqa: F401
from .observables import (Extrapolation, Samples, bond_correlation_function, bond_structure_factor, calc_ms,  # noqa: F401
                          correlation_function, density_spin, density_state, dim_state, double_occupancy, energy_variance,
                          extrapolate_energy, full_counting_statistics, momentum_distribution, sample, structure_factor)
from .states import (DMRG, DMRG2, IDMRG2, SEED_STEPS, TDVP, TDVP2, CorrectionVector, Environments, FiniteMPS,  # noqa: F401
                     InfiniteHamiltonian, InfiniteMPS, ThermalMPS, _NO_TRUNCATION, _no_thermal, _phys, _refuse_sharded, _truncation,
                     truncbelow, truncdim)


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
        chi, cut = _truncation(alg.trscheme, none=_NO_TRUNCATION)
        psi.result = _idmrg.idmrg2(psi.ops or _ops(), H.simul, chi_full=chi, cutoff=cut, tol=alg.tol,
                                   maxiter=alg.maxiter, sweeps_per_step=alg.sweeps_per_step,
                                   init_dimension=psi.max_dimension, krylovdim=alg.krylovdim,
                                   lanczos_tol=alg.eigsolve_tol, seed=psi.seed, verbosity=alg.verbosity,
                                   driver=alg.driver)
        return psi, Environments(psi.result.engine), psi.result.delta
    eng = psi.engine
    onesite = isinstance(alg, DMRG)     # one-site sweeps: the bond tables stay as they are, nothing is truncated
    if not onesite:
        cut = _truncation(alg.trscheme, none=None)
        if cut is not None:             # (trscheme=None leaves the engine's settings alone)
            eng.chi_full, eng.cutoff = cut
    eng.krylovdim, eng.lanczos_tol = alg.krylovdim, alg.eigsolve_tol
    label = "DMRG" if onesite else "DMRG2"

    def report(n, E, delta):
        print(f"{label} sweep {n}: E/L = {E / psi.L:.12f}  delta = {delta:.3e}  chi = {max(eng.bond_dims())}")
    _, delta = _sweep_until(eng.sweep1 if onesite else eng.sweep, psi.L, alg.tol, alg.maxiter, report if alg.verbosity else None)
    return psi, Environments(eng), delta


def _sweep_until(sweep, L, tol, maxiter, report=None):
    """sweep() -> E until E changes by less than tol per site between two sweeps, maxiter times at the most; report(n, E, delta)
    after the n-th sweep.  -> (E, delta) of the last sweep; delta is inf after a single sweep"""
    E, E_prev, delta = None, None, float("inf")
    for it in range(maxiter):
        E = sweep()
        if E_prev is not None:
            delta = abs(E - E_prev) / L
        if report is not None:
            report(it + 1, E, delta)
        E_prev = E
        if delta < tol:
            break
    return E, delta


# ---- finite temperature: purified thermal states cooled by two-site TDVP -----------------------------------------------
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
        def report(n, E, delta):
            print(f"state {k} sweep {n}: E = {E:.12f}")
        E, _ = _sweep_until(eng.sweep, L, tol, maxiter, report if verbosity else None)
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
        _sweep_until(eng.sweep1 if polish == "onesite" else eng.sweep, psi.L, kw.get("tol", 1e-6), kw.get("maxiter", 20))
    return {"ψ_trunc": psi, "envs_trunc": Environments(eng)}


def produce_TruncState(simul: Simulation, trunc_dim: int, trunc_scheme: int = 0, force: bool = False, **kw):
    """src:1378-1385 without the DrWatson disk cache"""
    return TruncState(simul, trunc_dim, trunc_scheme=trunc_scheme, **kw)
