"""Thin Python face of the C++ sweep engine (hubbardtn_amd/csrc/htn_engine.cpp and the files around it, behind include/hubbardtn_hip.h).

Everything below `find_groundstate(psi0, H, alg)` (src/HubbardFunctions.jl:1010) -- sector layouts, recoupling
coefficients, task lists, theta formation, Lanczos, per-sector SVD, the global truncation rule, write-back,
environment transfer, the sweep loop -- runs inside the library (`htn_mps_create`, `htn_bond_update`,
`htn_dmrg2_sweep`).  This module only converts the host-side model (list of models.MPOSite) and the initial state
(bond tables + block dictionaries) into the ABI's tables and reads results back.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi
from .models import SU2U1
from .sectors import Bond


@dataclass
class BondStats:
    bond: int
    direction: int
    energy: float
    n_matvec: int
    residual: float
    trunc_weight: float
    chi_full: int
    multiplets: int
    theta_size: int
    apply_flops: int
    apply_bytes: int
    svd_flops: int
    jacobi_sweeps: int
    n_tiles: int
    n_segs: int
    t_plan: float = 0.0
    t_total: float = 0.0
    t_lanczos: float = 0.0
    t_svd: float = 0.0
    t_env: float = 0.0
    matvec_ms: float = 0.0


def _stats(rec) -> BondStats:
    return BondStats(**{k: (float(rec[k]) if rec.dtype[k].kind == "f" else int(rec[k])) for k in rec.dtype.names})


def _side(letter) -> int:
    """the library's index of an environment side: 'L' -> 0, anything else ('R') -> 1"""
    return 0 if letter == "L" else 1


class CMpo:
    """htn_mpo handle built from a models.MPO (list of MPOSite + symmetry; a plain list means SU(2) x U(1) x fZ2)"""

    def __init__(self, ops, sites):
        self.ops, self.lib = ops, ops.lib
        self.sym = msym = getattr(sites, "sym", SU2U1)
        SITE_MULT, SITE_OPS = msym.site_mult, msym.site_ops
        names = sorted({e[2] for s in sites for e in s.entries})
        self.op_index = {n: k for k, n in enumerate(names)}
        optab = np.zeros(max(len(names), 1), dtype=abi.SITE_OP_DT)
        for n, k in self.op_index.items():
            kk, dN, red = SITE_OPS[n]
            optab[k]["k"], optab[k]["dN"] = kk, dN
            r = np.zeros((abi.MAX_SITE, abi.MAX_SITE))
            r[:red.shape[0], :red.shape[1]] = red
            optab[k]["red"] = r.reshape(-1)
        n = len(sites)
        levels, level_ptr = [], [0]
        bonds = [sites[0].left] + [s.right for s in sites]
        for i in range(1, n):
            if list(sites[i].left) != list(sites[i - 1].right):
                raise ValueError(f"MPO bond {i}: left levels of site {i} differ from right levels of site {i - 1}")
        for lv in bonds:
            levels.extend(lv)
            level_ptr.append(level_ptr[-1] + len(lv))
        ent = np.zeros(max(sum(len(s.entries) for s in sites), 1), dtype=abi.MPO_ENTRY_DT)
        entry_ptr, q = [0], 0
        for s in sites:
            for (wl, wr, name, coef) in s.entries:
                c = complex(coef)
                ent[q] = (wl, wr, self.op_index[name], 0, c.real, c.imag)
                q += 1
            entry_ptr.append(q)
        sym = abi.Symmetry()
        sym.kind, sym.n_site = msym.kind, len(SITE_MULT)
        for s, (N, j) in enumerate(SITE_MULT):
            sym.site_N[s], sym.site_j[s] = N, j
        lv = np.ascontiguousarray(np.array(levels, dtype=np.int32).reshape(-1, 2))
        lp = np.array(level_ptr, dtype=np.int32)
        ep = np.array(entry_ptr, dtype=np.int32)
        h = C.c_void_p()
        abi.check(self.lib, self.lib.htn_mpo_create(ops.ctx, C.byref(sym), n, optab.ctypes.data, len(names), lp.ctypes.data,
                                                    lv.ctypes.data, ep.ctypes.data, ent.ctypes.data, C.byref(h)),
                  "htn_mpo_create")
        self.handle = h
        self.sites = sites

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            self.lib.htn_mpo_destroy(h)


def sweep_opts(chi_full=None, cutoff=0.0, krylovdim=30, lanczos_tol=1e-12, maxrestart=3, weighting="sqrtdim",
               jacobi_tol=1e-14, jacobi_max_sweeps=40, svd_split=0, rank_cut=0.0, profile=False) -> abi.SweepOpts:
    """htn_sweep_opts of the engine's keyword options"""
    o = abi.SweepOpts()
    o.chi_full = int(chi_full) if chi_full else 0
    o.weighting = 0 if weighting == "sqrtdim" else 1
    o.cutoff = float(cutoff)
    o.krylovdim, o.maxrestart, o.lanczos_tol = int(krylovdim), int(maxrestart), float(lanczos_tol)
    o.jacobi_tol, o.jacobi_max_sweeps = float(jacobi_tol), int(jacobi_max_sweeps)
    o.svd_split_elems, o.rank_cut, o.profile = int(svd_split), float(rank_cut), 1 if profile else 0
    return o


class StateTables:
    """an MPS as the ABI's tables (htn_mps_create / htn_idmrg_step): bond_ptr, sectors, sub_ptr, subs, data_ptr, data"""

    def __init__(self, bond_ptr, sectors, sub_ptr, subs, data_ptr, data):
        self.arrays = (bond_ptr, sectors, sub_ptr, subs, data_ptr, data)

    def pointers(self):
        return [a.ctypes.data for a in self.arrays]


def state_tables(bonds, tensors) -> StateTables:
    """bonds: list of {sector: count} for bonds 0..L; tensors: list of {(l, s, r): ndarray[n_l, n_r]}"""
    bond_ptr, secs = [0], []
    for b in bonds:
        items = sorted((k, int(v)) for k, v in dict(b).items() if v > 0)
        secs.extend((N, j, n) for (N, j), n in items)
        bond_ptr.append(len(secs))
    sec_arr = np.array(secs, dtype=np.int32).reshape(-1, 3).view(abi.SECTOR_DT).reshape(-1)
    subs, sub_ptr, data_ptr, chunks, pos = [], [0], [0], [], 0
    for t in tensors:
        off = 0
        for (l, s, r), blk in t.items():
            blk = np.asarray(blk, dtype=np.complex128)
            m, n = blk.shape
            subs.append((l[0], l[1], s, r[0], r[1], m, off))
            chunks.append(np.asfortranarray(blk).reshape(-1, order="F"))
            off += m * n
        sub_ptr.append(len(subs))
        pos += off
        data_ptr.append(pos)
    sub_arr = np.array(subs, dtype=np.int64).reshape(-1, 7)
    sb = np.zeros(max(len(subs), 1), dtype=abi.SUBBLOCK_DT)
    if len(subs):
        for k, f in enumerate(("lN", "lj", "s", "rN", "rj", "ld", "off")):
            sb[f] = sub_arr[:, k]
    data = np.concatenate(chunks) if chunks else np.zeros(1, dtype=np.complex128)
    return StateTables(np.array(bond_ptr, dtype=np.int32), np.ascontiguousarray(sec_arr), np.array(sub_ptr, dtype=np.int32), sb,
                       np.array(data_ptr, dtype=np.int64), data)


class Variance:
    """result of DMRG2.variance / api.energy_variance"""

    def __init__(self, total, site, bond, energy, split=None):
        self.total, self.site, self.bond, self.energy, self.split = total, site, bond, energy, split

    def __repr__(self):
        return f"Variance(total={self.total:.6e}, energy={self.energy:.12g})"


class DMRG2:
    """finite two-site DMRG on reduced SU(2) x U(1) tensors -- handle of an `htn_mps` inside the library.

    ops        : context provider (hubbardtn_amd.device.HipOps in the product; `.lib`, `.ctx`)
    mpo        : list[models.MPOSite]
    bonds      : list of {sector: count} for bonds 0..L (initial state)
    tensors    : list of {(l, s, r): ndarray[n_l, n_r]} right-canonical initial site tensors
    chi_full   : truncdim(D) in TensorKit's `dim` units (sum (2S+1) n), or None
    cutoff     : truncbelow(eta) Schmidt-value cut (10^-svalue, src:1007), or 0
    left_env / right_env : boundary environments (flat arrays in the library's block order, `env_data`) of an iDMRG
                 window; None = open end
    Sharding (sector-parallel apply) is a property of the context: HipOps.set_comm / set_exchange.
    """

    def __init__(self, ops, mpo, bonds, tensors, chi_full=None, cutoff=0.0, krylovdim=30, lanczos_tol=1e-12,
                 maxrestart=3, weighting="sqrtdim", jacobi_tol=1e-14, jacobi_max_sweeps=40, left_env=None, right_env=None):
        self._setup(ops, mpo, chi_full, cutoff, krylovdim, lanczos_tol, maxrestart, weighting, jacobi_tol, jacobi_max_sweeps)
        tab = state_tables(bonds, tensors)
        le = None if left_env is None else np.ascontiguousarray(left_env, dtype=np.complex128)
        re_ = None if right_env is None else np.ascontiguousarray(right_env, dtype=np.complex128)
        h = C.c_void_p()
        abi.check(self.lib, self.lib.htn_mps_create(ops.ctx, self.cmpo.handle, self.L, *tab.pointers(),
                                                    None if le is None else le.ctypes.data,
                                                    None if re_ is None else re_.ctypes.data, C.byref(h)),
                  "htn_mps_create")
        self.handle = h

    @classmethod
    def wrap(cls, ops, mpo, handle, chi_full=None, cutoff=0.0, krylovdim=30, lanczos_tol=1e-12, maxrestart=3,
             weighting="sqrtdim", jacobi_tol=1e-14, jacobi_max_sweeps=40):
        """an engine around an existing `htn_mps` handle (e.g. the window of the native IDMRG2 driver, htn_idmrg_window).
        The engine takes over that reference (released in __del__); mpo: the CMpo the handle was built on."""
        self = cls.__new__(cls)
        self._setup(ops, mpo, chi_full, cutoff, krylovdim, lanczos_tol, maxrestart, weighting, jacobi_tol, jacobi_max_sweeps)
        if self.lib.htn_mps_nsites(handle) != self.L:
            raise ValueError("DMRG2.wrap: the handle's chain length differs from the MPO's")
        self.handle = handle
        return self

    def _setup(self, ops, mpo, chi_full, cutoff, krylovdim, lanczos_tol, maxrestart, weighting, jacobi_tol, jacobi_max_sweeps):
        self.ops, self.lib = ops, ops.lib
        self.cmpo = mpo if isinstance(mpo, CMpo) else CMpo(ops, mpo)
        self.mpo = self.cmpo.sites
        self.sym = self.cmpo.sym
        self.L = len(self.mpo)
        self.chi_full, self.cutoff, self.weighting = chi_full, cutoff, weighting
        self.krylovdim, self.lanczos_tol, self.maxrestart = krylovdim, lanczos_tol, maxrestart
        self.jacobi_tol, self.jacobi_max_sweeps = jacobi_tol, jacobi_max_sweeps
        self.rank_cut = 0.0          # optional rank-revealing QR cut (OFF: the 1e-8 spectra parity needs it off), DESIGN.md 4
        self.svd_split = 0           # tests: force small blocks through the large-block SVD path
        self.profile = False
        self.energy = None
        self.stats = []

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            self.lib.htn_mps_destroy(h)

    def _check(self, rc, what):
        """status of a library call that may have run the context's exchange hook: an exception raised inside the hook
        (stored by the context provider, the C side only saw "failed") is re-raised here in preference to the generic
        library error"""
        chk = getattr(self.ops, "check_exchange", None)
        if chk is not None:
            chk()
        abi.check(self.lib, rc, what)

    # ---- excited states: orthogonalised sweeps (htn_mps_set_orthogonal) --------------------------------
    def set_orthogonal(self, others=()):
        """keep every optimising update in the orthogonal complement of the given engines' states (same context, symmetry,
        chain length and total sector; at most 8; krylovdim + len(others) <= 31).  They must not be swept while attached;
        an empty list detaches.  The library holds its own references to the attached states."""
        others = list(others)
        arr = (C.c_void_p * max(len(others), 1))(*[o.handle for o in others])
        self._check(self.lib.htn_mps_set_orthogonal(self.handle, arr, len(others)), "htn_mps_set_orthogonal")
        self.attached = others

    def overlap(self, other) -> complex:
        """<self|other> by a transfer pass on the device"""
        out = (C.c_double * 2)()
        self._check(self.lib.htn_mps_overlap(self.handle, other.handle, out), "htn_mps_overlap")
        return complex(out[0], out[1])

    def dropped_projectors(self) -> int:
        """projector rows the last bond update dropped as numerically dependent on the others"""
        d = C.c_int32(0)
        self.lib.htn_mps_orthogonal_count(self.handle, C.byref(d))
        return d.value

    # ---- options ----------------------------------------------------------------------------------
    def _opts(self, cutoff=None):
        return sweep_opts(self.chi_full, self.cutoff if cutoff is None else cutoff, self.krylovdim, self.lanczos_tol,
                          self.maxrestart, self.weighting, self.jacobi_tol, self.jacobi_max_sweeps, self.svd_split,
                          self.rank_cut, self.profile)

    # ---- state queries ----------------------------------------------------------------------------
    @property
    def bonds(self):
        return [self.bond(b) for b in range(self.L + 1)]

    def _table(self, fn, dtype, *args, missing=None):
        """rows of one of the library's two-call table readers: fn(handle, *args, None) -> count, the same call with a buffer
        fills it.  missing: the text of the HtnError a negative count raises (without it the count is used as it comes)"""
        n = fn(self.handle, *args, None)
        if missing is not None and n < 0:
            raise abi.HtnError(missing)
        arr = np.zeros(max(n, 1), dtype=dtype)
        fn(self.handle, *args, arr.ctypes.data)
        return arr[:n]

    def _sector_bond(self, rows) -> Bond:
        return Bond({(int(r["N"]), int(r["j"])): int(r["count"]) for r in rows}, self.sym)

    def bond(self, b) -> Bond:
        return self._sector_bond(self._table(self.lib.htn_mps_bond, abi.SECTOR_DT, b))

    def bond_dims(self):
        """`dim_state` analogue (src/HubbardFunctions.jl:1399-1405): TensorKit dim of each bond"""
        return [b.dim_full for b in self.bonds]

    @property
    def spectra(self):
        return {b: s for b in range(1, self.L) for s in [self.spectrum(b)] if s}

    def spectrum(self, b):
        """Schmidt values of the last update of bond b: {sector: descending array}"""
        n = self.lib.htn_mps_spectrum(self.handle, b, None, None)
        if n <= 0:
            return {}
        secs = np.zeros(n, dtype=abi.SECTOR_DT)
        vals = np.zeros(n)
        self.lib.htn_mps_spectrum(self.handle, b, secs.ctypes.data, vals.ctypes.data)
        out, pos = {}, 0
        for r in secs:
            if pos >= n:
                break
            c = int(r["count"])
            out[(int(r["N"]), int(r["j"]))] = vals[pos:pos + c].copy()
            pos += c
        return out

    def download_site(self, i):
        """{(l, s, r): ndarray[n_l, n_r]} of site i as stored (left or right layout)"""
        nb = self.lib.htn_mps_get_site(self.handle, i, None, None)
        size = self.lib.htn_mps_site_size(self.handle, i, None)
        subs = np.zeros(max(nb, 1), dtype=abi.SUBBLOCK_DT)
        flat = np.zeros(max(size, 1), dtype=np.complex128)
        if self.lib.htn_mps_get_site(self.handle, i, subs.ctypes.data, flat.ctypes.data) < 0:
            raise abi.HtnError(self.lib.htn_last_error().decode())
        out = {}
        for sb in subs[:nb]:
            l, r = (int(sb["lN"]), int(sb["lj"])), (int(sb["rN"]), int(sb["rj"]))
            m, n = self.bond_of_site(i, 0)[l], self.bond_of_site(i, 1)[r]
            idx = int(sb["off"]) + np.arange(m)[:, None] + int(sb["ld"]) * np.arange(n)[None, :]
            out[(l, int(sb["s"]), r)] = flat[idx].copy()
        return out

    def bond_of_site(self, i, side):
        key = ("_b", i + side)
        cache = self.__dict__.setdefault("_bond_cache", {})
        # bonds change with every update: the cache is dropped by _step / _sweep (and by variance)
        if key not in cache:
            cache[key] = self.bond(i + side)
        return cache[key]

    def _drop_bond_cache(self):
        self.__dict__.pop("_bond_cache", None)

    def site_kind(self, i):
        k = C.c_int32(0)
        self.lib.htn_mps_site_size(self.handle, i, C.byref(k))
        return chr(k.value)

    def env_data(self, side, b):
        """flat environment (library block order) on bond b; side 'L' / 'R'"""
        sd = _side(side)
        n = self.lib.htn_mps_env_size(self.handle, sd, b)
        if n < 0:
            raise abi.HtnError(f"environment {side} of bond {b} does not exist")
        flat = np.zeros(max(n, 1), dtype=np.complex128)
        abi.check(self.lib, self.lib.htn_mps_get_env(self.handle, sd, b, flat.ctypes.data), "htn_mps_get_env")
        return flat[:n]

    def env_bond(self, side, b) -> Bond:
        """the bond table the environment on bond b was built on (left: last rightward update of that bond, right: last
        leftward update -- a truncation by dimension may keep different counts in between)"""
        return self._sector_bond(self._table(self.lib.htn_mps_env_bond, abi.SECTOR_DT, _side(side), b,
                                             missing=f"environment {side} of bond {b} does not exist"))

    def download_env(self, side, b):
        """{(x, w, y): matrix}: left env keys (bra, w, ket) -> [n_bra, n_ket]; right env (ket, w, bra) -> [n_ket, n_bra]"""
        blk = self._table(self.lib.htn_mps_env_blocks, abi.ENV_BLOCK_DT, _side(side), b)
        flat = self.env_data(side, b)
        out = {}
        for r in blk:
            m, n, off = int(r["rows"]), int(r["cols"]), int(r["off"])
            out[((int(r["aN"]), int(r["aj"])), int(r["w"]), (int(r["bN"]), int(r["bj"])))] = \
                flat[off:off + m * n].reshape(n, m).T.copy()
        return out

    def theta(self, i):
        n = self.lib.htn_mps_theta_size(self.handle, i)
        out = np.zeros(n, dtype=np.complex128)
        abi.check(self.lib, self.lib.htn_mps_get_theta(self.handle, i, out.ctypes.data), "htn_mps_get_theta")
        return out

    def apply_heff(self, i, x):
        """y = H_eff(bond i, i+1) x on host vectors in the library's theta layout"""
        return self._apply_host("htn_heff2_apply", self.lib.htn_heff2_apply, lambda: self.lib.htn_mps_theta_size(self.handle, i), i, x)

    def _apply_host(self, what, fn, size, i, x):
        """y = fn(i) x, an effective Hamiltonian of the library applied to a host vector: upload, one call, download.  size():
        the elements the library expects (queried after x is converted; it may raise)"""
        x = np.ascontiguousarray(x, dtype=np.complex128)
        n = size()
        assert x.shape == (n,)
        y = np.zeros(n, dtype=np.complex128)
        self._check(fn(self.handle, i, x.ctypes.data, y.ctypes.data), what)
        return y

    def centre_energy(self):
        """<psi|H|psi> / <psi|psi> of the state as stored, read where the centre is when that is site 0 (after construction
        and after every sweep): one H_eff2 apply on bond 0 and a dot product of two host vectors; theta of bond 0 has left
        dimension 1, so both are tiny.  Nothing moves and nothing is decomposed (bond_energies costs a pass of SVD moves)."""
        if self.centre() != 0:
            raise ValueError("DMRG2.centre_energy: the centre must be on site 0")
        th = self.theta(0)
        return float(np.real(np.vdot(th, self.apply_heff(0, th))) / np.real(np.vdot(th, th)))

    def site_expectation(self, name):
        """ndarray[L]: <O_i> of the scalar site operator `name` ("n", "docc", spinful mode "n_up", "sz", ...) on every site by one
        correlator pass on the device; the state is only read (any centre position).  The pass is a full one -- the L x L
        channel with `name` as its one-site entry, of which only the diagonal is kept -- so a call costs what correlator() costs
        per channel: the C interface has no entry that measures the diagonal alone."""
        M, _ = self.correlator_channel(name, "id", name, name)
        return np.real(np.diag(M)).copy()

    def plan_apply_dump(self, i, stage):
        """(tiles, segs, z_size, flops) of the H_eff apply on bond i as the kernels receive them (tests)"""
        nt, nsg, zs, fl = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
        abi.check(self.lib, self.lib.htn_plan_apply_dump(self.handle, i, stage, C.byref(nt), None, C.byref(nsg), None,
                                                         C.byref(zs), C.byref(fl)), "htn_plan_apply_dump")
        tiles = np.zeros(max(nt.value, 1), dtype=abi.TILE_DT)
        segs = np.zeros(max(nsg.value, 1), dtype=abi.SEG_DT)
        abi.check(self.lib, self.lib.htn_plan_apply_dump(self.handle, i, stage, C.byref(nt), tiles.ctypes.data,
                                                         C.byref(nsg), segs.ctypes.data, C.byref(zs), C.byref(fl)),
                  "htn_plan_apply_dump")
        return tiles[:nt.value], segs[:nsg.value], zs.value, fl.value

    @property
    def cache_hits(self):
        return self._cache_stats()[0]

    @property
    def cache_misses(self):
        return self._cache_stats()[1]

    def _cache_stats(self):
        h, m = C.c_int64(0), C.c_int64(0)
        self.lib.htn_mps_cache_stats(self.handle, C.byref(h), C.byref(m))
        return h.value, m.value

    # ---- updates ----------------------------------------------------------------------------------
    def _step(self, what, call, record, cutoff=None, drop_cache=True, sets_energy=True) -> BondStats:
        """one single-update entry of the library, call(opts, stats) -> status, with its one record.  The updates differ in
        three things, which their wrappers state: whether the bond tables may change (drop_cache: the cache of bond_of_site goes
        before the call), whether a recorded update's `energy` is an energy of the state (sets_energy: it becomes self.energy),
        and what they return (the BondStats returned here, or its energy)."""
        if drop_cache:
            self._drop_bond_cache()
        st = np.zeros(1, dtype=abi.BOND_STATS_DT)
        o = self._opts(cutoff)
        self._check(call(C.byref(o), st.ctypes.data), what)
        s = _stats(st[0])
        if record:
            self.stats.append(s)
            if sets_energy:
                self.energy = s.energy
        return s

    def _sweep(self, what, n, call, sets):
        """one sweep entry of the library, call(opts, stats, *scalars) -> status, with its n records, which go to `stats`.
        sets: the attributes that take the call's scalar outputs (doubles), in the order of its arguments."""
        self._drop_bond_cache()
        st = np.zeros(n, dtype=abi.BOND_STATS_DT)
        out = [C.c_double(0.0) for _ in sets]
        o = self._opts()
        self._check(call(C.byref(o), st.ctypes.data, *[C.byref(v) for v in out]), what)
        self.stats.extend(_stats(r) for r in st)
        for name, v in zip(sets, out):
            setattr(self, name, v.value)

    def update_bond(self, i, direction, placement, optimise=True, record=True, cutoff=None):
        """optimise sites (i, i+1); placement 'right': A_i = U, centre S V^H on i+1 (+ left env); 'left': centre U S on
        i, B_{i+1} = V^H (+ right env).  optimise=False only moves the centre (E = <theta|H|theta>)."""
        return self._step("htn_bond_update", lambda o, st: self.lib.htn_bond_update(
            self.handle, i, direction, 0 if placement == "right" else 1, 1 if optimise else 0, o, st), record, cutoff).energy

    def sweep(self):
        """one sweep in MPSKit's DMRG2 order (bonds 0..L-2 rightwards, L-3..0 leftwards), one library call"""
        self._sweep("htn_dmrg2_sweep", 2 * self.L - 3, lambda o, st, E: self.lib.htn_dmrg2_sweep(self.handle, o, st, E), ("energy",))
        return self.energy

    # ---- one-site DMRG at fixed bond tables (htn_site_update / htn_dmrg1_sweep) --------------------
    def centre(self) -> int:
        """the site that carries the centre (0 after construction and after every sweep)"""
        return int(self.lib.htn_mps_centre(self.handle))

    def update_site(self, i, direction, optimise=True, record=True):
        """one-site update of site i (the centre must be there): lowest eigenpair of the one-site effective Hamiltonian
        (optimise=False: <x|H_eff|x> only), then direction +1: QR, site i becomes a left isometry, the centre moves to
        i + 1; -1: LQ, the centre moves to i - 1; 0: it stays.  Bond tables never change.  Returns the eigenvalue, which
        is <psi|H|psi> of the stored state (nothing is truncated)."""
        return self._step("htn_site_update", lambda o, st: self.lib.htn_site_update(
            self.handle, i, direction, 1 if optimise else 0, o, st), record).energy

    def sweep1(self):
        """one one-site sweep at the current bond tables (sites 0..L-2 rightwards, L-1..1 leftwards, 2L-2 updates, one
        library call); the centre ends on site 0.  Grow the bonds with sweep() first.  The Schmidt spectra
        (`spectrum`) keep the values of the last two-site update of each bond."""
        self._sweep("htn_dmrg1_sweep", 2 * self.L - 2, lambda o, st, E: self.lib.htn_dmrg1_sweep(self.handle, o, st, E), ("energy",))
        return self.energy

    # ---- time evolution: two-site TDVP (htn_bond_evolve / htn_site_evolve / htn_tdvp2_sweep / htn_mps_set_mpo) ----
    def evolve_bond(self, i, direction, placement, dt, record=True):
        """theta <- exp(-i dt H_eff) theta on sites (i, i+1), then SVD, truncation, write-back and environment move as
        update_bond; dt complex (-i beta: imaginary time).  -> BondStats (energy = <theta|H_eff|theta> before the step,
        residual = the error estimate of the exponential)"""
        dt = complex(dt)
        return self._step("htn_bond_evolve", lambda o, st: self.lib.htn_bond_evolve(
            self.handle, i, direction, 0 if placement == "right" else 1, dt.real, dt.imag, o, st), record)

    def evolve_site(self, i, dt, record=True):
        """centre on site i <- exp(-i dt H_eff1) centre in place (no gauge move); -> BondStats.  No bond table changes (the
        cache of bond_of_site stays) and the record's energy does not become self.energy."""
        dt = complex(dt)
        return self._step("htn_site_evolve", lambda o, st: self.lib.htn_site_evolve(self.handle, i, dt.real, dt.imag, o, st), record,
                          drop_cache=False, sets_energy=False)

    def tdvp_sweep(self, dt):
        """one symmetric two-site TDVP step of length dt (complex; -i beta: imaginary time), one library call: half steps on
        the bonds rightwards and leftwards with backward one-site steps between them (2L-2 bond records).  The centre starts and
        ends on site 0, the state stays normalised; `log_norm` holds the logarithm of the norm change the exponentials produced
        (0 for real dt), `trunc_weights` the discarded weight per record.  lanczos_tol is the tolerance of the exponential.
        Returns <psi|H|psi> as the last bond step saw it."""
        dt = complex(dt)
        self._sweep("htn_tdvp2_sweep", 2 * self.L - 2, lambda o, st, E, lg: self.lib.htn_tdvp2_sweep(
            self.handle, dt.real, dt.imag, o, st, E, lg), ("energy", "log_norm"))
        return self.energy

    # ---- time evolution at fixed bond tables: one-site TDVP (htn_site_evolve_move / htn_tdvp1_sweep / htn_heff0_apply) ----
    def evolve_site_move(self, i, direction, dt_fwd, dt_back, record=True):
        """one move of one-site TDVP (the centre must be on site i): site <- exp(-i dt_fwd H_eff1) site, QR (direction +1) or
        LQ (-1) as update_site, the triangular factor C <- exp(-i dt_back H_eff0) C on the bond crossed, C into the neighbour,
        which becomes the centre.  Bond tables never change.  -> BondStats (energy = <psi|H|psi> before the move)"""
        f, b = complex(dt_fwd), complex(dt_back)
        return self._step("htn_site_evolve_move", lambda o, st: self.lib.htn_site_evolve_move(
            self.handle, i, direction, f.real, f.imag, b.real, b.imag, o, st), record)

    def tdvp1_sweep(self, dt):
        """one symmetric one-site TDVP step of length dt (complex; -i beta: imaginary time) at the current bond tables, one
        library call: evolve_site_move(i, +1, dt/2, -dt/2) rightwards, the last site by dt, the mirror image leftwards, site 0
        by dt/2 (2L-2 records, trunc_weight 0: nothing is truncated).  The centre starts and ends on site 0, the state stays
        normalised and `log_norm` holds the logarithm of the norm change (0 for real dt).  Grow the bonds with sweep() or
        tdvp_sweep() first; the Schmidt spectra (`spectrum`) keep the values of the last two-site update of each bond.
        Returns <psi|H|psi> as the closing step on site 0 saw it."""
        dt = complex(dt)
        self._sweep("htn_tdvp1_sweep", 2 * self.L - 2, lambda o, st, E, lg: self.lib.htn_tdvp1_sweep(
            self.handle, dt.real, dt.imag, o, st, E, lg), ("energy", "log_norm"))
        return self.energy

    # ---- correction-vector sweeps (htn_bond_solve / htn_cv_sweep) ------------------------------------------------
    @property
    def amplitude(self) -> float:
        """the factor beside the (normalised) stored tensors: 1 for every state but the result of apply_op (the applied norm)
        and a correction vector (|theta_new| of its last solve); `overlap` and `transition` apply it inside the library"""
        a = self.__dict__.get("_amplitude")
        if a is None:
            n2 = self.__dict__.get("applied_norm2")
            a = 1.0 if n2 is None else float(np.sqrt(max(n2, 0.0)))
        return a

    def solve_bond(self, i, direction, placement, z, record=True):
        """theta <- (z - H_eff)^-1 p on sites (i, i+1), p the projection of the ONE attached state (set_orthogonal([b])) times its
        amplitude, started from the current theta; then SVD, truncation, write-back and environment move as update_bond.
        lanczos_tol is the tolerance of the solve.  -> (BondStats with energy = Im <p|theta_new> and residual = the relative
        residual of the solve, <p|theta_new> = <b|x> before truncation, amplitude)"""
        z = complex(z)
        amp, bx = C.c_double(0.0), (C.c_double * 2)()
        s = self._step("htn_bond_solve", lambda o, st: self.lib.htn_bond_solve(
            self.handle, i, direction, 0 if placement == "right" else 1, z.real, z.imag, o, st, C.byref(amp), bx), record,
            sets_energy=False)              # (the record's energy is Im <p|theta_new>, no energy of the state)
        self._amplitude = amp.value
        return s, complex(bx[0], bx[1]), amp.value

    def cv_sweep(self, z):
        """one correction-vector sweep for (z - H) x = b, one library call: bonds 0..L-2 rightwards, L-2..0 leftwards (2L-2
        records); the centre starts and ends on site 0.  -> (<b|x> of the last bond before its truncation, amplitude): the state
        is amplitude x (the normalised stored tensors)."""
        z, bx = complex(z), (C.c_double * 2)()
        self._sweep("htn_cv_sweep", 2 * self.L - 2, lambda o, st, amp: self.lib.htn_cv_sweep(
            self.handle, z.real, z.imag, o, st, amp, bx), ("_amplitude",))       # (energy stays: a solve has none)
        return complex(bx[0], bx[1]), self._amplitude

    def bond_size(self, b) -> int:
        """elements of a vector in bond layout on bond b: one n_c x n_c column-major matrix per sector, in the order of
        `bonds[b]` (the layout of the triangular factors of a gauge move)"""
        n = int(self.lib.htn_mps_bond_size(self.handle, b))
        if n < 0:
            raise ValueError(f"bond_size: bond {b} out of range")
        return n

    def apply_heff0(self, b, x):
        """y = H_eff0(bond b) x on host vectors in bond layout (bond_size(b)); the centre must be on site b - 1 or b with both
        environments of the bond present, as after a gauge move across it"""
        return self._apply_host("htn_heff0_apply", self.lib.htn_heff0_apply, lambda: self.bond_size(b), b, x)

    def set_mpo(self, mpo):
        """swap the Hamiltonian under the state (a quench): same symmetry, chain length and site multiplets, centre on site
        0.  The environments are rebuilt on the device; the tensors are not touched."""
        cm = mpo if isinstance(mpo, CMpo) else CMpo(self.ops, mpo)
        self._check(self.lib.htn_mps_set_mpo(self.handle, cm.handle), "htn_mps_set_mpo")
        self.cmpo, self.mpo = cm, cm.sites
        self.energy = None

    def copy(self):
        """a second, independent engine holding the same state (bonds() + download_site through the constructor).  Call with
        the centre on site 0 (after construction or a sweep)."""
        if self.centre() != 0:
            raise ValueError("DMRG2.copy: the centre must be on site 0")
        tensors = [self.download_site(i) for i in range(self.L)]
        bonds = [dict(b.dims) for b in self.bonds]
        return DMRG2(self.ops, self.cmpo, bonds, tensors, self.chi_full, self.cutoff, self.krylovdim, self.lanczos_tol,
                     self.maxrestart, self.weighting, self.jacobi_tol, self.jacobi_max_sweeps)

    def apply_heff1(self, i, x):
        """y = H_eff(site i) x on host vectors in the stored layout of site i (the flat vector of `download_site`'s
        blocks: htn_mps_get_site); the centre must be on site i"""
        return self._apply_host("htn_heff1_apply", self.lib.htn_heff1_apply, lambda: self.lib.htn_mps_site_theta_size(self.handle, i), i, x)

    def site_vector(self, i):
        """the stored data of site i as one flat vector (the Lanczos vector of a one-site update when i is the centre)"""
        n = self.lib.htn_mps_site_size(self.handle, i, None)
        flat = np.zeros(max(n, 1), dtype=np.complex128)
        if self.lib.htn_mps_get_site(self.handle, i, None, flat.ctypes.data) < 0:
            raise abi.HtnError(self.lib.htn_last_error().decode())
        return flat[:n]

    def site_probabilities(self):
        """-> P[L, n_site]: probability of every site multiplet on every site.  Call after sweep() (centre on site 0,
        sites >= 1 right-canonical).  The centre is carried through the chain without optimisation; with the centre on
        site i the probability of site multiplet s is the squared norm of the (., s, .) blocks (tilde normalisation).
        Leaves stats/energy alone."""
        L = self.L
        P = np.zeros((L, self.sym.n_site))

        def read(i):
            p = np.zeros(self.sym.n_site)
            for (l, s, r), blk in self.download_site(i).items():
                p[s] += float(np.sum(np.abs(blk) ** 2))
            P[i] = p / p.sum()
        read(0)
        for i in range(L - 1):          # moving the centre must not truncate by value: cutoff 0
            self.update_bond(i, +1, "right", optimise=False, record=False, cutoff=0.0)
            read(i + 1)
        for i in range(L - 2, -1, -1):  # back to the post-sweep convention
            self.update_bond(i, -1, "left", optimise=False, record=False, cutoff=0.0)
        return P

    def site_occupations(self):
        """-> (n, d): <n_i> and the double occupancy <n_up n_dn>_i of every site (density_state, src:1495-1523)"""
        P = self.site_probabilities()
        Ns = np.array(self.sym.site_electrons, dtype=float)                     # electrons of every site multiplet
        return P @ Ns, P[:, -1].copy()                                            # (the last multiplet is the doubly occupied one)

    def spin_occupations(self):
        """-> (n_up, n_dn) per site; spinful U(1) x U(1) mode only (density_spin, src:1412-1456)"""
        if self.sym.su2:
            raise ValueError("This system is spin independent.")                # the reference's error text (src:1424)
        P = self.site_probabilities()
        return P[:, 1] + P[:, 3], P[:, 2] + P[:, 3]

    def bond_energies(self):
        """<psi| H |psi> of the state AS STORED (truncated), evaluated by a non-optimising pass: returns (E_total,
        per-bond running values).  Call after sweep() (centre on site 0).  The expectation value is the same number at
        every bond (the centre move is exact when nothing is truncated: cutoff 0, and the dimension limit is not
        reached by a state that already obeys it); the list documents that."""
        vals = []
        for i in range(self.L - 1):
            vals.append(self.update_bond(i, +1, "right" if i < self.L - 2 else "left", optimise=False, record=False,
                                         cutoff=0.0))
        for i in range(self.L - 3, -1, -1):
            vals.append(self.update_bond(i, -1, "left", optimise=False, record=False, cutoff=0.0))
        return vals[-1], vals

    def svd_cut(self, chi_full):
        """truncate every bond to truncdim(chi_full) by SVD alone (MPSKit `changebonds(psi, SvdCut(trscheme))`,
        used at src:1363-1365): one pass of centre moves without optimisation at the new limit, then a second,
        non-truncating pass that evaluates <psi|H|psi> of the TRUNCATED state, which is returned.  Call after sweep()."""
        self.chi_full = int(chi_full)
        for i in range(self.L - 1):
            self.update_bond(i, +1, "right" if i < self.L - 2 else "left", optimise=False, record=False, cutoff=0.0)
        for i in range(self.L - 3, -1, -1):
            self.update_bond(i, -1, "left", optimise=False, record=False, cutoff=0.0)
        E, _ = self.bond_energies()
        self.energy = E
        return E

    # ---- two-point correlation functions (htn_mps_correlator) ----------------------------------------
    def _site_op(self, name) -> abi.SiteOp:
        k, dN, red = self.sym.site_ops[name] if isinstance(name, str) else name      # a name of the symmetry or (k, dN, red)
        op = abi.SiteOp()
        op.k, op.dN = int(k), int(dN)
        r = np.zeros((abi.MAX_SITE, abi.MAX_SITE))
        r[:red.shape[0], :red.shape[1]] = red
        op.red[:] = list(r.reshape(-1))
        return op

    def correlator_channel(self, op_open, op_pass, op_close, op_onsite=None):
        """one channel, by site-operator names of the symmetry: C[i, j] = <close_j pass.. open_i> for i < j (coefficient 1 of the
        Hamiltonian term with these operators), C[i, i] = <onsite_i> if given, zeros below the diagonal; already divided by
        <psi|psi>.  One pass on the device, the state is only read (any centre position).  -> (C, <psi|psi>)"""
        ch = abi.CorrChannel()
        ch.open, ch.pass_, ch.close = self._site_op(op_open), self._site_op(op_pass), self._site_op(op_close)
        if op_onsite is not None:
            ch.onsite, ch.has_onsite = self._site_op(op_onsite), 1
        out = np.zeros((self.L, self.L), dtype=np.complex128)
        nrm = C.c_double(0.0)
        self._check(self.lib.htn_mps_correlator(self.handle, C.byref(ch), out.ctypes.data, C.byref(nrm)), "htn_mps_correlator")
        return out, nrm.value

    def correlator(self, kind, connected=False):
        """Hermitian ndarray[L, L] of two-point functions of the state as stored: kind "hop": sum_s <c+_is c_js>, "nn": <n_i n_j>,
        "ss": <S_i . S_j>, "pair": <D+_i D_j> (D = c_dn c_up); in the spinful U(1) x U(1) mode also the single channels "hop_up",
        "hop_dn", "szsz", "s+-" (<S+_i S-_j>), "s-+".  Operators, Jordan-Wigner strings and factors are the symmetry's term
        channels (models.TERM_CHANNELS*), the tables the Hamiltonian builder uses; the diagonal holds the one-site products n, n^2,
        S^2 = 3/4 (n - 2 docc), docc.  Channels that come as a Hermitian-conjugate pair ("hop+" / "hop-") fill the upper / the
        lower triangle, otherwise the lower triangle is the conjugate of the upper.  connected=True ("nn", "szsz") subtracts
        <n_i><n_j> (<sz_i><sz_j>)."""
        from .models import CORR_ONSITE, CORR_ONSITE_U1
        chans = self.sym.channels
        onsite = (CORR_ONSITE if self.sym.su2 else CORR_ONSITE_U1).get(kind)
        if kind in ("hop", "nn", "ss", "pair") and kind in chans:
            use = [(c, c[5]) for c in chans[kind]]
        elif not self.sym.su2 and kind in ("hop_up", "hop_dn"):
            use = [(c, c[5]) for c in chans["hop"] if c[0].startswith(kind)]
        elif not self.sym.su2 and kind in ("szsz", "s+-", "s-+"):
            use = [(c, 1.0) for c in chans["ss"] if c[0] == kind]
        else:
            raise ValueError(f"correlator kind '{kind}' is not available in the {self.sym.name} mode")
        if connected and kind not in ("nn", "szsz"):
            raise ValueError("connected=True is defined for 'nn' and 'szsz'")
        names = {c[0] for c, _ in use}
        upper = np.zeros((self.L, self.L), dtype=np.complex128)
        lower = None
        diag = None
        for (name, _q, op_open, op_pass, op_close, _f), fac in use:
            partner = name.endswith("-") and name[:-1] + "+" in names       # the h.c. of an upper channel: <.._j .._i>, j > i
            first = diag is None and not partner
            M, _ = self.correlator_channel(op_open, op_pass, op_close, onsite if first else None)
            if first:
                diag = np.diag(M).copy()
                M = M - np.diag(diag)
            if partner:
                lower = fac * M if lower is None else lower + fac * M
            else:
                upper += fac * M
        Cm = upper + (upper.conj().T if lower is None else lower.T) + np.diag(diag)
        if connected:
            one = "n" if kind == "nn" else "sz"
            m = np.real(np.diag(self.correlator_channel(one, "id", one, one)[0]))
            Cm = Cm - np.outer(m, m)
        return Cm

    # ---- correlation functions of nearest-neighbour bond operators (htn_mps_correlator2) -------------------
    def correlator2_channel(self, ops_open, op_pass, ops_close, open_level):
        """one channel of two bond operators: C[i, j] = <close1_{j+1} close0_j pass.. open1_{i+1} open0_i> for j >= i + 2, what an
        MPO path with these entries, coefficient 1 and the level open_level = (dN, k) after the open pair measures; zeros
        elsewhere; already divided by <psi|psi>.  ops_open: two site operators (names of the symmetry or (k, dN, red) tuples),
        ops_close: two, or one for the one-site close (products on three adjacent sites at j = i + 2).  One pass on the device, the
        state is only read (any centre position).  -> (C, <psi|psi>)"""
        if len(ops_open) != 2 or len(ops_close) not in (1, 2):
            raise ValueError("correlator2_channel: two open operators and one or two close operators")
        ch = abi.CorrChannel2()
        for n, o in enumerate(ops_open):
            ch.open[n] = self._site_op(o)
        for n, o in enumerate(ops_close):
            ch.close[n] = self._site_op(o)
        ch.pass_ = self._site_op(op_pass)
        ch.open_dN, ch.open_k, ch.n_close = int(open_level[0]), int(open_level[1]), len(ops_close)
        out = np.zeros((self.L, self.L), dtype=np.complex128)
        nrm = C.c_double(0.0)
        self._check(self.lib.htn_mps_correlator2(self.handle, C.byref(ch), out.ctypes.data, C.byref(nrm)), "htn_mps_correlator2")
        return out, nrm.value

    def _string_values(self, strings, sites):
        """sum over operator strings [(coef, [site operators], [(dN, k) of the level after each operator but the last])] on
        `sites` = 2 or 3 adjacent sites, or on two disjoint bonds (4): ndarray[L, L], entry [i, j] with i the first site and j
        the first site of the second bond (2: j = i + 1, 3: j = i + 2, 4: all j >= i + 2); one device pass per string"""
        out = np.zeros((self.L, self.L), dtype=np.complex128)
        for coef, ops, labels in strings:
            assert len(ops) == sites
            if sites == 2:
                M, _ = self.correlator_channel(ops[0], "id", ops[1])
                out += coef * np.diag(np.diag(M, 1), 1)
            else:
                M, _ = self.correlator2_channel(ops[:2], "F" if labels[1][0] % 2 else "id", ops[2:], labels[1])
                out += coef * (np.diag(np.diag(M, 2), 2) if sites == 3 else M)
        return out

    def bond_correlator(self, kind, connected=False):
        """Hermitian ndarray[L-1, L-1] of correlation functions of nearest-neighbour bond operators, indexed by each bond's left
        site: kind "bond": <B_i B_j>, B_i = sum_s (c+_{i s} c_{i+1 s} + h.c.) (bond order); "dimer": <(S_i . S_{i+1})
        (S_j . S_{j+1})>; "spair": <Delta+_i Delta_j>, Delta_i = (c_{i up} c_{i+1 dn} - c_{i dn} c_{i+1 up}) / sqrt 2 (singlet bond
        pair; needs a particle number, so not in the no-U(1) mode); in the spinful U(1) x U(1) mode also the single components
        "bond_up", "bond_dn" (one spin species), "dimer_zz" (Sz Sz bonds) and "dimer_xy" ((S+ S- + S- S+) / 2 bonds).  Disjoint
        bonds (j >= i + 2) take one htn_mps_correlator2 pass per operator string; bonds that share a site are products on
        three (j = i + 1) or two (j = i) sites, strings of their own (bondcorr.py).  connected=True ("bond", "dimer" and the
        components) subtracts <O_i><O_j>."""
        from . import bondcorr
        tab = bondcorr.strings(self.sym, kind)                    # raises ValueError for a kind the mode does not define
        if connected and kind == "spair":
            raise ValueError("connected=True is defined for 'bond' and 'dimer' (<Delta_i> = 0 in a state of fixed particle number)")
        if self.L < 2:
            raise ValueError("bond_correlator: the chain has no bond")
        upper = np.diag(np.diag(self._string_values(tab[0], 2), 1))                  # sites [i, i + 1] -> bond entry (i, i)
        if self.L >= 3:
            upper += np.diag(np.diag(self._string_values(tab[1], 3), 2), 1)          # [i, i + 2] -> (i, i + 1)
        if self.L >= 4:
            upper += self._string_values(tab[2], 4)[:-1, :-1]
        d = np.diag(np.diag(upper))
        Cm = upper - d + (upper - d).conj().T + d.real
        if connected:
            m = self.bond_expectation(kind)
            Cm = Cm - np.outer(m, m)
        return Cm

    def bond_expectation(self, kind):
        """ndarray[L-1]: <O_i> of the Hermitian bond operators of bond_correlator ("bond", "dimer" and their components)"""
        from . import bondcorr
        return np.real(np.diag(self._string_values(bondcorr.one_bond(self.sym, kind), 2), 1)).copy()

    # ---- local operators applied to the state (htn_mps_apply_op / htn_mps_transition) ------------------
    OP_ALIASES = {"c+": "cdag", "c+_up": "cdag_up", "c+_dn": "cdag_dn"}

    def _op_arg(self, op) -> abi.SiteOp:
        """a site operator by name (a key of the symmetry's site_ops; "c+" stands for "cdag") or as an abi.SiteOp"""
        if isinstance(op, abi.SiteOp):
            return op
        name = op if op in self.sym.site_ops else self.OP_ALIASES.get(op, op)
        if name not in self.sym.site_ops:
            raise ValueError(f"site operator '{op}' is not defined in the {self.sym.name} mode")
        return self._site_op(name)

    def move_centre(self, site):
        """carry the centre to `site` by non-optimising, non-truncating two-site updates"""
        if not 0 <= site < self.L:
            raise ValueError(f"site {site} out of range (the chain has {self.L} sites)")
        while self.centre() < site:
            self.update_bond(self.centre(), +1, "right", optimise=False, record=False, cutoff=0.0)
        while self.centre() > site:
            self.update_bond(self.centre() - 1, -1, "left", optimise=False, record=False, cutoff=0.0)

    def apply_op(self, site, op):
        """a NEW engine holding O_site |self> (same context, MPO and solver settings; not normalised: `applied_norm2` of the result
        is <O psi|O psi> = sum over the operator's components of <psi|O+_q O_q|psi>).  The centre must be on `site` and stays
        there in the result; self is only read.  op: a site-operator name of the symmetry ("c", "cdag" = "c+", "n", "S", spinful
        mode "c_up", "cdag_up", ...) or an abi.SiteOp.  SU(2) kinds: self has total spin 0 or the operator rank 0.
        Every update normalises the tensors it writes: after its first update the result keeps its norm in a factor inside the
        library, which `overlap` and `transition` apply; `copy()` goes through the tensors alone and gives the normalised state."""
        o = self._op_arg(op)
        h, n2 = C.c_void_p(), C.c_double(0.0)
        self._check(self.lib.htn_mps_apply_op(self.handle, int(site), C.byref(o), C.byref(h), C.byref(n2)), "htn_mps_apply_op")
        new = DMRG2.wrap(self.ops, self.cmpo, h, self.chi_full, self.cutoff, self.krylovdim, self.lanczos_tol, self.maxrestart,
                         self.weighting, self.jacobi_tol, self.jacobi_max_sweeps)
        new.applied_norm2 = n2.value
        return new

    def transition(self, op, ket) -> np.ndarray:
        """ndarray[L]: <O_x self|ket> for every site x in one pass on the device (self in any gauge, not modified); ket lives in
        the total sector of self fused with the operator's charge, e.g. an applied state after some time steps"""
        o = self._op_arg(op)
        out = np.zeros(self.L, dtype=np.complex128)
        self._check(self.lib.htn_mps_transition(self.handle, C.byref(o), ket.handle, out.ctypes.data), "htn_mps_transition")
        return out

    # ---- two-site energy variance (htn_mps_variance) ----------------------------------------------------
    def variance(self, timed=False):
        """two-site energy variance of the state as stored (Hubig, Haegeman, Schollwoeck, PRB 97, 045125): -> Variance with
        .total = sum(.site) + sum(.bond), .site[L] (one-site residuals), .bond[L - 1] (two-site residuals), .energy = <psi|H|psi>.
        Exact (<H^2> - <H>^2) for an MPO of range 1, a lower bound for longer range.  One library call; the centre may be
        anywhere and is back where it was afterwards, the state is the same state (to rounding), `energy` and `stats` are left
        alone.  An applied state reports the variance of the normalised state.  timed=True also fills .split = seconds spent in
        (theta + applies, projections, moves), each closed by a stream sync."""
        self._drop_bond_cache()
        site, bond = np.zeros(self.L), np.zeros(max(self.L - 1, 1))
        E, split = C.c_double(0.0), np.zeros(3)
        self._check(self.lib.htn_mps_variance(self.handle, site.ctypes.data, bond.ctypes.data, C.byref(E),
                                              split.ctypes.data if timed else None), "htn_mps_variance")
        bond = bond[:self.L - 1]
        return Variance(float(site.sum() + bond.sum()), site, bond, E.value, tuple(split) if timed else None)

    # ---- perfect sampling of site multiplets (htn_mps_sample) ----------------------------------------------
    def sample(self, u, measure=None, batch=None, timed=False):
        """independent configurations of site multiplets drawn from |psi|^2, each with its exact probability (Ferris, Vidal, PRB 85,
        165146): u[n, L] uniforms in [0, 1) -> (occ int32[n, L], logp[n]).  occ holds indices into the symmetry's site multiplets
        ({0, 1, 2} = empty, singly, doubly occupied in the SU(2) kinds, {0, up, dn, updn} in the spinful kind), logp the logarithm
        of the probability of each drawn configuration.  measure: L flags; a site with flag 0 is traced (nothing drawn, -1 in occ).
        batch: samples that advance through a site together (None: the library's default); results do not depend on it.  The
        centre must be on site 0 (as after a sweep); the state is only read.  timed=True: also (plan, device) seconds."""
        u = np.ascontiguousarray(u, dtype=np.float64)
        if u.ndim != 2 or u.shape[1] != self.L:
            raise ValueError(f"sample: u must have shape (n, {self.L})")
        if u.size and not (u.min() >= 0.0 and u.max() < 1.0):
            raise ValueError("sample: the uniforms must lie in [0, 1)")
        n = u.shape[0]
        m = None
        if measure is not None:
            m = np.ascontiguousarray(np.asarray(measure) != 0, dtype=np.int32)
            if m.shape != (self.L,):
                raise ValueError(f"sample: measure must have {self.L} flags")
        occ, logp, split = np.zeros((n, self.L), dtype=np.int32), np.zeros(n), np.zeros(2)
        self._check(self.lib.htn_mps_sample(self.handle, n, u.ctypes.data, None if m is None else m.ctypes.data,
                                            0 if batch is None else int(batch), occ.ctypes.data, logp.ctypes.data,
                                            split.ctypes.data if timed else None), "htn_mps_sample")
        return (occ, logp, tuple(split)) if timed else (occ, logp)

    def site_energies(self):
        """genuine <psi|H|psi> of the state as stored, split per site: e_i = energy of all Hamiltonian terms that END
        on site i (on-site terms of i, and every two-site term whose right-most site is i); sum(e) = <psi|H|psi>.
        Evaluated by one non-optimising rightward pass: with the centre in Schmidt form on bond b, the completed-term
        level of the left environment gives E(sites < b) = sum_c sum_k s~_{c,k}^2 GL_final[c][k, k]; the last site closes
        with the total <theta|H|theta>.  Call after sweep() (centre on site 0); the state is left as found."""
        L = self.L
        run = np.zeros(L)                                   # run[i] = energy of the terms inside sites 0..i
        E_tot = None
        nfin = len(self.mpo[0].right) - 1
        for i in range(L - 1):
            E_tot = self.update_bond(i, +1, "right", optimise=False, record=False, cutoff=0.0)
            spec = self.spectrum(i + 1)
            env = self.download_env("L", i + 1)
            wfin = len(self.mpo[i].right) - 1               # 'term complete' level of the MPO bond right of site i
            acc = 0.0
            for (bra, w, ket), M in env.items():
                if w == wfin and bra == ket and bra in spec:
                    s2 = self.sym.qdim(bra) * np.asarray(spec[bra]) ** 2
                    acc += float(np.real(np.sum(np.diag(M)[:len(s2)] * s2)))
            run[i] = acc
        run[L - 1] = E_tot
        for i in range(L - 2, -1, -1):                      # back to the post-sweep convention (centre on site 0)
            self.update_bond(i, -1, "left", optimise=False, record=False, cutoff=0.0)
        e = np.diff(np.concatenate([[0.0], run]))
        return e
