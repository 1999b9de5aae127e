"""TEST STATEMENT of the sweep driver in Python (the product's driver is C++: hubbardtn_amd/csrc/htn_engine.cpp, htn_site.cpp),
executed by the CPU suite on the numpy emulator of the kernel-level ABI (tests/emul.py).

Two-site DMRG sweep engine (finite chain) on the device primitives of hubbardtn_hip.h.

Stands in for MPSKit's two-site sweep body reached from
`find_groundstate(psi0, H, IDMRG2(; trscheme, tol))` (src/HubbardFunctions.jl:1010) -- per bond:
form theta, Lanczos lowest eigenpair of the AC2 effective Hamiltonian, SVD + truncation, write
back, move the environment.  The sweep schedule follows MPSKit's DMRG2:
bonds 1..L-1 going right, then L-2..1 going left (2L-3 bond updates per sweep).

All tensors stay on the device between bonds; the host sees only the Lanczos tridiagonal
coefficients and the singular values (needed for the global truncation rule, App. A.6).
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np

import ref_planner as pl
from ref_planner import (BUF_AUX, BUF_L, BUF_R, BUF_S1, BUF_S2, BUF_X, BUF_Y, BUF_Z, Bond, EnvLayout, SiteLayout,
                      ThetaLayout)


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


class DMRG2:
    """finite two-site DMRG on reduced SU(2) x U(1) tensors.

    ops        : device primitive provider (hubbardtn_amd.device.HipOps in the product)
    mpo        : list[models.MPOSite]
    bonds      : list of {sector: count} for bonds 0..L (initial state)
    tensors    : list of {(l, s, r): ndarray[n_l, n_r]} right-canonical initial site tensors
    chi_full   : truncdim(D) in TensorKit's `dim` units (sum (2S+1) n), or None
    cutoff     : truncbelow(eta) Schmidt-value cut (10^-svalue, src:1007), or 0
    shard      : optional (rank, world, allreduce_fn) for the sector-parallel apply
    """

    def __init__(self, ops, mpo, bonds, tensors, chi_full=None, cutoff=0.0, krylovdim=30, lanczos_tol=1e-12,
                 maxrestart=3, weighting="sqrtdim", jacobi_tol=1e-14, jacobi_max_sweeps=40, shard=None,
                 left_env=None, right_env=None):
        self.ops, self.mpo = ops, mpo
        self.L = len(mpo)
        self.chi_full, self.cutoff, self.weighting = chi_full, cutoff, weighting
        self.krylovdim, self.lanczos_tol, self.maxrestart = krylovdim, lanczos_tol, maxrestart
        self.jacobi_tol, self.jacobi_max_sweeps = jacobi_tol, jacobi_max_sweeps
        self.shard = shard
        self.profile = False
        # Optional rank-revealing cut of the blocks' pivoted QR (htn_jacobi_set_rank_cut): singular directions below
        # rank_cut x (the smallest value the last update of the same bond kept, or the truncbelow cut) are dropped
        # before the Jacobi sweeps.  Kept singular values then move by at most cut^2 / (2 sigma), i.e. up to
        # rank_cut^2 / 2 RELATIVE for the smallest kept one.  OFF by default: the north-star parity is 1e-8 relative
        # on every kept Schmidt value.  Measured at chi = 1024 (energy unchanged to 3e-15 in all cases):
        #   rank_cut 1e-3: sweep -4 %, smallest kept values to <= 5e-7 relative;  0.05: sweep -16 %, <= 1.3e-3.
        self.rank_cut = 0.0
        self._cut_hint = {}
        self.bonds = [Bond(b) for b in bonds]
        self._plan_cache = {}
        self.cache_hits = self.cache_misses = 0
        self.site_lay = [None] * self.L
        self.site_buf = [None] * self.L
        for i in range(self.L):
            self._upload_site(i, tensors[i], "R")
        self.Llay = [None] * (self.L + 1)
        self.Lbuf = [None] * (self.L + 1)
        self.Rlay = [None] * (self.L + 1)
        self.Rbuf = [None] * (self.L + 1)
        # boundaries: an open end (no environment blocks: only the implicit identity level), or -- for a window
        # inside a larger system (idmrg.py) -- the (EnvLayout, device buffer) of the block beyond that end
        if left_env is None:
            self.Llay[0] = EnvLayout.build("L", self.bonds[0], mpo[0].left)
            self.Lbuf[0] = ops.zeros_z(max(self.Llay[0].size, 1))
        else:
            self.Llay[0], self.Lbuf[0] = left_env
            assert self.Llay[0].bond == self.bonds[0] and self.Llay[0].levels == list(mpo[0].left)
        if right_env is None:
            self.Rlay[self.L] = EnvLayout.build("R", self.bonds[self.L], mpo[self.L - 1].right)
            self.Rbuf[self.L] = ops.zeros_z(max(self.Rlay[self.L].size, 1))
        else:
            self.Rlay[self.L], self.Rbuf[self.L] = right_env
            assert self.Rlay[self.L].bond == self.bonds[self.L] and self.Rlay[self.L].levels == list(mpo[self.L - 1].right)
        for i in range(self.L - 1, 0, -1):
            self._right_env(i)
        self.energy = None
        self.stats = []
        self.spectra = {}

    # ---- plan cache --------------------------------------------------------------------------------
    # Task lists depend only on the sector tables of the bonds involved (and the MPO site), not on the
    # tensor data, and in converged sweeps the same tables recur bond after bond, sweep after sweep.
    # Like TensorKit's global fusion-tree-transformer caches, compiled plans (already uploaded) are
    # memoised by those tables.
    def _cached(self, key, builder):
        hit = self._plan_cache.get(key)
        if hit is None:
            if len(self._plan_cache) > 20000:
                self._plan_cache.clear()
            hit = builder()
            self._plan_cache[key] = hit
            self.cache_misses += 1
        else:
            self.cache_hits += 1
        return hit

    def _site_layout(self, kind, bl, br):
        return self._cached(("slay", kind, bl.key(), br.key()), lambda: SiteLayout.build(kind, bl, br))

    def _theta_layout(self, bl, br):
        return self._cached(("tl", bl.key(), br.key()), lambda: ThetaLayout.build(bl, br))

    # ---- host <-> device site tensors -----------------------------------------------------------
    def _upload_site(self, i, blocks, kind):
        lay = self._site_layout(kind, self.bonds[i], self.bonds[i + 1])
        flat = np.zeros(max(lay.size, 1), dtype=np.complex128)
        for key, (off, m, n, ld) in lay.blocks.items():
            blk = blocks.get(key)
            if blk is None:
                continue
            assert blk.shape == (m, n), (key, blk.shape, (m, n))
            # scatter column-major with leading dimension ld
            idx = off + np.arange(m)[:, None] + ld * np.arange(n)[None, :]
            flat[idx] = blk
        self.site_lay[i] = lay
        self.site_buf[i] = self.ops.to_device(flat)

    def download_site(self, i):
        lay = self.site_lay[i]
        flat = self.ops.to_host(self.site_buf[i])
        out = {}
        for key, (off, m, n, ld) in lay.blocks.items():
            idx = off + np.arange(m)[:, None] + ld * np.arange(n)[None, :]
            out[key] = flat[idx].copy()
        return out

    def download_env(self, side, i):
        lay = self.Llay[i] if side == "L" else self.Rlay[i]
        flat = self.ops.to_host(self.Lbuf[i] if side == "L" else self.Rbuf[i])
        return {key: flat[off:off + m * n].reshape(n, m).T.copy() for key, (off, m, n) in lay.blocks.items()}

    # ---- environments -----------------------------------------------------------------------------
    def _bufs(self, **kw):
        table = [None] * 8
        for k, v in kw.items():
            table[{"x": BUF_X, "y": BUF_Y, "l": BUF_L, "r": BUF_R, "z": BUF_Z, "s1": BUF_S1, "s2": BUF_S2,
                   "aux": BUF_AUX}[k]] = v
        return table

    def _left_env(self, i):
        """GL on bond i+1 from GL on bond i and the left-layout tensor of site i"""
        ops = self.ops
        lay = self.site_lay[i]
        assert lay.kind == "L"

        def build():
            Lnew = EnvLayout.build("L", self.bonds[i + 1], self.mpo[i].right)
            t1, t2, zsize = pl.plan_env_cached("L", self.Llay[i], lay, self.mpo[i], Lnew)
            return Lnew, ops.upload_tasks(t1), ops.upload_tasks(t2), zsize, t1.flops + t2.flops
        Lnew, d1, d2, zsize, flops = self._cached(("lenv", i, self.bonds[i].key(), self.bonds[i + 1].key()), build)
        z = ops.empty_z(max(zsize, 1))
        out = ops.empty_z(max(Lnew.size, 1))
        ops.grouped_gemm(self._bufs(l=self.Lbuf[i], s1=self.site_buf[i], z=z), d1)
        ops.grouped_gemm(self._bufs(s1=self.site_buf[i], z=z, y=out), d2)
        self.Llay[i + 1], self.Lbuf[i + 1] = Lnew, out
        return flops

    def _right_env(self, i):
        """GR on bond i from GR on bond i+1 and the right-layout tensor of site i"""
        ops = self.ops
        lay = self.site_lay[i]
        assert lay.kind == "R"

        def build():
            Rnew = EnvLayout.build("R", self.bonds[i], self.mpo[i].left)
            t1, t2, zsize = pl.plan_env_cached("R", self.Rlay[i + 1], lay, self.mpo[i], Rnew)
            return Rnew, ops.upload_tasks(t1), ops.upload_tasks(t2), zsize, t1.flops + t2.flops
        Rnew, d1, d2, zsize, flops = self._cached(("renv", i, self.bonds[i].key(), self.bonds[i + 1].key()), build)
        z = ops.empty_z(max(zsize, 1))
        out = ops.empty_z(max(Rnew.size, 1))
        ops.grouped_gemm(self._bufs(r=self.Rbuf[i + 1], s1=self.site_buf[i], z=z), d1)
        ops.grouped_gemm(self._bufs(s1=self.site_buf[i], z=z, y=out), d2)
        self.Rlay[i], self.Rbuf[i] = Rnew, out
        return flops

    # ---- effective Hamiltonian --------------------------------------------------------------------
    def _make_apply(self, i, tl):
        """stage list of the H_eff apply on bond (i, i+1): [(buffer table, device task list), ...]"""
        ops = self.ops

        def build():
            tz, ty, zsize, nterms = pl.plan_apply_cached(tl, self.Llay[i], self.Rlay[i + 2], self.mpo[i], self.mpo[i + 1])
            flops = ty.flops + (tz.flops if tz is not None else 0)
            ntiles = ty.ntiles + (tz.ntiles if tz else 0)
            nsegs = ty.nsegs + (tz.nsegs if tz else 0)
            if self.shard is not None:
                rank, world, _ = self.shard
                ty = _shard_tasks(ty, rank, world)
            return (ops.upload_tasks(tz) if tz is not None else None, ops.upload_tasks(ty), zsize, flops, ntiles, nsegs)
        dz, dy, zsize, flops, ntiles, nsegs = self._cached(
            ("apply", i, self.bonds[i].key(), self.bonds[i + 2].key()), build)
        z = ops.empty_z(max(zsize, 1))
        Lb, Rb = self.Lbuf[i], self.Rbuf[i + 2]
        stages = []
        if dz is not None:
            stages.append((self._bufs(l=Lb, z=z), dz))
        stages.append((self._bufs(l=Lb, r=Rb, z=z), dy))
        nbytes = 16 * (2 * tl.size + self.Llay[i].size + self.Rlay[i + 2].size)
        return stages, flops, nbytes, ntiles, nsegs

    # ---- one bond ---------------------------------------------------------------------------------
    def update_bond(self, i, direction, placement, optimise=True):
        """optimise sites (i, i+1); placement 'right': A_i = U, centre S V^H on i+1 (+ left env);
        'left': centre U S on i, B_{i+1} = V^H (+ right env).  optimise=False only moves the centre: the
        eigensolver stops after its first step (x = theta normalised, E = <theta|H|theta>)."""
        t0 = time.perf_counter()
        ops = self.ops
        bl, br = self.bonds[i], self.bonds[i + 2]
        tl = self._theta_layout(bl, br)
        n = tl.size
        kd = self.krylovdim
        lay1, lay2 = self.site_lay[i], self.site_lay[i + 1]
        mode = lay1.kind + lay2.kind
        assert mode in ("RR", "LL", "LR"), mode
        V = ops.empty_z((kd + 2) * n)
        # theta -> V[0] (the Lanczos driver normalises it)
        dth = self._cached(("theta", mode, bl.key(), self.bonds[i + 1].key(), br.key()),
                           lambda: ops.upload_tasks(pl.plan_theta(mode, lay1, lay2, tl)))
        ops.grouped_gemm(self._bufs(s1=self.site_buf[i], s2=self.site_buf[i + 1], y=V[0:n]), dth)
        stages, aflops, abytes, ntiles, nsegs = self._make_apply(i, tl)
        if self.profile:
            ops.sync()
        t_plan = time.perf_counter() - t0
        E, nmv, res = ops.lanczos(stages, BUF_X, BUF_Y, V, n, kd, self.lanczos_tol if optimise else 1e300, self.maxrestart,
                                  zero_y=self.shard is not None,
                                  exchange=self.shard[2] if self.shard is not None else None)
        if self.profile:
            ops.sync()
        t_lan = time.perf_counter() - t0 - t_plan
        x = V[0:n]
        # ---- SVD + truncation ----
        sp, d_stage, d_desc = self._cached(("svd", placement, bl.key(), br.key()),
                                           lambda: (lambda p_: (p_, ops.to_device(p_.stage), ops.to_device(p_.desc)))(
                                               pl.plan_svd(tl, placement)))
        nb = len(sp.mids)
        G = ops.empty_z(max(sp.g_size, 1))
        Vj = ops.empty_z(max(sp.v_size, 1))
        S = ops.empty_f64(max(sp.s_size, 1))
        info = ops.empty_i32(max(nb, 1))
        ops.batched_copy(G, x, None, None, d_stage, nb, 1.0)
        # Singular directions far below what the truncation keeps need not be resolved.  truncbelow(eta): everything
        # below eta goes anyway.  truncdim(D): if the previous update of this bond (same D) was limited by D, its
        # smallest kept value is where the cut will fall again.  x is normalised, so values compare across sweeps.
        cut = 0.0
        set_cut = getattr(ops, "jacobi_set_rank_cut", None)
        if set_cut is not None and self.rank_cut > 0.0:
            hint = self._cut_hint.get(i + 1)
            if hint is not None and hint[0] == (self.chi_full, self.cutoff):
                cut = self.rank_cut * hint[1]
            cut = max(cut, self.rank_cut * self.cutoff)
        if cut > 0.0:
            set_cut(cut)
        try:
            ops.jacobi_svd(G, Vj, S, d_desc, nb, sp.max_m, self.jacobi_max_sweeps, self.jacobi_tol, info,
                           desc_host=sp.desc)
        finally:
            if cut > 0.0:
                set_cut(0.0)
        s_host = ops.to_host(S)
        info_h = ops.to_host(info)
        if nb and int(info_h[:nb].min()) < 0:
            raise RuntimeError("Jacobi SVD did not converge")
        # per-block descending order and the global truncation on flat arrays (one lexsort instead of a Python loop
        # over the blocks; the sector numbering of sp.mids is the sorted label order truncate() uses)
        st_ = sp.__dict__.get("_flat")
        if st_ is None:
            offs = sp.desc["s_off"][:nb].astype(np.int64)
            lens = sp.desc["n"][:nb].astype(np.int64)
            assert list(sp.mids) == sorted(sp.mids) and np.array_equal(offs, np.cumsum(lens) - lens)
            sid = np.repeat(np.arange(nb), lens)
            st_ = sp.__dict__["_flat"] = (offs, lens, sid, np.arange(int(lens.sum())) - np.repeat(offs, lens),
                                          np.array([c[1] + 1 for c in sp.mids], dtype=np.int64)[sid])
        offs, lens, sid, pos, dims = st_
        sv = s_host[:len(sid)]
        perm = np.lexsort((pos, -sv, sid))                    # by block, value descending, original index ascending
        vals = sv[perm]
        counts, tw, nrm = pl.truncate_arrays(vals, sid, pos, dims, nb, self.chi_full, self.cutoff, self.weighting)
        local = perm - np.repeat(offs, lens)                  # column index inside its block
        svals = {c: vals[offs[k]:offs[k] + lens[k]] for k, c in enumerate(sp.mids)}
        order = {c: local[offs[k]:offs[k] + lens[k]] for k, c in enumerate(sp.mids)}
        keep = {c: int(counts[k]) for k, c in enumerate(sp.mids)}
        mid = Bond({c: k for c, k in keep.items() if k > 0})
        # hint for the next visit of this bond: the smallest kept value, valid only if the dimension limit (not the
        # number of available states) ended the kept set
        kept_tot = int(counts.sum())
        if self.chi_full is not None and tw > 0.0 and kept_tot > 0 and kept_tot < int((vals > 0.0).sum()):
            ends = offs + np.maximum(counts, 1) - 1
            self._cut_hint[i + 1] = ((self.chi_full, self.cutoff), float(vals[ends][counts > 0].min()))
        else:
            self._cut_hint.pop(i + 1, None)
        # the finalisation plan depends on the kept COUNTS only (not on which columns carry them): in converged sweeps
        # the same counts recur at the same bond, so layouts, copy items and the centre GEMM list (already on the
        # device) are memoised; only the column indices travel per update
        def build_fin():
            layA_ = self._site_layout("L", bl, mid)
            layB_ = self._site_layout("R", mid, br)
            ident = {c: np.arange(int(lens[k])) for k, c in enumerate(sp.mids)}        # placeholder order: idx only
            ig, cg, iv, _, cen = pl.plan_finalize(tl, sp, ident, keep, layA_, layB_, placement, 0, layA_.size)
            ig_d, cg_d, iv_d = ops.to_device_packed([ig, cg, iv])
            return (layA_, layB_, ig_d, len(ig), cg_d, len(cg), iv_d, len(iv),
                    ops.upload_tasks(cen) if cen is not None else None)
        layA, layB, iso_g_d, n_ig, cen_g_d, n_cg, iso_v_d, n_iv, cen_dev = self._cached(
            ("fin", placement, bl.key(), br.key(), counts.tobytes()), build_fin)
        offA, offB = 0, layA.size
        idx = np.concatenate([order[c][:keep[c]] for c in sp.mids if keep[c] > 0]).astype(np.int32) if kept_tot else \
            np.zeros(1, dtype=np.int32)
        out = ops.zeros_z(max(layA.size + layB.size, 1))
        idx_d = ops.to_device(idx)
        if n_ig:
            ops.batched_copy(out, G, idx_d, S, iso_g_d, n_ig, 1.0)
        if n_cg:
            ops.batched_copy(out, G, idx_d, S, cen_g_d, n_cg, 1.0 / nrm)
        if n_iv:
            ops.batched_copy(out, Vj, idx_d, S, iso_v_d, n_iv, 1.0)
        if cen_dev is not None:
            ops.scale_inplace(x, 1.0 / nrm)                      # centre = U^H (M / nrm)
            ops.grouped_gemm(self._bufs(x=x, s1=out, y=out), cen_dev)
        bufA, bufB = out[offA:offA + max(layA.size, 1)], out[offB:offB + max(layB.size, 1)]
        self.bonds[i + 1] = mid
        self.site_lay[i], self.site_buf[i] = layA, bufA
        self.site_lay[i + 1], self.site_buf[i + 1] = layB, bufB
        if self.profile:
            ops.sync()
        t_svd = time.perf_counter() - t0 - t_plan - t_lan
        if placement == "right":
            self._left_env(i)
        else:
            self._right_env(i + 1)
        if self.profile:
            ops.sync()
        t_env = time.perf_counter() - t0 - t_plan - t_lan - t_svd
        self.energy = E
        self.spectra[i + 1] = {c: svals[c][:keep[c]] / nrm / np.sqrt(c[1] + 1) for c in svals if keep[c] > 0}
        st = BondStats(bond=i + 1, direction=direction, energy=E, n_matvec=nmv, residual=res, trunc_weight=tw,
                       chi_full=mid.dim_full, multiplets=mid.multiplets, theta_size=n, apply_flops=aflops,
                       apply_bytes=abytes, svd_flops=sp.flops,
                       jacobi_sweeps=int(info_h[:nb].max()) if nb else 0, n_tiles=ntiles, n_segs=nsegs,
                       t_plan=t_plan, t_total=time.perf_counter() - t0, t_lanczos=t_lan, t_svd=t_svd,
                       t_env=t_env)
        self.stats.append(st)
        return E

    def sweep(self):
        """one sweep in MPSKit's DMRG2 order: bonds 0..L-2 rightwards, L-3..0 leftwards."""
        L = self.L
        for i in range(L - 1):
            self.update_bond(i, +1, "right" if i < L - 2 else "left")
        for i in range(L - 3, -1, -1):
            self.update_bond(i, -1, "left")
        return self.energy

    def site_occupations(self):
        """-> (n, d): <n_i> and the double occupancy <n_up n_dn>_i of every site (density_state, src:1495-1523).
        Call after sweep() (centre on site 0, sites >= 1 right-canonical).  The centre is carried through the chain
        without optimisation; with the centre on site i the probability of site multiplet s is the squared norm
        of the (., s, .) blocks (tilde normalisation), and n = P(single) + 2 P(double)."""
        L = self.L
        n, d = np.zeros(L), np.zeros(L)

        def read(i):
            p = np.zeros(3)
            for (l, s, r), blk in self.download_site(i).items():
                p[s] += float(np.sum(np.abs(blk) ** 2))
            p /= p.sum()
            n[i], d[i] = p[1] + 2.0 * p[2], p[2]
        saved = (self.chi_full, self.cutoff, self.stats, self.energy, dict(self.spectra))
        self.cutoff = 0.0                                       # moving the centre must not truncate by value
        read(0)
        for i in range(L - 1):
            self.update_bond(i, +1, "right", optimise=False)
            read(i + 1)
        for i in range(L - 2, -1, -1):                          # back to the post-sweep convention
            self.update_bond(i, -1, "left", optimise=False)
        self.chi_full, self.cutoff, self.stats, self.energy, self.spectra = saved
        return n, d

    def svd_cut(self, chi_full):
        """truncate every bond to truncdim(chi_full) by SVD alone (MPSKit `changebonds(psi, SvdCut(trscheme))`,
        used at src:1363-1365): one pass of centre moves without optimisation at the new limit.  Returns the
        energy <psi|H|psi> of the truncated state.  Call after sweep()."""
        saved = (self.cutoff, self.stats)
        self.chi_full, self.cutoff = int(chi_full), 0.0
        for i in range(self.L - 1):
            self.update_bond(i, +1, "right" if i < self.L - 2 else "left", optimise=False)
        for i in range(self.L - 3, -1, -1):
            self.update_bond(i, -1, "left", optimise=False)
        self.cutoff, self.stats = saved
        return self.energy

    def bond_dims(self):
        """`dim_state` analogue (src/HubbardFunctions.jl:1399-1405): TensorKit dim of each bond"""
        return [b.dim_full for b in self.bonds]


def _shard_tasks(tasks, rank, world):
    """owner-computes split of the output tiles over ranks: tiles are sorted by work (LPT order),
    dealing them round-robin balances MACs; every rank keeps the full segment table."""
    import copy
    t = copy.copy(tasks)
    sel = np.arange(tasks.ntiles)[rank::world]
    t.tiles = np.ascontiguousarray(tasks.tiles[sel]) if len(sel) else tasks.tiles[:1].copy()
    t.ntiles = len(sel)
    return t
