"""Shared by test_dmrg1_cpu.py / test_dmrg1_gpu.py: small chains for the one-site sweep, on either library."""
import numpy as np

import excited_common as xc
from hubbardtn_amd import engine, models, mps
from oracle import ed

SYMS = ["SU2U1", "U1U1", "SU2P"]


def _lowest(L, nu, nd):
    from scipy.sparse.linalg import eigsh
    Hs = ed.SectorED(L, nu, nd, [1.0], [4.0]).hamiltonian()
    if Hs.shape[0] < 64:
        return np.linalg.eigvalsh(Hs.toarray())[0]
    return eigsh(Hs.astype(np.float64) if np.isrealobj(Hs.data) else Hs, k=1, which="SA", tol=0, ncv=40)[0][0]


def ed_energy(symname, L=8):
    """ground-state energy of the L = 8 chain of xc.model in the sector the DMRG run targets (sparse Lanczos on the ED matrix)"""
    if symname == "SU2P":          # grand-canonical H - mu N, mu = 2 = U / 2: the minimum sits within two particles of half filling
        return min(_lowest(L, (N + 1) // 2, N // 2) - 2.0 * N for N in range(L - 2, L + 3))
    return _lowest(L, L // 2, L // 2)


def loose_state(ops, symname, L=8, seed=3, H=None, target=None):
    """an engine after ONE loose two-site sweep (krylovdim 4, tolerance 1e-3) from a random start, untruncated"""
    sym, H0, tgt = xc.model(symname, L)
    H = H0 if H is None else H
    b, t = mps.random_mps(L, tgt if target is None else target, 6, seed=seed, sym=sym)
    e = engine.DMRG2(ops, H, b, t, lanczos_tol=1e-3, krylovdim=4)
    e.sweep()
    e.lanczos_tol, e.krylovdim = 1e-12, 20
    return e


def tables(e):
    return [dict(x.dims) for x in e.bonds]


def converge_onesite(e, max_sweeps=12):
    """sweep1 until the energy moves by less than 1e-12; every Ritz value of every site update is recorded"""
    ritz, E_prev = [], None
    for _ in range(max_sweeps):
        n0 = len(e.stats)
        E = e.sweep1()
        ritz.extend(s.energy for s in e.stats[n0:])
        if E_prev is not None and abs(E - E_prev) < 1e-12:
            break
        E_prev = E
    return E, ritz


def isometry_defects(e):
    """max |A^H A - 1| over the left tensors and |B B^H - 1| over the right tensors of the state as stored"""
    worst = 0.0
    c = e.centre()
    for i in range(e.L):
        if i == c:
            continue
        blocks = e.download_site(i)
        groups = {}
        for (l, s, r), blk in blocks.items():
            groups.setdefault(r if i < c else l, []).append(((l, s, r), blk))
        for key, items in groups.items():
            items.sort(key=lambda kv: kv[0])
            M = np.concatenate([b for _, b in items], axis=0 if i < c else 1)
            G = M.conj().T @ M if i < c else M @ M.conj().T
            worst = max(worst, np.abs(G - np.eye(G.shape[0])).max())
    return worst
