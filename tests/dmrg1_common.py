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


def gauge_block_shapes(e, i, direction):
    """[(m, n)] of the blocks the gauge move of update_site(i, direction) factorises (plan_gauge1 of htn_plan_env.cpp: one
    sector matrix per right sector of the centre, its (l, s) blocks stacked, for direction +1; per left sector, the (s, r)
    blocks side by side and m their total width, for -1) -- from the stored blocks of the centre, before the move"""
    assert e.centre() == i
    ext = {}
    for (l, s, r), blk in e.download_site(i).items():
        key, long_, short = (r, blk.shape[0], blk.shape[1]) if direction > 0 else (l, blk.shape[1], blk.shape[0])
        m, n = ext.get(key, (0, short))
        assert n == short
        ext[key] = (m + long_, n)
    return sorted(ext.values())


def tall_gauge_round_trip(ops):
    """the centre of tall_state's L = 14 state (bond tables capped at tall_state.CAP = 150 per sector) carried from site I0
    to the right end and back to site 0 by update_site(optimise=False): nothing but the QR / LQ gauge move, the
    environment steps and <x|H_eff|x> runs.  Asserts the left isometries at the turning point.
    -> (engine, the returned values, largest m of a factorised block)"""
    import qr_cases as qc
    import tall_state as ts
    e = ts.centred_engine(ops)
    vals, m_max = [], 0
    for i in range(ts.I0, ts.L - 1):
        m_max = max(m_max, max(m for m, _ in gauge_block_shapes(e, i, +1)))
        vals.append(e.update_site(i, +1, optimise=False, record=False))
    assert e.centre() == ts.L - 1
    for i in range(ts.I0, ts.L - 1):
        ts.assert_left_isometry(e, i)
    left_defect = isometry_defects(e)
    assert left_defect <= 1e-12
    for i in range(ts.L - 1, 0, -1):
        m_max = max(m_max, max(m for m, _ in gauge_block_shapes(e, i, -1)))
        vals.append(e.update_site(i, -1, optimise=False, record=False))
    assert e.centre() == 0
    print("tall gauge round trip: largest m", m_max, "panel width", qc.panel_width(m_max), "moves", len(vals),
          "E first", repr(vals[0]), "max |E - E first| / |E first|", max(abs(v - vals[0]) for v in vals) / abs(vals[0]),
          "isometry defects: all left", left_defect, "all right", isometry_defects(e))
    return e, vals, m_max


def assert_tall_gauge_round_trip(ops):
    """the assertions both libraries must meet; returns the moved engine"""
    import qr_cases as qc
    import tall_state as ts
    e, vals, m_max = tall_gauge_round_trip(ops)
    assert qc.panel_width(m_max) < qc.W, "the engine must reach a block too tall for the full panel width (m > 464)"
    assert max(abs(v - vals[0]) for v in vals) <= 1e-11 * abs(vals[0])
    assert isometry_defects(e) <= 1e-12
    twin = ts.centred_engine(ops)
    ov = e.overlap(twin)
    print("overlap with the untouched twin", ov, "| |ov| - 1 |", abs(abs(ov) - 1.0))
    assert abs(abs(ov) - 1.0) <= 1e-12
    return e


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
