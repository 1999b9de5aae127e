"""TEST INFRASTRUCTURE: a one-band chain whose centre bond has a coupled-sector block above 512 rows in both orientations
(the multi-CU streamed SVD path of htn_jacobi_svd_z), and numpy statements of what a bond update on it must produce.
Shared by test_tall_svd_cpu.py and test_tall_svd_gpu.py."""
import numpy as np

import ref_planner as pl
from hubbardtn_amd import engine, models, mps

L, CAP, SEED = 14, 150, 5
I0 = L // 2 - 1          # the bond update on sites (I0, I0 + 1) decomposes the centre bond L // 2


def hamiltonian():
    return models.hamiltonian(models.OB_Sim([1.0], [4.0]), L)


def coupled_blocks(eng, i):
    """{sector: rows x cols matrix} of theta(i) in the library's layout (tests/ref_planner.ThetaLayout)"""
    eb = eng.bonds
    tl = pl.ThetaLayout.build(eb[i], eb[i + 2])
    th = eng.theta(i)
    assert th.size == tl.size
    return {c: th[off:off + rows * cols].reshape(cols, rows).T for c, (off, rows, cols, *_) in tl.mats.items()}


def largest_block(blocks):
    return max(min(M.shape) for M in blocks.values())


def centred_engine(ops, **kw):
    """the random state with its centre moved to site I0 by non-optimising updates (no truncation)"""
    bonds, tens = mps.random_mps(L, (L, 0), CAP, seed=SEED)
    eng = engine.DMRG2(ops, hamiltonian(), bonds, tens, chi_full=None, **kw)
    for i in range(I0):
        eng.update_bond(i, +1, "right", optimise=False, record=False, cutoff=0.0)
    return eng


def schmidt_reference(blocks):
    """Schmidt values the update must report: theta's blocks are stored in the Euclidean ("tilde") normalisation, so the
    Schmidt values of sector c are its singular values over sqrt(2S_c + 1) (the label's second entry is 2S), scaled so
    that sum_c (2S_c + 1) sum s^2 = 1"""
    sv = {c: np.linalg.svd(M, compute_uv=False) / np.sqrt(c[1] + 1) for c, M in blocks.items()}
    nrm = np.sqrt(sum((c[1] + 1) * float(np.sum(s ** 2)) for c, s in sv.items()))
    return {c: s / nrm for c, s in sv.items()}


def assert_spectrum_matches(got, ref, rel=1e-8, floor=1e-6):
    """every reference value >= floor * max must be reported to rel (per value)"""
    smax = max(float(s.max()) for s in ref.values())
    for c, s in ref.items():
        big = s[s >= floor * smax]
        if big.size == 0:
            continue
        assert c in got, c
        g = np.sort(np.asarray(got[c]))[::-1]
        assert g.size >= big.size, (c, g.size, big.size)
        assert np.abs(g[:big.size] / big - 1.0).max() <= rel, c


def assert_left_isometry(eng, site, tol=1e-12):
    """A_site (left layout): orthonormal columns per right sector"""
    assert eng.site_kind(site) == "L"
    acc = {}
    for (l, s, r), blk in eng.download_site(site).items():
        acc[r] = acc.get(r, 0) + blk.conj().T @ blk
    for c, g in acc.items():
        assert np.abs(g - np.eye(g.shape[0])).max() < tol, (site, c)


def largest_coupled_block(eng):
    """max over the chain's two-site layouts of min(rows, cols) of a coupled-sector block, and the bond where it sits"""
    eb = eng.bonds
    best = (0, -1)
    for i in range(len(eb) - 2):
        tl = pl.ThetaLayout.build(eb[i], eb[i + 2])
        for (_, rows, cols, *_) in tl.mats.values():
            best = max(best, (min(rows, cols), i))
    return best
