"""Shared by test_dmrg1_cpu.py / test_dmrg1_gpu.py: the matrix cases of htn_qr_blocks_z, numpy's Householder QR on the same
inputs as the yardstick, and the checks.  Every case has ld > m; each runs as QR (trans = 0) and as LQ (trans = 1).

The kernel's control flow depends on the block shape: the panel width w (16 while 16 columns of m rows fit the LDS panel,
halved beyond: panel_width), and the number of 128-column rounds in which a panel is projected against the finished
columns (projection_rounds).  EXPECT pins every case added for one of these paths to the (w, rounds) it is meant for; the
module asserts it on import, so a later change of the kernel's constants cannot quietly move a case to another path."""
import numpy as np

from hubbardtn_amd import abi

EPS = np.finfo(np.float64).eps
W = abi.QR_PANEL            # panel width of the kernel
CHUNK = abi.QR_CHUNK        # rows one pass of its row loops covers
PANEL_ELEMS = 7680          # complex128 elements of the kernel's LDS panel (QR_PANEL_ELEMS of htn_qr.hip)
GROUP = 128                 # finished columns projected per round (QR_GROUP: 16 per wave, eight waves)
R_SENTINEL = 3.25 + 1.5j    # what the R buffer holds before the call, wherever the library must not write
A_PAD = 7.5 - 2.5j          # padding rows of every A block
A_GAP = -1.25 + 0j          # the five elements after every A block


def panel_width(m):
    """the kernel's panel width for a block of m rows: halved from abi.QR_PANEL until w columns of stride
    mp = ((m + 15) & ~15) + 1 fit the LDS panel"""
    assert 1 <= m <= abi.QR_MAX_M
    mp = ((m + 15) & ~15) + 1
    w = W
    while w > 1 and w * mp > PANEL_ELEMS:
        w >>= 1
    return w


def projection_rounds(m, n):
    """rounds of GROUP finished columns the LAST panel of an m x n block is projected in (0: a single panel)"""
    w = panel_width(m)
    j0 = (n - 1) // w * w
    return -(-j0 // GROUP)


def width_edges():
    """[(m, w)]: the last m of every panel width and the first of the next, derived from the constants"""
    out, w = [], W
    while w >= 1:
        last = min((PANEL_ELEMS // w - 1) & ~15, abi.QR_MAX_M)      # largest m with w * (((m + 15) & ~15) + 1) <= PANEL_ELEMS
        out.append((last, w))
        if w > 1:
            out.append((last + 1, w >> 1))
        w >>= 1
    assert all(panel_width(m) == w for m, w in out) and out[-1][0] == abi.QR_MAX_M, out
    return out


def _rand(rng, m, n):
    return rng.normal(size=(m, n)) + 1j * rng.normal(size=(m, n))


def graded(rng, m, n, decades=12.0):
    """singular values graded over `decades` decades between random unitary factors"""
    U, _ = np.linalg.qr(_rand(rng, m, n))
    V, _ = np.linalg.qr(_rand(rng, n, n))
    s = 10.0 ** (-decades * np.arange(n) / max(n - 1, 1))
    return (U * s) @ V.conj().T


def dependent(rng, m, n):
    """three columns that are exact copies / sums of earlier ones"""
    A = _rand(rng, m, n)
    A[:, 5] = A[:, 2]
    A[:, n // 2] = A[:, 0] + A[:, 1]
    A[:, n - 1] = A[:, 3] - A[:, 4]
    return A


def cases():
    """name -> list of logical m x n matrices (one call each)"""
    rng = np.random.default_rng(2024)
    out = {}
    for n in (1, W - 1, W, W + 1, 2 * W + 1):
        for m in sorted({n, n + 1, 2 * n + 3}):
            out[f"n{n}_m{m}"] = [_rand(rng, m, n)]
    out["row_chunk"] = [_rand(rng, CHUNK + 18, 20)]              # m crosses the row-chunk length (and the full-width panel)
    out["big_600x130"] = [_rand(rng, 600, 130)]
    shapes = [(5, 3), (40, 17), (64, 64), (33, 1), (100, 31), (17, 16), (16, 16), (129, 47), (70, 33), (12, 12), (300, 20),
              (48, 32), (31, 30), (200, 65), (9, 2), (90, 49), (256, 16), (65, 15)]
    out["batch18"] = [_rand(rng, m, n) for m, n in shapes]
    out["graded12"] = [graded(rng, 150, 40)]
    out["dependent3"] = [dependent(rng, 60, 24)]

    rng = np.random.default_rng(2025)                             # (a stream of its own: the cases above keep their entries)
    # the last m of every panel width and the first of the next; n = 21 is a multiple of no width and two panels at w = 16
    edges = width_edges()
    out["width_edges_n21"] = [_rand(rng, m, 21) for m, _ in edges[:-1]]
    out["m_max_n21"] = [_rand(rng, edges[-1][0], 21)]             # m = abi.QR_MAX_M, a call of its own
    # a second and a third projection round (g0 = 128, 256) at every width that reaches one in a quick test
    out["rounds_160x160"] = [_rand(rng, 160, 160)]                # round g0 = 128: wave 0 alone is live
    out["rounds_300x290"] = [_rand(rng, 300, 290)]                # three rounds, the last with two live waves; nearly square:
    out["rounds_600x150"] = [_rand(rng, 600, 150)]                # late columns lose most of their norm -> re-projection
    out["rounds_2000x140"] = [_rand(rng, 2000, 140)]
    out["rounds_3825x140"] = [_rand(rng, edges[-2][0], 140)]      # w = 1: no Gram-Schmidt inside the panel at all
    out["graded12_1000x40"] = [graded(rng, 1000, 40)]
    out["graded12_2000x30"] = [graded(rng, 2000, 30)]
    out["dependent3_2000x24"] = [dependent(rng, 2000, 24)]        # replacement vectors orthogonalised against columns read
    A = _rand(rng, 40, 12)                                        # back from global memory
    A[:, 0] = 0.0
    out["zero_col0_40x12"] = [A]                                  # the replacement path with nothing before it (c = 0, j0 = 0)
    out["zeros_5x3"] = [np.zeros((5, 3), dtype=np.complex128)]
    A = _rand(rng, 70, 20)
    A[:, 16] = A[:, 1]
    A[:, 17] = A[:, 1]
    out["twin_dependent_70x20"] = [A]                             # two dependent columns side by side, first of the second panel
    for name, want in EXPECT.items():
        got = [(panel_width(M.shape[0]), projection_rounds(*M.shape)) for M in out[name]]
        assert got == want, f"{name}: (panel width, projection rounds) {got}, meant for {want}"
    assert set(GRADED) | set(PLANTED) <= set(out)
    return out


# (panel width, projection rounds of the last panel) every block of a case is meant to run at
EXPECT = {
    "big_600x130": [(8, 1)],
    "width_edges_n21": [(16, 1), (8, 1), (8, 1), (4, 1), (4, 1), (2, 1), (2, 1), (1, 1)],
    "m_max_n21": [(1, 1)],
    "rounds_160x160": [(16, 2)],
    "rounds_300x290": [(16, 3)],
    "rounds_600x150": [(8, 2)],
    "rounds_2000x140": [(2, 2)],
    "rounds_3825x140": [(1, 2)],
    "graded12_1000x40": [(4, 1)],
    "graded12_2000x30": [(2, 1)],
    "dependent3_2000x24": [(2, 1)],
    "zero_col0_40x12": [(16, 0)],
    "zeros_5x3": [(16, 0)],
    "twin_dependent_70x20": [(16, 1)],
}
# 12-decade blocks: they must meet the orthogonality bar of a well-conditioned block of their shape
GRADED = ("graded12", "graded12_1000x40", "graded12_2000x30")
# columns planted as exactly dependent on earlier ones (or zero), per block: R's diagonal is an exact 0.0 there -- both
# libraries promise it (include/hubbardtn_hip.h on htn_qr_blocks_z, htn_backend_host.cpp on qr_blocks_host) -- and positive
# on every other column of every case
PLANTED = {
    "dependent3": [{5, 12, 23}],
    "dependent3_2000x24": [{5, 12, 23}],
    "zero_col0_40x12": [{0}],
    "zeros_5x3": [{0, 1, 2}],
    "twin_dependent_70x20": [{16, 17}],
}


def orth_bar(name, mats):
    """the orthogonality bar of a GRADED case (None for every other case: check() then takes bars())"""
    if name not in GRADED:
        return None
    return bars(np.random.default_rng(5).normal(size=mats[0].shape) + 0j)[0]


def pack(mats, trans):
    """-> (A flat, desc, R size): every block stored with ld = rows + 3 and a gap between blocks; trans = 1 stores the
    conjugate transpose (an n x m view), the kernel factorises the logical matrix either way"""
    desc = np.zeros(len(mats), dtype=abi.QR_DT)
    chunks, off, roff = [], 0, 0
    for k, Mx in enumerate(mats):
        m, n = Mx.shape
        V = Mx.conj().T if trans else Mx
        ld = V.shape[0] + 3
        buf = np.full((ld, V.shape[1]), A_PAD, dtype=np.complex128, order="F")       # padding rows: must stay untouched
        buf[:V.shape[0], :] = V
        chunks.append(buf.reshape(-1, order="F"))
        chunks.append(np.full(5, A_GAP))
        desc[k] = (off, m, n, ld, 0, roff, n + 2, trans)
        off += buf.size + 5
        roff += (n + 2) * n + 1
    return np.concatenate(chunks), desc, roff


def unpack(flat, rflat, desc, k):
    """-> (Q, R) of the logical matrix of block k"""
    d = desc[k]
    m, n, ld, ldr, tr = int(d["m"]), int(d["n"]), int(d["ld"]), int(d["ldr"]), int(d["trans"])
    vr, vc = (n, m) if tr else (m, n)
    V = flat[int(d["offset"]):int(d["offset"]) + ld * vc].reshape(ld, vc, order="F")
    pad = V[vr:, :]
    assert np.all(pad == A_PAD), "padding rows of the view were written"
    Rs = rflat[int(d["r_offset"]):int(d["r_offset"]) + ldr * n].reshape(ldr, n, order="F")[:n, :]
    if tr:
        return V[:vr, :].conj().T.copy(), Rs.conj().T.copy()
    return V[:vr, :].copy(), Rs.copy()


def errors(Q, R, A):
    n = A.shape[1]
    orth = np.abs(Q.conj().T @ Q - np.eye(n)).max()
    nrm = np.linalg.norm(A)
    resid = np.linalg.norm(Q @ R - A) / (nrm if nrm > 0 else 1.0)
    return orth, resid


def numpy_errors(A):
    Q, R = np.linalg.qr(A)
    return errors(Q, R, A)


def bars(A):
    """10 x what LAPACK's Householder QR leaves on the same input, floor 256 eps"""
    o, r = numpy_errors(A)
    return max(10 * o, 256 * EPS), max(10 * r, 256 * EPS)


def check_padding(name, trans, flat, rflat, desc):
    """what the library must write and what it must leave alone, on an R buffer that held R_SENTINEL everywhere before the
    call (pack()'s layout: ldr = n + 2, one element between R blocks, five A_GAP elements after every A block):
    the strict lower (trans = 1: upper) triangle of every factor is an exact zero the library wrote; rows n .. ldr - 1 of
    every R column, the elements between R blocks and the fillers after every A block are untouched"""
    assert flat.size == int(desc[-1]["offset"]) + int(desc[-1]["ld"]) * int(desc[-1]["m" if desc[-1]["trans"] else "n"]) + 5
    assert rflat.size == int(desc[-1]["r_offset"]) + int(desc[-1]["ldr"]) * int(desc[-1]["n"]) + 1
    for k, d in enumerate(desc):
        m, n, ld, ldr, tr = int(d["m"]), int(d["n"]), int(d["ld"]), int(d["ldr"]), int(d["trans"])
        a_end = int(d["offset"]) + ld * (m if tr else n)
        assert np.all(flat[a_end:a_end + 5] == A_GAP), (name, trans, k, "the gap after the A block was written")
        ro = int(d["r_offset"])
        Rs = rflat[ro:ro + ldr * n].reshape(ldr, n, order="F")
        assert np.all(Rs[n:, :] == R_SENTINEL), (name, trans, k, "rows n .. ldr - 1 of R were written")
        assert rflat[ro + ldr * n] == R_SENTINEL, (name, trans, k, "the element after the R block was written")
        off_diag = np.triu(Rs[:n, :], 1) if tr else np.tril(Rs[:n, :], -1)
        assert np.all(off_diag == 0.0), (name, trans, k, "the zero triangle of R holds something else (not written?)")


def check(name, trans, mats, flat, rflat, desc, well_conditioned_orth_bar=None):
    """prints every figure, then asserts; returns the figures.  rflat must have held R_SENTINEL everywhere before the call."""
    check_padding(name, trans, flat, rflat, desc)
    planted = PLANTED.get(name, [set()] * len(mats))
    figs = []
    for k, A in enumerate(mats):
        Q, R = unpack(flat, rflat, desc, k)
        orth, resid = errors(Q, R, A)
        bo, br = bars(A)
        if well_conditioned_orth_bar is not None:
            bo = well_conditioned_orth_bar
        lower = np.abs(np.tril(R, -1)).max() if R.shape[0] > 1 else 0.0
        dg = np.diag(R)
        print(f"{name} trans={trans} block {k} {A.shape}: orth {orth:.3e} (bar {bo:.3e})  resid {resid:.3e} (bar {br:.3e})  "
              f"min diag {dg.real.min():.3e}")
        figs.append((orth, resid, bo, br))
        assert orth <= bo, (name, trans, k, orth, bo)
        assert resid <= br, (name, trans, k, resid, br)
        assert lower == 0.0, (name, trans, k, lower)
        assert np.all(dg.imag == 0.0) and np.all(dg.real >= 0.0), (name, trans, k)
        dep = np.zeros(A.shape[1], dtype=bool)
        dep[sorted(planted[k])] = True
        assert np.all(dg.real[dep] == 0.0), (name, trans, k, "a planted dependent column has no exact zero on R's diagonal", dg.real[dep])
        assert np.all(dg.real[~dep] > 0.0), (name, trans, k, "an independent column has a zero on R's diagonal")
    return figs
