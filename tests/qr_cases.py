"""Shared by test_dmrg1_cpu.py / test_dmrg1_gpu.py: the matrix cases of htn_qr_blocks_z, numpy's Householder QR on the same
inputs as the yardstick, and the checks.  Every case has ld > m; each runs as QR (trans = 0) and as LQ (trans = 1)."""
import numpy as np

from hubbardtn_amd import abi

EPS = np.finfo(np.float64).eps
W = abi.QR_PANEL            # panel width of the kernel
CHUNK = abi.QR_CHUNK        # rows one pass of its row loops covers


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
    return out


def pack(mats, trans):
    """-> (A flat, desc, R size): every block stored with ld = rows + 3 and a gap between blocks; trans = 1 stores the
    conjugate transpose (an n x m view), the kernel factorises the logical matrix either way"""
    desc = np.zeros(len(mats), dtype=abi.QR_DT)
    chunks, off, roff = [], 0, 0
    for k, Mx in enumerate(mats):
        m, n = Mx.shape
        V = Mx.conj().T if trans else Mx
        ld = V.shape[0] + 3
        buf = np.full((ld, V.shape[1]), 7.5 - 2.5j, dtype=np.complex128, order="F")       # padding rows: must stay untouched
        buf[:V.shape[0], :] = V
        chunks.append(buf.reshape(-1, order="F"))
        chunks.append(np.full(5, -1.25 + 0j))
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
    assert np.all(pad == 7.5 - 2.5j), "padding rows of the view were written"
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


def check(name, trans, mats, flat, rflat, desc, well_conditioned_orth_bar=None):
    """prints every figure, then asserts; returns the figures"""
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
    return figs
