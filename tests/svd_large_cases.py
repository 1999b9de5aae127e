"""Shared by test_svd_large_cpu.py / test_svd_large_gpu.py: the cases of the three multi-workgroup Jacobi SVD paths of
htn_svd.hip -- the ring (k_jacobi_ring), the pair visits (k_jacobi_pairs_gram + k_jacobi_check + k_jacobi_finish, the same
blocks in a process started with HTN_SVD_PAIRS=1) and the tall visits (k_jacobi_tall_visit + k_jacobi_check) -- at the
smallest shapes that reach them.  Blocks, truth (np.clongdouble Hestenes), bars and checks are those of svd_cases.py.

Which path a block takes, and in which geometry, is decided on the host (htn_jacobi_svd_z, classify_large, plan_ring);
geometry() states those rules a second time, in Python:

  large   QRCP, n >= 2, host descriptors, padded_rows(n0) x r > min(split or WINDOW, WINDOW)
  ring    gs = 16 up to 256 rows (n0), 64 above; mp = gs ceil(n0 / gs); wcap = min(512 / gs, 4608 / mp), for gs = 16 a wcap
          of 17..31 becomes 16, with split > 0 it is capped at 3; P = ceil(r / (2 wcap)) workgroups, panels of
          w = ceil(r / (2 P)) columns
  tall    plain, m > 512, host descriptors: panels of 8 columns, a visit is 16 columns

EXPECT is the table (shape, split) -> (path, gs, P, w) of what every block is meant to run (tall: gs None, P the number of
panels); the module asserts it when the cases are built, so a later change of the kernels' constants cannot quietly move
a case.  Shapes are G0 m0 x n0 for QRCP blocks -- the rotated matrix is n0 x r, r = min(m0, n0) <= 100 to keep the truth
affordable -- and m x n for tall blocks.  Wide tall blocks (n > m > 512) are left to tests/test_tall_svd_gpu.py: they need
more than 513 columns.

Without a rank cut (none of these calls passes one) the large paths rotate all r columns of R^H whatever the rank the QR
found: an all-zero block and a rank-1 block run the ring / the visits with columns that are exactly zero, which no
rotation touches (zero2 = 0, |a|^2 <= zero2), and finish after one sweep that saw nothing.

The stopping rule: last_sweep_old() is what the three paths used (done = mx <= max(tol^2, 0.1 tol)), last_sweep() restates
jacobi_last_sweep of htn_svd_cols.h.  twin_stopped() runs the complex128 Hestenes loop of svd_cases with either."""
import numpy as np

from svd_cases import (EPS, GAP, MAX_SWEEPS, MULTIPLETS, TOL, WINDOW, Block, Call, _rand, check, check_plain,  # noqa: F401
                       check_qrcp, graded_spectrum, hestenes, orthogonal_columns, pack, padded_rows, ref_of,
                       relative_deviation, run, same_bytes, scale_report, twin_of, with_spectrum)

RING_THREADS = 512          # of htn_svd_ring.h
RING_PANEL_ELEMS = 4608
RING_MAX_P = 64
JAC_PANEL = 8               # of htn_svd_visits.h
TALL_ROWS = 512             # plain blocks with more rows are tall


def ring_gs(rows):
    return 16 if rows <= 256 else 64


def geometry(kind, shape, split=0, host=True):
    """(path, gs, P, w) of a block: path "one" (the one-workgroup kernel), "ring" (pair visits in a process with
    HTN_SVD_PAIRS=1, same blocks) or "tall" """
    if kind == "plain":
        m, n = shape
        if m > TALL_ROWS and host:
            return ("tall", None, -(-n // JAC_PANEL), JAC_PANEL)
        return ("one", None, None, None)
    m0, n0 = shape
    r = min(m0, n0)
    if not (host and r >= 2 and padded_rows(n0) * r > min(split or WINDOW, WINDOW)):
        return ("one", None, None, None)
    gs = ring_gs(n0)
    mp = gs * -(-n0 // gs)
    wcap = min(RING_THREADS // gs, RING_PANEL_ELEMS // mp)
    if gs == 16 and 16 < wcap < 32:
        wcap = 16
    if split > 0:
        wcap = min(wcap, 3)
    P = max(1, -(-r // (2 * wcap)))
    assert wcap >= 1 and P <= RING_MAX_P
    return ("ring", gs, P, -(-r // (2 * P)))


class LargeBlock(Block):
    def __init__(self, name, kind, M, split=0, **kw):
        super().__init__(name, kind, M, **kw)
        self.split = split

    def instance(self):
        return geometry(self.kind, self.M.shape, self.split)


class LargeCall(Call):
    def __init__(self, name, blocks, split=0):
        super().__init__(name, blocks, host=True)
        self.split = split

    def ring(self):
        return self.blocks[0].kind == "qrcp"


def run_large(ops, call, P=None):
    return run(ops, call, P, split=call.split, max_sweeps=MAX_SWEEPS)


# ---- the stopping rules and their twin ----------------------------------------------------------------------------------
def last_sweep_old(mx, t2, tol):
    """what k_jacobi_ring, run_pair_visits and jacobi_svd_tall decided by: the largest squared cosine alone"""
    return mx <= max(tol * tol, 0.1 * tol)


def last_sweep(mx, t2, tol):
    """jacobi_last_sweep (htn_svd_cols.h): mx the largest squared cosine the sweep saw, t2 the largest tan^2 it rotated by"""
    tol2 = tol * tol
    return mx <= tol2 or (mx <= 0.1 * tol and t2 * mx <= tol2)


def twin_stopped(b, rule):
    """the complex128 twin (svd_cases.twin_of) stopped by `rule` -> (singular values, descending; sweeps)"""
    return hestenes(b.M, dtype=np.complex128, tol=TOL, zero_rel=1e-15, max_sweeps=MAX_SWEEPS,
                    stop=lambda mx, t2: rule(float(mx), float(t2), TOL))


def qrcp_twin(M):
    """R^H of a column-pivoted QR of M in complex128 (modified Gram-Schmidt, every column projected twice): what the large
    paths rotate, n0 x r, by plain numpy"""
    A = np.array(M, dtype=np.complex128)
    m0, n0 = A.shape
    r = min(m0, n0)
    R = np.zeros((r, n0), dtype=np.complex128)
    for j in range(r):
        p = int(np.argmax((np.abs(A) ** 2).sum(axis=0)))
        nrm = np.linalg.norm(A[:, p])
        if nrm == 0.0:
            break
        q = A[:, p] / nrm
        for _ in range(2):
            c = q.conj() @ A
            R[j] += c
            A -= np.outer(q, c)
        A[:, p] = 0.0
    return R.conj().T


# ---- the cases -----------------------------------------------------------------------------------------------------------
# (shape, split) -> (path, gs, P, w).  Ring, 16-lane form: E = 13 with P = 2; the last row count of the form; w = 25 with
# the first and the last workgroup only; with split = 1 seven workgroups (interior ones) of panels 3 wide -- (40, 40): the
# last panel holds one column, (41, 50): the last workgroup starts with panels of 3 and 2 columns, (37, 50): with one of 1
# column and an EMPTY one (14 panels of 3 for 37 columns).  64-lane form: its first row count; P = 3, w = 7 with a last
# panel of 5; the most rows.
EXPECT = {
    "ring16": [(((48, 202), 0), ("ring", 16, 2, 12)), (((40, 256), 0), ("ring", 16, 2, 10)),
               (((100, 100), 0), ("ring", 16, 2, 25))],
    "ring16_split": [(((40, 40), 1), ("ring", 16, 7, 3)), (((41, 50), 1), ("ring", 16, 7, 3)),
                     (((37, 50), 1), ("ring", 16, 7, 3))],
    "ring64": [(((36, 257), 0), ("ring", 64, 3, 6)), (((40, 280), 0), ("ring", 64, 3, 7)),
               (((24, 512), 0), ("ring", 64, 2, 6))],
    # tall, plain: one pair of columns; three panels, the last a single column; three full panels; 8 + 4 columns; 8 + 1
    "tall": [(((513, 2), 0), ("tall", None, 1, 8)), (((520, 17), 0), ("tall", None, 3, 8)),
             (((600, 24), 0), ("tall", None, 3, 8)), (((600, 12), 0), ("tall", None, 2, 8)),
             (((530, 9), 0), ("tall", None, 2, 8))],
}
TALL_ACC = {(513, 2): True, (520, 17): False, (600, 24): True, (600, 12): True, (530, 9): False}
SHAPE_CALLS = ("ring16", "ring16_split", "ring64", "tall")
# spectra, one carrier per path: (suffix of the call, kind, shape, split)
CARRIERS = (("r16", "qrcp", (48, 202), 0), ("r64", "qrcp", (40, 280), 0), ("r16x7", "qrcp", (40, 40), 1),
            ("tall", "plain", (600, 24), 0))
CARRIER_EXPECT = {"r16": ("ring", 16, 2, 12), "r64": ("ring", 64, 3, 7), "r16x7": ("ring", 16, 7, 3),
                  "tall": ("tall", None, 3, 8)}
SPECTRA = ("graded", "multiplets", "cluster", "rank0", "rank1", "rank_half", "zero_columns", "orthogonal", "scaled",
           "column_graded")


def _build():
    calls = {}
    rng = np.random.default_rng(4101)
    for name in SHAPE_CALLS:
        blocks = []
        for (shape, split), _ in EXPECT[name]:
            kind = "plain" if name == "tall" else "qrcp"
            M = with_spectrum(rng, shape[0], shape[1], graded_spectrum(min(shape)))
            blocks.append(LargeBlock(f"{name}_{shape[0]}x{shape[1]}", kind, M, split=split, acc=TALL_ACC.get(shape, False)))
        splits = {s for (_, s), _ in EXPECT[name]}
        assert len(splits) == 1
        calls[name] = LargeCall(name, blocks, split=splits.pop())
        got = [b.instance() for b in blocks]
        want = [g for _, g in EXPECT[name]]
        assert got == want, f"{name}: geometry {got}, meant for {want}"

    rng = np.random.default_rng(4102)

    def matrices(spec, kind, shape):
        """-> [(suffix, M, keywords of the block)]"""
        k = min(shape)
        spectrum = {"graded": lambda: graded_spectrum(k), "multiplets": lambda: MULTIPLETS,
                    "cluster": lambda: 1.0 + 1e-13 * np.arange(k), "rank0": lambda: [], "rank1": lambda: [1.0],
                    "rank_half": lambda: graded_spectrum(k // 2, 8.0)}
        if spec in spectrum:
            s = spectrum[spec]()
            return [("", with_spectrum(rng, shape[0], shape[1], s), {"rank": len(s) if spec.startswith("rank") else None})]
        if spec == "zero_columns":
            M = with_spectrum(rng, shape[0], shape[1], graded_spectrum(k, 8.0))
            M[:, (3, shape[1] - 5)] = 0.0
            return [("", M, {"rank": min(shape[0], shape[1] - 2)})]
        if spec == "orthogonal":
            if shape[0] < shape[1]:
                return []           # more orthogonal columns than rows do not exist
            d = 1.0 / (1.0 + 0.37 * np.arange(shape[1]))
            return [("", orthogonal_columns(rng, shape[0], shape[1], d), {"diag": d})]
        if spec == "scaled":
            M = with_spectrum(rng, shape[0], shape[1], graded_spectrum(k))
            return [("", M, {})] + [(sfx, np.ldexp(M.real, p) + 1j * np.ldexp(M.imag, p), {"scaled": (None, p)})
                                    for sfx, p in (("_up", 100), ("_down", -100))]
        assert spec == "column_graded"
        if kind != "plain":
            return []               # the tall carrier only
        B = _rand(rng, shape[0], 12)
        B /= np.linalg.norm(B, axis=0)
        return [("", B * graded_spectrum(12), {"colgraded": True})]

    for spec in SPECTRA:
        for cname, kind, shape, split in CARRIERS:
            name = f"{spec}_{cname}"
            blocks = []
            for sfx, M, kw in matrices(spec, kind, shape):
                if kw.get("scaled"):
                    kw["scaled"] = (name, kw["scaled"][1])
                blocks.append(LargeBlock(name + sfx, kind, M, split=split, acc=True, **kw))
            if not blocks:
                continue
            for b in blocks:
                want = CARRIER_EXPECT[cname] if not b.colgraded else ("tall", None, 2, 8)
                assert b.instance() == want, (b.name, b.instance(), want)
            calls[name] = LargeCall(name, blocks, split=split)
    for c in calls.values():
        for b in c.blocks:
            assert b.n <= 100, (b.name, "the truth is kept affordable: at most 100 rotated columns")
            assert b.instance()[0] == ("ring" if c.ring() else "tall"), (c.name, b.name)
            assert b.split == c.split and (b.kind == "qrcp") == c.ring()
    names = [b.name for c in calls.values() for b in c.blocks]
    assert len(set(names)) == len(names)
    return calls


CALLS = _build()
SPECTRUM_CALLS = tuple(n for n in CALLS if n not in SHAPE_CALLS)
RING_CALLS = tuple(n for n in CALLS if CALLS[n].ring())          # what the pair visits run as well
CLUSTER_CALLS = tuple(n for n in SPECTRUM_CALLS if n.startswith("cluster_"))
