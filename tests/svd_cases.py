"""Shared by test_svd_one_cpu.py / test_svd_one_gpu.py: the cases of the one-workgroup Jacobi SVD kernel (k_jacobi_svd of
htn_svd_one.h, its rotations in htn_svd_cols.h, its pivoted QR qrcp_mgs in htn_svd_qr.h), an extended-precision truth, and
the checks.

Which code a block runs is decided by its shape alone:

  plain block (m x n)          jacobi_sweeps<GS>, GS = 16 | 32 | 64 for m <= 128 | 256 | 512; the matrix sits in LDS when
                               m n <= WINDOW, else in global memory
  QRCP block (G0 is m0 x n0)   qrcp_mgs<GQ>, GQ by m0 like GS by m; then X = R^H (n0 x r, r = min(m0, n0)) is rotated by
                               jacobi_sweeps_pad<GS, E>, GS by n0, E = ceil(n0 / GS); X sits in LDS when GS E r <= WINDOW,
                               else in the block's Vj workspace

instance() states these rules a second time, in Python; EXPECT below is the table of what every block of every shape call
is meant to run, and the module asserts it when the cases are built: a later change of the kernel's constants cannot
quietly move a case to another instance.  Every call is also checked never to leave the one-workgroup kernel (routes()):
with the host copy of the descriptors no QRCP block is above the window; without it the host cannot classify anything.

Truth: cyclic one-sided (Hestenes) Jacobi in np.clongdouble on the double-rounded matrix (hestenes()), every sweep visiting
each column pair once, in rounds of disjoint pairs that numpy rotates together.  The bar of the singular values is what
numpy.linalg.svd itself leaves against that truth, times ten, floor 64 eps (ref_of())."""
import numpy as np
import pytest

from hubbardtn_amd import abi

EPS = np.finfo(np.float64).eps
EPSL = np.finfo(np.longdouble).eps
if not EPSL < 1e-18:
    pytest.skip(f"np.longdouble is no extended precision here (eps {EPSL:.1e}): no truth for the Jacobi SVD cases",
                allow_module_level=True)

WINDOW = 9216               # complex128 elements of the kernel's LDS window (JAC_LDS_ELEMS of htn_svd.hip)
MAXEL = 8                   # column elements per lane (JAC_MAXEL): rows <= GS * MAXEL
TOL = 1e-14                 # what every call passes as tol ...
MAX_SWEEPS = 40             # ... and as max_sweeps
GAP = 7                     # NaN elements after every block's region of G, S and Vj
V_SENTINEL = 7.0 + 3.0j     # the Vj region of a plain block without HTN_SVD_ACCUMULATE
INFO_FILL = -77


def group_size(rows):
    assert 1 <= rows <= 64 * MAXEL
    return 16 if rows <= 16 * MAXEL else (32 if rows <= 32 * MAXEL else 64)


def padded_rows(rows):
    gs = group_size(rows)
    return gs * -(-rows // gs)


class Block:
    """one block of a call.  kind "plain": M is G (m x n); kind "qrcp": M is G0 (m0 x n0).
    rank: planted exact rank (None: full); diag: the positive diagonal of an already orthogonal block; colgraded: the
    column-graded block of the relative-accuracy test; scaled: (name of the unscaled block, power of two)"""

    def __init__(self, name, kind, M, acc=False, rank=None, diag=None, colgraded=False, scaled=None):
        assert kind in ("plain", "qrcp")
        self.name, self.kind, self.M, self.acc = name, kind, np.asarray(M, dtype=np.complex128), acc
        self.rank, self.diag, self.colgraded, self.scaled = rank, diag, colgraded, scaled
        r0, c0 = self.M.shape
        if kind == "qrcp":      # descriptor: m = n0, n = r, pad = m0
            self.m, self.n, self.pad, self.flags = c0, min(r0, c0), r0, abi.SVD_QRCP
            self.g_size, self.v_size = r0 * c0, -(-c0 // 64) * 64 * self.n
        else:
            self.m, self.n, self.pad, self.flags = r0, c0, 0, (abi.SVD_ACCUMULATE if acc else 0)
            self.g_size, self.v_size = r0 * c0, c0 * c0
        self.s_size = self.n

    def instance(self):
        """(path, GS, E, window) the kernel runs this block at; QRCP blocks add the group size of qrcp_mgs"""
        if self.kind == "qrcp":
            gs = group_size(self.m)
            e = -(-self.m // gs)
            return ("qrcp", gs, e, "lds" if gs * e * self.n <= WINDOW else "global", group_size(self.pad))
        return ("plain", group_size(self.m), None, "lds" if self.m * self.n <= WINDOW else "global")

    def above_window(self):
        return self.instance()[3] == "global"


class Call:
    def __init__(self, name, blocks, host):
        self.name, self.blocks, self.host = name, list(blocks), host      # host: pass the host copy of the descriptors


def routes(call):
    """the call stays in k_jacobi_svd: nothing taller than 512 rows, and where the host sees the descriptors
    (classify_large) no QRCP block of two or more columns is above the window"""
    for b in call.blocks:
        assert max(b.m, b.pad) <= 64 * MAXEL, (call.name, b.name)
        assert b.n <= 96, (call.name, b.name, "the truth is kept affordable: at most 96 columns")
        if call.host:
            assert not (b.kind == "qrcp" and b.n >= 2 and padded_rows(b.m) * b.n > WINDOW), (call.name, b.name)
    if not call.host:
        assert any(b.above_window() for b in call.blocks), (call.name, "a call without the host descriptors is for blocks above the window")


# ---- matrices ----------------------------------------------------------------------------------------------------------
def _rand(rng, m, n):
    return rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n))


def with_spectrum(rng, m, n, s):
    """U diag(s) W^H in double, U (m x k) and W (n x k) with orthonormal columns, k = len(s) <= min(m, n)"""
    s = np.asarray(s, dtype=np.float64)
    k = len(s)
    assert k <= min(m, n)
    if k == 0:
        return np.zeros((m, n), dtype=np.complex128)
    U, _ = np.linalg.qr(_rand(rng, m, k))
    W, _ = np.linalg.qr(_rand(rng, n, k))
    return (U * s) @ W.conj().T


def graded_spectrum(k, decades=12.0):
    return 10.0 ** (-decades * np.arange(k) / max(k - 1, 1))


def orthogonal_columns(rng, m, n, d):
    """(m x n isometry) diag(d): the isometry is polished in extended precision (two Newton-Schulz steps) and the product
    rounded to double once, so the column norms are d to a fraction of eps and the cosines are at rounding level"""
    U, _ = np.linalg.qr(_rand(rng, m, n))
    U = U.astype(np.clongdouble)
    for _ in range(2):
        U = U @ (3 * np.eye(n, dtype=np.clongdouble) - U.conj().T @ U) / 2
    return (U * np.asarray(d, dtype=np.longdouble)).astype(np.complex128)


# ---- truth ---------------------------------------------------------------------------------------------------------------
def _rounds(n):
    """round-robin tournament over n columns: n - 1 (n even) or n (n odd) rounds of disjoint pairs, every pair once"""
    npad = n + (n & 1)
    out = []
    for r in range(npad - 1):
        I, J = [], []
        for p in range(npad // 2):
            i, j = (npad - 1, r) if p == 0 else ((r + p) % (npad - 1), (r + npad - 1 - p) % (npad - 1))
            if i < n and j < n:
                I.append(min(i, j))
                J.append(max(i, j))
        out.append((np.array(I, dtype=np.int64), np.array(J, dtype=np.int64)))
    return out


def hestenes(M, dtype=np.clongdouble, tol=None, zero_rel=None, max_sweeps=60, stop=None):
    """cyclic one-sided Jacobi on the columns of M (of M^H when M is wide) in `dtype`: a pair is rotated when its squared
    cosine exceeds tol^2 (default 4 eps of dtype), sweeps go on until one has rotated nothing.  A column below
    zero_rel |M|_F (default 1000 eps) takes no part: it is the rounding residue of an exactly rank-deficient input and
    has no direction; its norm, below that threshold, is still reported.  -> (column norms, descending; sweeps)
    stop(mx, t2) -> bool (the twins of the kernels' stopping rules, svd_large_cases.py): decides instead whether a sweep
    was the last, from the largest squared cosine it saw before its rotations and the largest tan^2 it rotated by"""
    A = np.array(M, dtype=dtype)
    if A.shape[0] < A.shape[1]:
        A = A.conj().T.copy()
    real = A.real.dtype.type
    eps = np.finfo(real).eps
    tol2 = real(4 * eps if tol is None else tol) ** 2
    n = A.shape[1]
    zero2 = real(1000 * eps if zero_rel is None else zero_rel) ** 2 * (A.real ** 2 + A.imag ** 2).sum()
    rounds = _rounds(n)
    for sweep in range(1, max_sweeps + 1):
        rotated = False
        mx = t2 = real(0)
        for I, J in rounds:
            a, b = A[:, I], A[:, J]
            aa = (a.real ** 2 + a.imag ** 2).sum(axis=0)
            bb = (b.real ** 2 + b.imag ** 2).sum(axis=0)
            g = (a.conj() * b).sum(axis=0)
            g2 = g.real ** 2 + g.imag ** 2
            live = (aa > zero2) & (bb > zero2)
            if stop is not None and live.any():
                mx = max(mx, (g2[live] / (aa[live] * bb[live])).max())
            k = np.nonzero(live & (g2 > tol2 * aa * bb))[0]
            if len(k) == 0:
                continue
            rotated = True
            ga = np.sqrt(g2[k])
            zeta = (bb[k] - aa[k]) / (2 * ga)
            t = np.where(zeta >= 0, real(1), real(-1)) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
            t2 = max(t2, (t * t).max())
            c = 1 / np.sqrt(1 + t * t)
            s = c * t
            bt = b[:, k] * (g[k] / ga).conj()           # a^H bt = |a^H b|: a real rotation finishes the pair
            ak = a[:, k]
            A[:, I[k]] = c * ak - s * bt
            A[:, J[k]] = s * ak + c * bt
        if stop(mx, t2) if stop is not None else not rotated:
            break
    else:
        raise AssertionError(f"hestenes: {max_sweeps} sweeps of a {A.shape} matrix in {np.dtype(dtype)} did not converge")
    nrm = np.sqrt((A.real ** 2 + A.imag ** 2).sum(axis=0))
    return np.sort(nrm)[::-1], sweep


_REF = {}


def ref_of(b):
    """(truth padded with zeros to the block's n, in longdouble; sigma_max; bar), computed once per block name.
    bar = max(10 x max |numpy.linalg.svd - truth| / sigma_max, 64 eps): numpy's own deviation, never the kernel's"""
    if b.name not in _REF:
        truth, _ = hestenes(b.M)
        lap = np.linalg.svd(b.M, compute_uv=False)
        sig = float(truth[0]) if len(truth) else 0.0
        npdev = float(np.abs(lap.astype(np.longdouble) - truth).max()) / sig if sig > 0 else 0.0
        full = np.zeros(b.n, dtype=np.longdouble)
        full[:len(truth)] = truth
        _REF[b.name] = (full, sig, max(10 * npdev, 64 * EPS), npdev)
    return _REF[b.name][:3]


def numpy_deviation(b):
    ref_of(b)
    return _REF[b.name][3]


def twin_of(b):
    """the same Hestenes loop in complex128 with the kernel's tol, zero-column threshold and sweep limit: what plain double
    arithmetic makes of the algorithm -> singular values, descending"""
    return hestenes(b.M, dtype=np.complex128, tol=TOL, zero_rel=1e-15, max_sweeps=MAX_SWEEPS)[0]


def relative_deviation(s_sorted, b):
    truth = ref_of(b)[0]
    return float(np.abs(np.asarray(s_sorted, dtype=np.longdouble) / truth - 1).max())


# ---- buffers -------------------------------------------------------------------------------------------------------------
class Packed:
    pass


def pack(call):
    """G, Vj, S as the call gets them: every block's region followed by GAP NaN elements.  A QRCP block's G region is G0
    (m0 x n0, column major), its Vj region the roundup(n0, 64) x r workspace (NaN: the kernel must fill what it reads); a
    plain block's Vj region is n x n, NaN with HTN_SVD_ACCUMULATE and V_SENTINEL without"""
    P = Packed()
    nb = len(call.blocks)
    P.desc = np.zeros(nb, dtype=abi.SVD_DT)
    nan = np.nan + 1j * np.nan
    g, v, P.regions = [], [], []
    go = vo = so = 0
    for k, b in enumerate(call.blocks):
        P.desc[k] = (go, vo, so, b.m, b.n, b.flags, b.pad)
        P.regions.append((go, vo, so))
        g += [b.M.T.reshape(-1), np.full(GAP, nan)]
        v += [np.full(b.v_size, V_SENTINEL if (b.kind == "plain" and not b.acc) else nan), np.full(GAP, nan)]
        go, vo, so = go + b.g_size + GAP, vo + b.v_size + GAP, so + b.s_size + GAP
    P.G, P.V, P.S = np.concatenate(g), np.concatenate(v), np.full(so, np.nan)
    P.info = np.full(nb, INFO_FILL, dtype=np.int32)
    P.max_m = max(max(b.m, b.pad) for b in call.blocks)
    return P


def run(ops, call, P=None, split=0, max_sweeps=MAX_SWEEPS):
    """one htn_jacobi_svd_z call from fresh copies of the packed buffers -> (G, Vj, S, info on the host, return value).
    split: htn_svd_opts.split_elems, the test mode that sends QRCP blocks below the window to the large-block path"""
    P = pack(call) if P is None else P
    dG, dV, dS, info = ops.to_device(P.G), ops.to_device(P.V), ops.to_device(P.S), ops.to_device(P.info)
    used = ops.jacobi_svd(dG, dV, dS, ops.to_device(P.desc), len(call.blocks), P.max_m, max_sweeps, TOL, info,
                          desc_host=P.desc if call.host else None, **({"split": split} if split else {}))
    return ops.to_host(dG), ops.to_host(dV), ops.to_host(dS), ops.to_host(info), used


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _gaps_untouched(what, before, after, spans):
    inside = np.zeros(before.size, dtype=bool)
    for off, size in spans:
        inside[off:off + size] = True
    assert (~inside).sum() == GAP * len(spans)
    assert same_bytes(before[~inside], after[~inside]), f"{what}: a gap between the blocks' regions was written"
    assert np.isnan(after[~inside].real).all()


# ---- checks --------------------------------------------------------------------------------------------------------------
def check_plain(b, gp, s, J, ref, sig, bar):
    """the contract of a plain block, as tests/test_kernels_gpu.py::test_jacobi_svd_matches_lapack states it, against the
    truth and its bar: G' = G J has orthogonal columns whose norms are the singular values"""
    got = np.sort(s)[::-1]
    dev = float(np.abs(got - ref).max())
    print(f"{b.name}: |S - truth| {dev:.3e}, bar x sigma_max {bar * sig:.3e}")
    assert dev <= bar * sig, (b.name, "singular values", dev, bar * sig)
    gram = gp.conj().T @ gp
    dg = np.sqrt(np.abs(np.diag(gram)))
    live = dg > 1e-14 * sig                 # columns below 1e-15 |G|_F are treated as zero by the kernel
    off = np.abs(gram - np.diag(np.diag(gram)))[np.ix_(live, live)]
    assert (off <= 1e-13 * np.outer(dg[live], dg[live])).all(), (b.name, "live columns are not mutually orthogonal")
    assert live.sum() >= (ref > 1e-13 * sig).sum(), (b.name, "fewer live columns than the numerical rank")
    if b.acc:
        n = b.n
        assert np.abs(J.conj().T @ J - np.eye(n)).max() < 1e-13, (b.name, "J is not unitary")
        assert np.abs(b.M @ J - gp).max() <= 1e-13 * sig, (b.name, "G' != M J")
    else:
        assert same_bytes(J, np.full((b.n, b.n), V_SENTINEL)), (b.name, "Vj was written without HTN_SVD_ACCUMULATE")
    return dev


def check_qrcp(b, out, s, ref, sig, bar):
    """the contract of a QRCP block, as test_jacobi_svd_qr_preconditioned states it: out (n0 x r, rows in the original
    column order of G0) = right singular vectors x Sigma"""
    order = np.argsort(-s)
    dev = float(np.abs(s[order] - ref).max())
    print(f"{b.name}: |S - truth| {dev:.3e}, bar x sigma_max {bar * sig:.3e}")
    assert dev <= bar * sig, (b.name, "singular values", dev, bar * sig)
    live = s > 1e-13 * sig
    if live.any():
        Viso = out[:, live] / s[live]
        assert np.abs(Viso.conj().T @ Viso - np.eye(live.sum())).max() < 1e-12, (b.name, "live columns are not orthonormal")
        assert np.abs(np.linalg.norm(b.M @ Viso, axis=0) - s[live]).max() <= 1e-12 * sig, (b.name, "|G0 v| != sigma")
        resid = b.M.conj().T @ (b.M @ Viso) - Viso * s[live] ** 2
        assert np.abs(resid).max() <= 1e-12 * sig ** 2, (b.name, "G0^H G0 v != sigma^2 v")
    return dev


def check(call, P, result, check_info=True, check_relative=True, large=False):
    """prints every figure, then asserts; -> {block name: (deviation / sigma_max, bar, sorted S)}.
    check_relative=False leaves out the one RELATIVE bound (S of an already orthogonal block to 4 eps of every entry): a
    property of one-sided Jacobi that LAPACK, accurate to eps sigma_max, does not have.
    large=True (svd_large_cases.py): the call is meant for the multi-workgroup paths, whose outer sweeps the return value
    counts: it must be >= 1, and comes back beside the figures -> (figures, used)"""
    G, V, S, info, used = result
    if large:
        assert used is not None and used >= 1, (call.name, "the call stayed in the one-workgroup kernel", used)
    else:
        assert used in (0, None), (call.name, "the call left the one-workgroup kernel: outer sweeps of the large-block path", used)
    _gaps_untouched("G", P.G, G, [(go, b.g_size) for (go, _, _), b in zip(P.regions, call.blocks)])
    _gaps_untouched("Vj", P.V, V, [(vo, b.v_size) for (_, vo, _), b in zip(P.regions, call.blocks)])
    _gaps_untouched("S", P.S, S, [(so, b.s_size) for (_, _, so), b in zip(P.regions, call.blocks)])
    figs, failures = {}, []
    for k, ((go, vo, so), b) in enumerate(zip(P.regions, call.blocks)):
        try:        # every block is measured and printed before the first failure is raised
            figs[b.name] = _check_block(call, b, k, go, vo, so, G, V, S, info, check_info, check_relative)
        except AssertionError as e:
            print(f"{call.name} / {b.name}: FAILED {e}")
            failures.append(e)
    if failures:
        raise failures[0]
    return (figs, used) if large else figs


def _check_block(call, b, k, go, vo, so, G, V, S, info, check_info, check_relative):
    ref, sig, bar = ref_of(b)
    s = S[so:so + b.n]
    assert not np.isnan(s).any(), (b.name, "S holds a NaN inside the block")
    if b.kind == "qrcp":
        out = G[go:go + b.m * b.n].reshape(b.n, b.m).T
        assert np.isfinite(out).all() and np.isfinite(s).all(), (b.name, "output not finite")
        dev = check_qrcp(b, out, s, ref, sig, bar)
    else:
        gp = G[go:go + b.m * b.n].reshape(b.n, b.m).T
        assert np.isfinite(gp).all() and np.isfinite(s).all(), (b.name, "output not finite")
        dev = check_plain(b, gp, s, V[vo:vo + b.n * b.n].reshape(b.n, b.n).T, ref, sig, bar)
    got = np.sort(s)[::-1]
    print(f"{call.name} / {b.name} {b.M.shape} {b.instance()}: |S - truth| / sigma_max {dev / sig if sig > 0 else dev:.3e}"
          f" (bar {bar:.3e}, numpy {numpy_deviation(b):.3e})  info {int(info[k])}")
    fig = (dev / sig if sig > 0 else dev, bar, got)
    if b.rank is not None:
        assert int((s > 1e-11 * sig).sum()) == b.rank, (b.name, "singular values above 1e-11 sigma_max", s, b.rank)
        if b.rank == 0:
            assert np.all(s == 0.0), (b.name, "S of an all-zero block", s)
    if b.diag is not None and check_relative:
        d = np.sort(b.diag)[::-1]
        print(f"{call.name} / {b.name}: S against the diagonal, worst {np.abs(got / d - 1).max() / EPS:.2f} eps (bar 4 eps)")
        assert np.all(np.abs(got - d) <= 4 * EPS * d), (b.name, "S of an already orthogonal block", np.abs(got / d - 1).max() / EPS)
    if check_info:
        assert int(info[k]) >= 0, (b.name, "not converged", int(info[k]))
        if b.n < 2:
            assert int(info[k]) == 0, (b.name, int(info[k]))
        elif b.rank is not None and (b.rank == 0 or (b.kind == "qrcp" and b.rank < 2)):
            pass        # nothing (rank 0) or a single column of R^H (rank 1 after the pivoted QR) to rotate: >= 0
        else:
            assert int(info[k]) >= 1, (b.name, int(info[k]))
        if b.diag is not None:
            assert int(info[k]) == 1, (b.name, "an already orthogonal block needs one sweep", int(info[k]))
    return fig


def scale_report(call, figs):
    """the blocks scaled by a power of two: is S / 2^p bit-identical to the unscaled block's S?  (printed, not asserted)"""
    for b in call.blocks:
        if b.scaled is not None:
            base, p = b.scaled
            same = same_bytes(np.ldexp(figs[b.name][2], -p), figs[base][2])
            print(f"{call.name} / {b.name}: S / 2^{p} bit-identical to {base}: {same}")


# ---- the cases -----------------------------------------------------------------------------------------------------------
def _graded_block(rng, name, kind, shape, acc=False):
    m, n = shape
    return Block(name, kind, with_spectrum(rng, m, n, graded_spectrum(min(m, n))), acc=acc)


# What every block of the shape calls is meant to run.  QRCP: (m0, n0) -> ("qrcp", GS, E, window, group size of qrcp_mgs);
# plain: (m, n) -> ("plain", GS, None, window).  GS x E are the 16 reachable instances of jacobi_dispatch_e -- 16 x 1..8,
# 32 x 5..8, 64 x 5..8 -- and jacobi_sweeps<16 | 32 | 64>; "lds" / "global" is where the rotated matrix lives.
_M0 = (3, 12, 17)           # m0 of the QRCP instance calls, cycling
EXPECT = {
    # every E of GS = 16, at its first and last n0 (E = 1: n0 = 1, 2 too: nothing / one pair to rotate)
    "qrcp_gs16": [((_M0[k % 3], n0), ("qrcp", 16, e, "lds", 16)) for k, (n0, e) in enumerate(
        [(1, 1), (2, 1), (15, 1), (16, 1), (17, 2), (32, 2), (33, 3), (48, 3), (49, 4), (64, 4), (65, 5), (80, 5), (81, 6),
         (96, 6), (97, 7), (112, 7), (113, 8), (128, 8)])],
    "qrcp_gs32": [((_M0[k % 3], n0), ("qrcp", 32, e, "lds", 16)) for k, (n0, e) in enumerate(
        [(129, 5), (160, 5), (161, 6), (192, 6), (193, 7), (224, 7), (225, 8), (256, 8)])],
    "qrcp_gs64": [((_M0[k % 3], n0), ("qrcp", 64, e, "lds", 16)) for k, (n0, e) in enumerate(
        [(257, 5), (320, 5), (321, 6), (384, 6), (385, 7), (448, 7), (449, 8), (512, 8)])],
    # X in the Vj workspace (global_* addressing of the same instances).  No block of E = 2 or E = 5 at GS = 16 can leave
    # the window (32 x 32, 80 x 80 < 9216): (96, 20) and (96, 80) run these two with r = 20 and 80 columns, in LDS
    "qrcp_global": [((96, 20), ("qrcp", 16, 2, "lds", 16)), ((96, 80), ("qrcp", 16, 5, "lds", 16)),
                    ((80, 128), ("qrcp", 16, 8, "global", 16)), ((40, 257), ("qrcp", 64, 5, "global", 16)),
                    ((19, 512), ("qrcp", 64, 8, "global", 16)), ((96, 97), ("qrcp", 16, 7, "global", 16))],
    # X exactly fills the window (96 x 96, 512 x 18 = 9216); qrcp_mgs<16 | 32 | 64> at m0 = 128 | 129, 256 | 257, 512
    "qrcp_edges": [((97, 96), ("qrcp", 16, 6, "lds", 16)), ((18, 512), ("qrcp", 64, 8, "lds", 16)),
                   ((128, 40), ("qrcp", 16, 3, "lds", 16)), ((129, 40), ("qrcp", 16, 3, "lds", 32)),
                   ((256, 40), ("qrcp", 16, 3, "lds", 32)), ((257, 40), ("qrcp", 16, 3, "lds", 64)),
                   ((512, 18), ("qrcp", 16, 2, "lds", 64))],
    # jacobi_sweeps<GS> at m = 128 | 129, 256 | 257, 511, 512 (512 x 18 fills the window); wide blocks (n - m zero
    # columns), odd n (a bye in every round), n < 2 (nothing to do)
    "plain_lds": [((128, 12), ("plain", 16, None, "lds")), ((129, 12), ("plain", 32, None, "lds")),
                  ((256, 12), ("plain", 32, None, "lds")), ((257, 12), ("plain", 64, None, "lds")),
                  ((511, 9), ("plain", 64, None, "lds")), ((512, 18), ("plain", 64, None, "lds")),
                  ((12, 30), ("plain", 16, None, "lds")), ((5, 12), ("plain", 16, None, "lds")),
                  ((300, 7), ("plain", 64, None, "lds")), ((1, 1), ("plain", 16, None, "lds")),
                  ((1, 3), ("plain", 16, None, "lds")), ((3, 1), ("plain", 16, None, "lds"))],
    # one column more than the window: rotated in global memory
    "plain_global": [((512, 19), ("plain", 64, None, "global")), ((300, 7), ("plain", 64, None, "lds"))],
}
SHAPE_CALLS = ("qrcp_gs16", "qrcp_gs32", "qrcp_gs64", "qrcp_global", "qrcp_edges", "plain_lds_acc", "plain_lds_noacc",
               "plain_global_acc", "plain_global_noacc")
# spectra, each on three carriers: plain 300 x 12 (jacobi_sweeps<64>, LDS), QRCP (12, 300) (jacobi_sweeps_pad<64, 5>, LDS),
# QRCP (40, 40) (jacobi_sweeps_pad<16, 3>, LDS).  None of the three can be above the window, so each runs once, with the
# host descriptors.
CARRIERS = (("p300x12", "plain", (300, 12)), ("q12x300", "qrcp", (12, 300)), ("q40x40", "qrcp", (40, 40)))
SPECTRUM_CALLS = ("graded", "multiplets", "cluster", "rank0", "rank1", "rank_half", "zero_columns", "orthogonal", "scaled",
                  "column_graded")
MULTIPLETS = [1.0] * 3 + [0.5] * 5 + [0.25] + [1e-3] * 3


def _build():
    calls = {}
    rng = np.random.default_rng(3101)
    for name in ("qrcp_gs16", "qrcp_gs32", "qrcp_gs64", "qrcp_edges", "qrcp_global"):
        blocks = [_graded_block(rng, f"{name}_{m0}x{n0}", "qrcp", (m0, n0)) for (m0, n0), _ in EXPECT[name]]
        calls[name] = Call(name, blocks, host=name != "qrcp_global")
    rng = np.random.default_rng(3102)
    for base, host in (("plain_lds", True), ("plain_global", False)):
        mats = [with_spectrum(rng, m, n, graded_spectrum(min(m, n))) for (m, n), _ in EXPECT[base]]
        for acc in (True, False):
            name = f"{base}_{'acc' if acc else 'noacc'}"
            calls[name] = Call(name, [Block(f"{name}_{M.shape[0]}x{M.shape[1]}", "plain", M, acc=acc) for M in mats], host)
            EXPECT[name] = EXPECT[base]
    for name in SHAPE_CALLS:
        got = [b.instance() for b in calls[name].blocks]
        want = [inst for _, inst in EXPECT[name]]
        assert got == want, f"{name}: instances {got}, meant for {want}"

    rng = np.random.default_rng(3103)

    def spectrum_call(name, make):
        blocks = []
        for cname, kind, shape in CARRIERS:
            blocks += make(f"{name}_{cname}", kind, shape)
        calls[name] = Call(name, blocks, host=True)

    def one(s_of, **kw):
        def make(name, kind, shape):
            rank = kw.get("rank_of")
            s = s_of(min(shape))
            return [Block(name, kind, with_spectrum(rng, shape[0], shape[1], s), acc=True,
                          rank=None if rank is None else len(s))]
        return make

    spectrum_call("graded", one(graded_spectrum))
    spectrum_call("multiplets", one(lambda k: MULTIPLETS))                           # rank 12 of 40 on the third carrier
    spectrum_call("cluster", one(lambda k: 1.0 + 1e-13 * np.arange(k)))
    spectrum_call("rank0", one(lambda k: [], rank_of=True))
    spectrum_call("rank1", one(lambda k: [1.0], rank_of=True))
    spectrum_call("rank_half", one(lambda k: graded_spectrum(k // 2, 8.0), rank_of=True))

    def zero_columns(name, kind, shape):
        M = with_spectrum(rng, shape[0], shape[1], graded_spectrum(min(shape), 8.0))
        cols = (3, shape[1] - 5)
        M[:, cols] = 0.0
        return [Block(name, kind, M, acc=True, rank=min(shape[0], shape[1] - 2))]
    spectrum_call("zero_columns", zero_columns)

    def orthogonal(name, kind, shape):
        if shape[0] < shape[1]:
            return []           # 300 orthogonal columns of 12 rows do not exist
        d = 1.0 / (1.0 + 0.37 * np.arange(shape[1]))
        return [Block(name, kind, orthogonal_columns(rng, shape[0], shape[1], d), acc=True, diag=d)]
    spectrum_call("orthogonal", orthogonal)

    def scaled(name, kind, shape):
        M = with_spectrum(rng, shape[0], shape[1], graded_spectrum(min(shape)))
        return [Block(name, kind, M, acc=True), Block(name + "_up", kind, np.ldexp(M.real, 100) + 1j * np.ldexp(M.imag, 100), acc=True, scaled=(name, 100)),
                Block(name + "_down", kind, np.ldexp(M.real, -100) + 1j * np.ldexp(M.imag, -100), acc=True, scaled=(name, -100))]
    spectrum_call("scaled", scaled)

    B = _rand(rng, 200, 12)
    B /= np.linalg.norm(B, axis=0)
    calls["column_graded"] = Call("column_graded", [Block("column_graded_p200x12", "plain", B * graded_spectrum(12), acc=True,
                                                          colgraded=True)], host=True)
    for c in calls.values():
        routes(c)
    names = [b.name for c in calls.values() for b in c.blocks]
    assert len(set(names)) == len(names)
    assert set(calls) == set(SHAPE_CALLS) | set(SPECTRUM_CALLS)
    return calls


CALLS = _build()


# ---- the staging copy of the same translation unit (k_batched_copy) -------------------------------------------------------
COPY_SHAPES = ((16, 16), (257, 1), (64, 64), (70, 61), (200, 250))      # 256, 257, 4096 (one trip of the grid), 4270, 50000 elements
COPY_CFG = ((abi.OP_N, 1, 1, 1), (abi.OP_N, 1, -1, 0), (abi.OP_C, 0, 0, 0), (abi.OP_C, 0, 0, 1), (abi.OP_N, 0, -1, 0),
            (abi.OP_C, 1, -1, 0))       # (op, gather_dim, scale_dim, inv_norm) of test_batched_copy_matches_numpy; the fifth without gather
COPY_GAP = 5


def copy_case():
    """-> (dst filled with NaN, src, idx, scl, items, spans of the items in dst): ten items, every shape twice and every
    configuration at least once; ldd = rows + 3; every item with inv_norm has one scale entry of exactly 0.0 that it uses"""
    rng = np.random.default_rng(77)
    items = np.zeros(2 * len(COPY_SHAPES), dtype=abi.COPY_DT)
    src, idx, scl, spans = [], [], [], []
    d_off = s_off = x_off = 0
    for k in range(len(items)):
        rows, cols = COPY_SHAPES[k % len(COPY_SHAPES)]
        op, gd, sd, inv = COPY_CFG[k % len(COPY_CFG)]
        gather = k % len(COPY_CFG) != 4
        s_rows, s_cols = (rows, cols) if op == abi.OP_N else (cols, rows)
        lds, big = s_rows + 2, max(rows, cols)
        src.append(rng.standard_normal(lds * s_cols) + 1j * rng.standard_normal(lds * s_cols))
        ix = rng.integers(0, rows if gd == 0 else cols, size=big).astype(np.int32)
        sc = rng.random(big) + 0.5
        if inv:
            pos = 1 if (rows if sd == 0 else cols) > 1 else 0
            sc[int(ix[pos]) if (gather and gd == sd) else pos] = 0.0
        idx.append(ix)
        scl.append(sc)
        it = items[k]
        it["dst_off"], it["src_off"], it["idx_off"], it["scl_off"] = d_off, s_off, (x_off if gather else -1), x_off
        it["rows"], it["cols"], it["ldd"], it["lds"] = rows, cols, rows + 3, lds
        it["op"], it["gather_dim"], it["scale_dim"], it["inv_norm"] = op, gd, sd, inv
        spans.append((d_off, rows, cols, rows + 3))
        d_off, s_off, x_off = d_off + (rows + 3) * cols + COPY_GAP, s_off + lds * s_cols, x_off + big
    dst = np.full(d_off, np.nan + 1j * np.nan)
    return dst, np.concatenate(src), np.concatenate(idx), np.concatenate(scl), items, spans


def check_copy(dst0, got, ref, items, spans):
    """got against ref (NumpyOps.batched_copy on the same NaN-filled dst) to 4 eps per element; what ref left NaN -- padding
    rows, gaps between items -- still holds dst0's bytes; every item with inv_norm holds exact zeros where ref does"""
    written = np.zeros(dst0.size, dtype=bool)
    for off, rows, cols, ldd in spans:
        for j in range(cols):
            written[off + j * ldd:off + j * ldd + rows] = True
    assert not np.isnan(ref[written]).any() and np.isnan(ref[~written].real).all()
    assert same_bytes(got[~written], dst0[~written]), "padding rows or gaps between the items were written"
    err = np.abs(got[written] - ref[written])
    worst = float((err / np.maximum(np.abs(ref[written]), np.finfo(np.float64).tiny)).max())
    print(f"batched copy: worst relative deviation {worst / EPS:.2f} eps over {int(written.sum())} elements")
    assert np.all(err <= 4 * EPS * np.abs(ref[written]))
    for it, (off, rows, cols, ldd) in zip(items, spans):
        if int(it["inv_norm"]):
            blk = ref[off:off + ldd * cols].reshape(cols, ldd).T[:rows]
            assert (blk == 0).any(), "the case lost its zero scale entry"
    return worst
