"""TEST INFRASTRUCTURE: what k steps of Lanczos MEAN, in extended precision, independent of how the kernels get there.

krylov_ritz(A, x0, k, Q) returns, for every j = 1..k, the lowest Ritz pair of P A P (P = 1 - Q^H Q for the frozen rows Q,
P = 1 without) on the Krylov space K_j(P A P, P x0).  These are properties of the SUBSPACE, not of a recurrence: an
orthonormal basis B is built by repeated modified Gram-Schmidt in numpy.clongdouble (80-bit on x86: eps = 1.1e-19) and
the lowest eigenpair of B^H A B is a float64 eigh refined by residual correction in the same precision.  numpy only.

The operator is a dense Hermitian float64 matrix, a callable on clongdouble vectors, or SylvesterOp(H, K):
X -> H X + X K^T on X[m, nc] stored column-major (vector index = i + m * j), the shape of the tests' grouped-GEMM stage,
which is never formed as a Kronecker matrix.  numpy multiplies long doubles with a plain triple loop (2.4 s for one
448 x 448 complex product); matmul_f64_ld() gets the same product out of float64 BLAS calls that are EXACT: the factors
are cut into slices of 21 mantissa bits (relative to the row / column maximum), so that a sum of up to 2048 slice products
fits the 53 bits of a double, and the slice products are added in long double.
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
EPS_LD = float(np.finfo(LD).eps)

_BITS = 21          # 2 * (21 + 1) + 11 <= 53: exact sums of up to 2048 products of two slices
_SLICES = 3


def _slices(A, axis):
    """float64 A -> ([S_1, S_2, S_3], R): A = sum S_i + R exactly; S_i holds at most _BITS + 1 leading bits (relative to the
    maximum of its row (axis = 1) or column (axis = 0)) of what the earlier slices left; |R| <= 2^-63 of that maximum"""
    R = np.array(A, dtype=np.float64)
    mu = np.abs(R).max(axis=axis, keepdims=True)
    e = np.where(mu > 0, np.ceil(np.log2(np.where(mu > 0, mu, 1.0))) + 1.0, 0.0)
    out = []
    for _ in range(_SLICES):
        sigma = np.ldexp(0.75, (e + 53 - _BITS).astype(np.int64))     # (R + sigma) - sigma rounds R to multiples of 2^(e - _BITS)
        S = (R + sigma) - sigma
        R = R - S                                                       # exact: S is R rounded to fewer bits
        out.append(S)
        e = e - _BITS
    return out, R


def _real_matmul_f64_ld(A, Xhi, Xlo):
    """A (float64) @ (Xhi + Xlo) with Xhi, Xlo float64, |Xlo| <= 2^-53 |Xhi|: long double result, error ~ 2^-63 |A| |X|"""
    assert A.shape[1] <= 2048
    As, Ar = _slices(A, 1)
    Xs, Xr = _slices(Xhi, 0)
    acc = np.zeros((A.shape[0], Xhi.shape[1]), dtype=LD)
    # smallest terms first; the remainders and Xlo are 2^-53 .. 2^-63 of the result, a float64 product is plenty for them
    acc += (A @ Xlo).astype(LD)
    acc += (Ar @ Xhi).astype(LD)
    acc += ((A - Ar) @ Xr).astype(LD)
    for s in range(2 * _SLICES - 2, -1, -1):
        for i in range(_SLICES):
            j = s - i
            if 0 <= j < _SLICES:
                acc += (As[i] @ Xs[j]).astype(LD)                       # exact in float64
    return acc


def matmul_f64_ld(A, X):
    """A @ X for a complex128 (or float64) matrix A and a clongdouble matrix X, to long double accuracy"""
    A = np.asarray(A)
    X = np.asarray(X, dtype=CLD)
    Ar, Ai = np.ascontiguousarray(A.real, dtype=np.float64), np.ascontiguousarray(A.imag, dtype=np.float64)
    parts = []
    for Xp in (X.real, X.imag):
        hi = np.ascontiguousarray(Xp, dtype=np.float64)
        lo = np.ascontiguousarray(Xp - hi.astype(LD), dtype=np.float64)
        parts.append((hi, lo))
    rr = _real_matmul_f64_ld(Ar, *parts[0])
    ri = _real_matmul_f64_ld(Ar, *parts[1])
    if np.iscomplexobj(A):
        ir = _real_matmul_f64_ld(Ai, *parts[0])
        ii = _real_matmul_f64_ld(Ai, *parts[1])
        return (rr - ii) + 1j * (ri + ir).astype(CLD)
    return rr + 1j * ri.astype(CLD)


class SylvesterOp:
    """x -> vec(H X + X K^T), X = x.reshape(nc, m).T (column-major m x nc); H, K Hermitian complex128"""

    def __init__(self, H, K):
        self.H, self.K = np.asarray(H, dtype=np.complex128), np.asarray(K, dtype=np.complex128)
        self.m, self.nc = self.H.shape[0], self.K.shape[0]
        self.n = self.m * self.nc

    def __call__(self, x):
        if x.dtype == np.complex128:
            X = x.reshape(self.nc, self.m).T
            return (self.H @ X + X @ self.K.T).T.reshape(-1)
        X = np.asarray(x, dtype=CLD).reshape(self.nc, self.m).T
        Y = matmul_f64_ld(self.H, X) + matmul_f64_ld(self.K, X.T).T
        return np.ascontiguousarray(Y.T).reshape(-1)

    def dense(self):
        return np.kron(np.eye(self.nc), self.H) + np.kron(self.K, np.eye(self.m))

    def norm_bound(self):
        """|A|_2 = max |eig H + eig K| (the summands commute)"""
        h, k = np.linalg.eigvalsh(self.H), np.linalg.eigvalsh(self.K)
        return float(max(abs(h[0] + k[0]), abs(h[-1] + k[-1])))


def as_operator(A):
    if callable(A):
        return A
    M = np.asarray(A)
    return lambda x: (M @ x) if x.dtype == np.complex128 else matmul_f64_ld(M, np.asarray(x, dtype=CLD)[:, None])[:, 0]


def _vdot(a, b):
    return (a.conj() * b).sum()


def _norm(a):
    return np.sqrt((a.real * a.real + a.imag * a.imag).sum())


def _mgs(w, rows, passes=2):
    """w minus its components along the orthonormal rows, one row at a time, `passes` times (long double)"""
    for _ in range(passes):
        for r in rows:
            w = w - r * _vdot(r, w)
    return w


def _lowest_eigpair_ld(G):
    """lowest eigenpair of the Hermitian clongdouble matrix G: float64 eigh, then residual correction in long double
    (y += sum_{i > 0} u_i <u_i, r> / (theta - w_i): every step gains the ~16 digits of the float64 eigenvectors)"""
    j = G.shape[0]
    w, U = np.linalg.eigh(np.asarray(G, dtype=np.complex128))
    U = U.astype(CLD)
    y = U[:, 0].copy()
    theta = LD(w[0])
    for _ in range(4):
        y = y / _norm(y)
        Gy = G @ y
        theta = _vdot(y, Gy).real
        r = Gy - theta * y
        if j == 1:
            break
        c = U[:, 1:].conj().T @ r
        y = y + U[:, 1:] @ (c / (theta - w[1:].astype(LD)))
    y = y / _norm(y)
    theta = _vdot(y, G @ y).real
    return theta, y


def krylov_ritz(A, x0, k, Q=None, ks=None, breakdown=1e-17, check=False):
    """-> dict: "theta"[j-1], "res"[j-1] (float64 arrays over j = 1..k_eff), "x" {j: complex128 unit Ritz vector} for j in ks
    (default: every j), "k_eff" (< k when the Krylov space is exhausted: |new vector| <= breakdown * max |A b|),
    "v0" (P x0 / |P x0|, complex128); with check: "ortho" / "orthoQ" (max |B^H B - 1| and max |Q B^H| of the reference basis).
    The phase of x_j is fixed by <v_0, x_j> > 0; res_j = |P (A x_j - theta_j x_j)|."""
    op = as_operator(A)
    n = len(x0)
    Qr = [] if Q is None else [np.asarray(q, dtype=CLD) for q in np.asarray(Q).reshape(-1, n)]
    if Qr:                                        # the frozen rows as given are orthonormal to float64 rounding only
        fixed = []
        for q in Qr:
            q = _mgs(q, fixed)
            fixed.append(q / _norm(q))
        Qr = fixed
    b = _mgs(np.asarray(x0, dtype=CLD), Qr)
    B = [b / _norm(b)]
    AB = []
    G = np.zeros((k, k), dtype=CLD)
    scale = LD(0)
    want = set(range(1, k + 1)) if ks is None else set(ks)
    out = {"theta": [], "res": [], "x": {}, "v0": np.asarray(B[0], dtype=np.complex128)}
    for j in range(1, k + 1):
        ab = op(B[j - 1])
        AB.append(ab)
        scale = max(scale, _norm(ab))
        for i in range(j):
            G[i, j - 1] = _vdot(B[i], ab)
            G[j - 1, i] = G[i, j - 1].conj()
        G[j - 1, j - 1] = G[j - 1, j - 1].real
        theta, y = _lowest_eigpair_ld(G[:j, :j])
        y = y * (y[0].conj() / abs(y[0]))         # <v_0, x_j> = y[0] > 0
        out["theta"].append(float(theta))
        out["res"].append(np.nan)                 # (only asked for where the vector is)
        if j in want:
            x = sum(B[i] * y[i] for i in range(j))
            r = _mgs(sum(AB[i] * y[i] for i in range(j)) - theta * x, Qr)
            out["res"][-1] = float(_norm(r))
            out["x"][j] = np.asarray(x, dtype=np.complex128)
        if j == k:
            break
        w = _mgs(ab, Qr + B, passes=2)            # (every pass over ALL rows: what a pass removes along B re-opens Q at its rounding)
        nw = _norm(w)
        if not nw > breakdown * scale:            # invariant subspace: the space cannot grow
            break
        B.append(w / nw)
    out["k_eff"] = len(out["theta"])
    out["theta"], out["res"] = np.array(out["theta"]), np.array(out["res"])
    if check:
        out["ortho"] = float(max(abs(_vdot(B[i], B[j]) - (i == j)) for i in range(len(B)) for j in range(i + 1)))
        out["orthoQ"] = float(max((abs(_vdot(q, b)) for q in Qr for b in B), default=0.0))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the operators of the Lanczos tests (tests/test_ref_krylov_cpu.py measures them, tests/test_krylov_steps_gpu.py uses them)
# ----------------------------------------------------------------------------------------------------------------------
EPS = float(np.finfo(np.float64).eps)
EDGE_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 256 * 667 + 1]
NF_LIST = [0, 1, 3, 8]
KMAX = 31


def rand_z(rng, n):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def factor(n):
    """n = m * nc with nc <= m as close to square as the divisors of n allow (a prime n: m = n, nc = 1)"""
    nc = max(d for d in range(1, int(np.sqrt(n)) + 1) if n % d == 0)
    return n // nc, nc


def make_operator(seed, m, nc, degenerate=False):
    """H (m x m), K (nc x nc) Hermitian: small random couplings on diagonals ~ sqrt(index) (the `_operator` of
    test_excited_gpu.py: the low end of the spectrum is well separated).  degenerate: the two lowest diagonal entries of K
    are equal and decoupled from the rest and from each other, so the lowest eigenvalue of H (x) 1 + 1 (x) K is double."""
    rng = np.random.default_rng(seed)
    H = 0.05 * rand_z(rng, m * m).reshape(m, m)
    H = H + H.conj().T + np.diag(10.0 * np.sqrt(np.linspace(0.0, 1.0, m)))
    K = 0.05 * rand_z(rng, nc * nc).reshape(nc, nc)
    K = K + K.conj().T + np.diag(3.0 * np.sqrt(np.linspace(0.0, 1.0, nc)))
    if degenerate:
        K[0:2, :] = 0.0
        K[:, 0:2] = 0.0
    return H, K


def random_rows(rng, nf, n):
    q, _ = np.linalg.qr(rand_z(rng, n * nf).reshape(n, nf))
    return np.ascontiguousarray(q.T)            # rows orthonormal: Q Q^H = 1


def sylvester_stages(ops, H, K, variant="one"):
    """the stage list of Y = H X + X K^T for ops.lanczos (buffers: 0 = x, 1 = y, 2 = H, 3 = K^T, 4 = side buffer Z):
    "one": one stage, two GEMM segments per tile; "empty_first": a stage without tiles, then the work;
    "two": Z = H X into the side buffer, then Y = Z (COPY segment) + X K^T"""
    from hubbardtn_amd import abi
    from ref_planner import TaskList
    m, nc = H.shape[0], K.shape[0]
    # column-major storage: H as H.T.reshape(-1); K^T as K.reshape(-1)
    bufs = [None, None, ops.to_device(H.T.reshape(-1).copy()), ops.to_device(K.reshape(-1).copy()), None] + [None] * 3

    def tl_hx(dst):
        tl = TaskList()
        tl.block(0, dst, 0, m, nc, m)
        tl.gemm(0, 2, 0, m, abi.OP_N, 0, 0, m, abi.OP_N, m, 1.0)          # H (buf 2) . X (buf 0)
        return tl

    def add_xk(tl):
        tl.gemm(0, 0, 0, m, abi.OP_N, 3, 0, nc, abi.OP_N, nc, 1.0)        # X (buf 0) . K^T (buf 3)
        return tl
    if variant == "two":
        bufs[4] = ops.zeros_z(m * nc)
        second = TaskList()
        second.block(0, 1, 0, m, nc, m)
        second.copy(0, 4, 0, m, 1.0)
        lists = [tl_hx(4), add_xk(second)]
    else:
        lists = [add_xk(tl_hx(1))]
        if variant == "empty_first":
            lists.insert(0, TaskList())
    return [(bufs, ops.upload_tasks(tl.finalize())) for tl in lists]


def bar(measured):
    """the allowance of the GPU tests for a figure whose float64-vs-reference deviation was `measured` on the CPU: same
    algorithm and conditioning, another summation order -- one decimal digit, and never below 256 eps"""
    return max(10.0 * measured, 256 * EPS)


# max over k (and over the nf of NF_LIST) of |theta_f64 - theta_ref| / |A|, |res_f64 - res_ref| / |A|, |x_f64 - x_ref|_2,
# NumpyOps.lanczos against krylov_ritz: measured by tests/test_ref_krylov_cpu.py (which fails if a fresh measurement
# exceeds twice the entry), never tuned against GPU output.  Keys: "n<size>".
F64_DEVIATION = {
    "n3000": (3.8e-16, 1.6e-16, 3.4e-15),
    "n200704": (2.4e-16, 1.6e-16, 6.1e-15),
    "n63": (8.0e-17, 4.2e-17, 1.1e-15),
    "n64": (1.2e-16, 6.7e-17, 1.1e-15),
    "n65": (5.8e-16, 1.1e-18, 1.0e-15),
    "n255": (9.2e-17, 3.3e-17, 1.2e-15),
    "n256": (1.4e-16, 2.5e-17, 1.9e-15),
    "n257": (2.3e-16, 5.8e-17, 1.2e-15),
    "n1023": (1.4e-16, 6.4e-17, 1.5e-15),
    "n1025": (6.5e-17, 3.3e-17, 1.1e-15),
    "n170753": (9.6e-17, 1.1e-16, 3.1e-15),
}
