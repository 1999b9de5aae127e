"""The extended-precision Krylov reference (tests/ref_krylov.py) against the float64 numpy statement of the driver's own
algorithm (tests/emul.py: NumpyOps.lanczos stopped after k steps: tol = 0, max_restart = 0), for every k = 2..31 and
nf in {0, 1, 3, 8} frozen rows.  THIS IS WHERE THE BARS OF tests/test_krylov_steps_gpu.py COME FROM: the GPU kernels run
the same algorithm at the same conditioning with another summation order, and are allowed
max(10 x the deviation measured here, 256 eps); ref_krylov.F64_DEVIATION holds the measured figures and this file fails
when a fresh measurement exceeds twice its entry (or 1e-13: such an operator is replaced, the bar is not widened).

Measured (max over k and over nf; seeds as in CASES; |A| = the spectral norm of the operator):

    operator            |theta_f64 - theta_ref| / |A|   |res_f64 - res_ref| / |A|   |x_f64 - x_ref|_2
    n = 3000 (100 x 30)           3.8e-16                     1.6e-16                   3.4e-15
    n = 448 x 448                 2.4e-16                     1.6e-16                   6.1e-15
    n = 63                        8.0e-17                     4.2e-17                   1.1e-15
    n = 64                        1.2e-16                     6.7e-17                   1.1e-15
    n = 65                        5.8e-16                     1.1e-18                   1.0e-15
    n = 255                       9.2e-17                     3.3e-17                   1.2e-15
    n = 256                       1.4e-16                     2.5e-17                   1.9e-15
    n = 257                       2.3e-16                     5.8e-17                   1.2e-15
    n = 1023                      1.4e-16                     6.4e-17                   1.5e-15
    n = 1025                      6.5e-17                     3.3e-17                   1.1e-15
    n = 256 * 667 + 1             9.6e-17                     1.1e-16                   3.1e-15

`python tests/test_ref_krylov_cpu.py` prints the table afresh.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ref_krylov as rk                                   # noqa: E402
from emul import NumpyOps                                 # noqa: E402

# case -> (seed, m, nc, nf list, k list or None = every k in 2 .. 31 - nf)
CASES = {"n3000": (1, 100, 30, rk.NF_LIST, None), "n200704": (2, 448, 448, rk.NF_LIST, "thin")}
for _n in rk.EDGE_SIZES:
    if _n > rk.KMAX:
        CASES["n%d" % _n] = (100 + _n % 97, *rk.factor(_n), [0], [2, 9, 31])


def case_problem(case):
    """-> H, K, x0, {nf: Q}: the problem of a case, the same arrays in the CPU and the GPU tests"""
    seed, m, nc, nfs, _ = CASES[case]
    H, K = rk.make_operator(seed, m, nc)
    rng = np.random.default_rng(1000 + seed)
    x0 = rk.rand_z(rng, m * nc)
    Qs = {nf: (rk.random_rows(rng, nf, m * nc) if nf else None) for nf in nfs}
    return H, K, x0, Qs


def case_ks(case, nf):
    ks = CASES[case][4]
    if ks == "thin":
        return [2, 5, 17, rk.KMAX - nf]
    return list(range(2, rk.KMAX - nf + 1)) if ks is None else ks


def f64_steps(ops, stages, n, x0, k, Q=None):
    """NumpyOps.lanczos stopped after k steps -> theta, n_matvec, res, x with <v_0, x> > 0, record"""
    V = ops.zeros_z((k + 2) * n)
    V[0:n] = x0
    rec = {}
    theta, nmv, res = ops.lanczos(stages, 0, 1, V, n, k, 0.0, 0, frozen=Q, record=rec)
    x = V[0:n].copy()
    ov = np.vdot(rec["basis"][0], x)                      # (numpy's eigh leaves the sign of the Ritz coefficients open)
    return theta, nmv, res, x * (1.0 if ov.real >= 0 else -1.0), rec


def measure(case):
    H, K, x0, Qs = case_problem(case)
    op = rk.SylvesterOp(H, K)
    n, scale = op.n, op.norm_bound()
    ops = NumpyOps()
    stages = rk.sylvester_stages(ops, H, K)
    dev = np.zeros(3)
    for nf, Q in Qs.items():
        ks = case_ks(case, nf)
        ref = rk.krylov_ritz(op, x0, max(ks), Q, ks=ks, check=True)
        # the reference's own basis: an order of magnitude inside float64 rounding (sums of 2 * 10^5 long doubles)
        assert ref["k_eff"] == max(ks) and ref["ortho"] <= rk.EPS / 8 and ref["orthoQ"] <= rk.EPS / 8
        for k in ks:
            theta, nmv, res, x, rec = f64_steps(ops, stages, n, x0, k, Q)
            assert nmv == k and len(rec["alpha"]) == k and rec["basis"].shape == (k + 1, n)
            d = (abs(theta - ref["theta"][k - 1]) / scale, abs(res - ref["res"][k - 1]) / scale,
                 float(np.linalg.norm(x - ref["x"][k])))
            dev = np.maximum(dev, d)
    return dev


@pytest.mark.parametrize("case", list(CASES))
def test_float64_statement_agrees_with_the_reference(case):
    dev = measure(case)
    print(case, "theta %.2e res %.2e x %.2e" % tuple(dev), "recorded", rk.F64_DEVIATION[case])
    assert (dev <= 1e-13).all()                           # else: another operator, not a wider bar
    assert (dev <= 2 * np.maximum(np.array(rk.F64_DEVIATION[case]), rk.EPS)).all()


def test_recorded_basis_is_orthonormal_and_tridiagonalises():
    """record = {...}: alpha / beta / basis of NumpyOps.lanczos are those of the recurrence A V_k = V_k T_k + beta_k v_k e_k^T"""
    H, K, x0, Qs = case_problem("n3000")
    op, ops = rk.SylvesterOp(H, K), NumpyOps()
    for nf in (0, 3):
        k, Q = 17, Qs[nf]
        _, _, _, _, rec = f64_steps(ops, rk.sylvester_stages(ops, H, K), op.n, x0, k, Q)
        B = rec["basis"]
        assert np.abs(B.conj() @ B.T - np.eye(k + 1)).max() <= 64 * rk.EPS
        AB = np.array([op(b) for b in B[:k]])
        if Q is not None:
            assert np.abs(Q.conj() @ B.T).max() <= 64 * rk.EPS
            AB = AB - (AB @ Q.conj().T) @ Q
        T = np.diag(rec["alpha"]) + np.diag(rec["beta"][:-1], 1) + np.diag(rec["beta"][:-1], -1)
        R = AB - T @ B[:k]
        R[k - 1] -= rec["beta"][-1] * B[k]
        assert np.abs(R).max() <= 64 * rk.EPS * op.norm_bound()


def test_default_call_of_the_float64_statement_is_unchanged():
    """existing callers (no keyword) get what they got: same value, same count, same vector bits as frozen=None, record=None"""
    H, K, x0, _ = case_problem("n63")
    ops = NumpyOps()
    n = len(x0)
    outs = []
    for kw in ({}, {"frozen": None, "record": {}}, {"frozen": np.zeros((0, n), dtype=np.complex128)}):
        V = ops.zeros_z(12 * n)
        V[0:n] = x0
        outs.append((ops.lanczos(rk.sylvester_stages(ops, H, K), 0, 1, V, n, 10, 1e-10, 50, **kw), V[0:n].copy()))
    w = np.linalg.eigvalsh(rk.SylvesterOp(H, K).dense())
    assert abs(outs[0][0][0] - w[0]) <= 1e-9 * abs(w[-1])
    for o in outs[1:]:
        assert o[0] == outs[0][0] and np.array_equal(o[1], outs[0][1])


RESTART_TOL, RESTART_MAX = 1e-8, 4000


def restart_count(x0, kd, H, K):
    ops = NumpyOps()
    n = len(x0)
    V = ops.zeros_z((kd + 2) * n)
    V[0:n] = x0
    rec = {}
    theta, nmv, res = ops.lanczos(rk.sylvester_stages(ops, H, K), 0, 1, V, n, kd, RESTART_TOL, RESTART_MAX, record=rec)
    return theta, nmv, res, rec["stop"]


@pytest.mark.parametrize("kd", [2, 3, 5])
def test_restart_counts_do_not_hang_on_one_ulp(kd):
    """the GPU test asserts the matvec count of short restarted cycles against this statement: the count must not move
    under a one-ulp change of the start vector (else: another problem)"""
    H, K, x0, _ = case_problem("n3000")
    a = restart_count(x0, kd, H, K)
    b = restart_count(x0 * (1.0 + rk.EPS), kd, H, K)
    c = restart_count(x0 * (1.0 - rk.EPS / 2), kd, H, K)
    print("kd", kd, a[1:], b[1:], c[1:])
    assert a[2] < RESTART_TOL and a[1] == b[1] == c[1] and a[3] == b[3] == c[3]


def test_sliced_product_is_a_long_double_product():
    rng = np.random.default_rng(5)
    A = rk.rand_z(rng, 60 * 50).reshape(60, 50) * np.exp(6 * rng.standard_normal((60, 50)))
    X = (rk.rand_z(rng, 50 * 7).reshape(50, 7) * np.exp(6 * rng.standard_normal((50, 7)))).astype(rk.CLD)
    X = X + X * rk.LD(1e-17) * 3                           # bits below float64
    plain = A.astype(rk.CLD) @ X
    bound = (np.abs(A).astype(rk.LD) @ np.abs(X)) * rk.EPS_LD * (50 + 8)
    assert (np.abs(rk.matmul_f64_ld(A, X) - plain) <= bound).all()
    assert (np.abs(rk.matmul_f64_ld(A.real, X) - A.real.astype(rk.LD) @ X) <= bound).all()


def test_reference_against_dense_eigh_when_the_space_is_full():
    """k = n: the Krylov space is everything, the Ritz pair is the eigenpair; and an exhausted space stops the reference"""
    H, K = rk.make_operator(3, 4, 3)
    op = rk.SylvesterOp(H, K)
    A = op.dense()
    x0 = rk.rand_z(np.random.default_rng(4), 12)
    for arg in (op, A):
        ref = rk.krylov_ritz(arg, x0, 12)
        w, U = np.linalg.eigh(A)
        assert ref["k_eff"] == 12 and abs(ref["theta"][-1] - w[0]) <= 8 * rk.EPS * abs(w[-1]) and ref["res"][-1] <= 1e-16 * abs(w[-1])
        assert abs(abs(np.vdot(U[:, 0], ref["x"][12])) - 1) <= 64 * rk.EPS and np.vdot(ref["v0"], ref["x"][12]).real > 0
        assert (np.diff(ref["theta"]) <= 0).all()             # the lowest Ritz value of nested spaces never rises
    Q = rk.random_rows(np.random.default_rng(5), 3, 12)
    ref = rk.krylov_ritz(A, x0, 12, Q)                        # the complement of three rows has nine dimensions
    Bc = np.linalg.qr(Q.T, mode="complete")[0][:, 3:]
    assert ref["k_eff"] == 9 and abs(ref["theta"][-1] - np.linalg.eigvalsh(Bc.conj().T @ A @ Bc)[0]) <= 8 * rk.EPS * abs(w[-1])
    assert np.abs(Q.conj() @ ref["x"][9]).max() <= 8 * rk.EPS


if __name__ == "__main__":
    for c in CASES:
        print('    "%s": (%.1e, %.1e, %.1e),' % ((c,) + tuple(measure(c))), flush=True)
