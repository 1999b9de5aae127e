"""htn_krylov_solve_z and htn_krylov_combine2_z on the MI355X: (z - H) x = b for a dense Hermitian H fed as one grouped-GEMM stage
against numpy.linalg.solve (cases, gates and the model's matvec counts: tests/krylov_solve_common.py); the combine launch
against numpy."""
import numpy as np
import pytest

import krylov_solve_common as ks

pytestmark = pytest.mark.gpu


def _stages(hip_ops, p):
    Hd = hip_ops.to_device(np.ascontiguousarray(p["H"].T.reshape(-1)))
    return [([None, None, Hd] + [None] * 5, hip_ops.upload_tasks(ks.tasks_for(p["n"])))]


def _solve(hip_ops, p, kd, z, tol, max_restart, guess):
    n = p["n"]
    V = hip_ops.zeros_z((max(kd, 2) + 2) * n)
    V[0:n] = hip_ops.to_device(p["b"])
    X = hip_ops.zeros_z(n) if guess is None else hip_ops.to_device(np.ascontiguousarray(guess))
    nrm, res, nmv = hip_ops.krylov_solve(_stages(hip_ops, p), 0, 1, V, n, kd, z, tol, max_restart, X, use_guess=guess is not None)
    return nrm, res, nmv, hip_ops.to_host(X), hip_ops.to_host(V[0:n])


def test_cases_gates_and_matvec_counts(hip_ops):
    ks.run_cases(lambda p, kd, z, tol, mr, guess: _solve(hip_ops, p, kd, z, tol, mr, guess), speculative=1)


def test_two_calls_give_identical_bits(hip_ops):
    p = ks.problem("d")
    a = _solve(hip_ops, p, p["kd"], p["z"], ks.TOL, p["max_restart"], None)
    b = _solve(hip_ops, p, p["kd"], p["z"], ks.TOL, p["max_restart"], None)
    assert a[:3] == b[:3] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


@pytest.mark.parametrize("n", [1, 3, 257, 4099])
def test_combine2_kernel_against_numpy(hip_ops, n):
    """htn_krylov_combine2_z: m = 1, 2, 5, 31 (rho has m + 1 <= 32 entries: the compile-time row counts 4, 8 and 32 and their
    edges), keep 0 / 1, with and without rho, ldv > n; element-wise to the rounding bound of the sums, 4 eps sum |c_i| |V_i|;
    rows 1.. and the padding behind every row stay bit-identical, and without rho row 0 does too"""
    rng = np.random.default_rng(n)
    eps = np.finfo(float).eps
    ldv = n + 5
    for m in (1, 2, 5, 31):
        for keep in (0, 1):
            for with_rho in (False, True):
                Vh = ks.rand_z(rng, (m + 1) * ldv)
                Xh = ks.rand_z(rng, n + 3)
                y, rho = ks.rand_z(rng, m), ks.rand_z(rng, m + 1)
                V, X = hip_ops.to_device(Vh), hip_ops.to_device(Xh)
                hip_ops.krylov_combine2(V, ldv, m, y, rho if with_rho else None, X, keep, n)
                gv, gx = hip_ops.to_host(V), hip_ops.to_host(X)
                rows = Vh.reshape(m + 1, ldv)[:, :n]
                want_x = (Xh[:n] if keep else 0.0) + y @ rows[:m]
                bound_x = (np.abs(Xh[:n]) if keep else 0.0) + np.abs(y) @ np.abs(rows[:m])
                assert np.all(np.abs(gx[:n] - want_x) <= 4 * eps * bound_x), (m, keep, with_rho)
                assert np.array_equal(gx[n:], Xh[n:])
                if with_rho:
                    assert np.all(np.abs(gv[:n] - rho @ rows) <= 4 * eps * (np.abs(rho) @ np.abs(rows))), (m, keep)
                    assert np.array_equal(gv[n:], Vh[n:]), (m, keep)
                else:
                    assert np.array_equal(gv, Vh), (m, keep)
    for bad in (0, 32):
        with pytest.raises(Exception, match="m must be"):
            hip_ops.krylov_combine2(hip_ops.zeros_z(64), 1, bad, np.zeros(bad, dtype=complex), None, hip_ops.zeros_z(4), 0, 1)
