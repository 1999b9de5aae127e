"""htn_krylov_expm_z on the MI355X: x = exp(-i dt H) x0 for a dense Hermitian H fed as one grouped-GEMM stage, against eigh
(cases and gate: tests/krylov_expm_common.py); determinism; and a solver call after an exponential on the same stream."""
import numpy as np
import pytest

import krylov_expm_common as kc

pytestmark = pytest.mark.gpu


def _stages(hip_ops, p):
    Hd = hip_ops.to_device(np.ascontiguousarray(p["H"].T.reshape(-1)))
    return [([None, None, Hd] + [None] * 5, hip_ops.upload_tasks(kc.tasks_for(p["n"])))]


def _solve(hip_ops, p, kd, dt, tol, max_restart):
    n = p["n"]
    V = hip_ops.zeros_z((max(kd, 2) + 2) * n)
    V[0:n] = hip_ops.to_device(p["x0"])
    g, a0, nmv, err = hip_ops.krylov_expm(_stages(hip_ops, p), 0, 1, V, n, kd, dt, tol, max_restart)
    return g, a0, nmv, err, hip_ops.to_host(V[0:n])


def test_cases_and_accuracy_gate(hip_ops):
    worst = {}
    kc.run_cases(lambda p, kd, dt, tol, mr: _solve(hip_ops, p, kd, dt, tol, mr),
                 report=lambda name, ex, eg: worst.__setitem__(name, max(worst.get(name, 0.0), ex, eg)), speculative=1)
    print("largest error per case (MI355X):", worst, "overall", max(worst.values()))


def test_two_calls_give_identical_bits(hip_ops):
    for name in "abd":
        p = kc.problem(name)
        a = _solve(hip_ops, p, p["kd"], p["dt"], 1e-8, p["max_restart"])        # (1e-8: case b in fewer sub-steps)
        b = _solve(hip_ops, p, p["kd"], p["dt"], 1e-8, p["max_restart"])
        assert a[:4] == b[:4] and np.array_equal(a[4], b[4]), name


def test_solver_after_an_exponential_on_the_same_stream_is_unchanged(hip_ops):
    """the drivers share the per-stream records, events and serial numbers: htn_lanczos_z gives the same bits whether or not
    an exponential (one that ends on a speculative step, and one that restarts) ran before it"""
    p = kc.problem("b")
    n = p["n"]
    st = _stages(hip_ops, p)

    def lanczos():
        V = hip_ops.zeros_z(22 * n)
        V[0:n] = hip_ops.to_device(p["x0"])
        out = hip_ops.lanczos(st, 0, 1, V, n, 20, 1e-10, 5)
        return out, hip_ops.to_host(V[0:n])
    ref = lanczos()
    for name in "ab":
        q = kc.problem(name)
        _solve(hip_ops, q, q["kd"], q["dt"], 1e-8, q["max_restart"])
        got = lanczos()
        assert got[0] == ref[0] and np.array_equal(got[1], ref[1]), name


@pytest.mark.parametrize("n", [1, 1000, 262145 + 3])
def test_combine_kernel_against_numpy(hip_ops, n):
    """htn_krylov_combine_z: every compile-time row count (steps of four) and its edges, n = 1, n no multiple of the block, and
    n beyond one pass of the grid (1024 blocks x 256 threads); rows 1.. and the padding behind a row (ldv > n) stay untouched"""
    rng = np.random.default_rng(n)
    ldv = n + 5
    for m in ((5, 32) if n > 100000 else (1, 2, 4, 5, 8, 9, 13, 17, 21, 25, 29, 31, 32)):
        Vh = kc.rand_z(rng, m * ldv)
        c = kc.rand_z(rng, m)
        V = hip_ops.to_device(Vh)
        hip_ops.krylov_combine(V, ldv, m, c, n)
        got = hip_ops.to_host(V)
        rows = Vh.reshape(m, ldv)
        want = c @ rows[:, :n]
        scale = np.abs(c) @ np.abs(rows[:, :n])
        assert np.all(np.abs(got[:n] - want) <= 8 * m * np.finfo(float).eps * scale), m     # a sum of m products, any order
        assert np.array_equal(got[n:], Vh[n:]), m
    for bad in (0, 33):
        with pytest.raises(Exception, match="nvec"):
            hip_ops.krylov_combine(hip_ops.zeros_z(64), 1, bad, np.zeros(bad, dtype=complex), 1)
