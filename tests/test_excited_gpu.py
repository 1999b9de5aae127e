"""Excited states on the MI355X: the Lanczos kernels with frozen rows (htn_lanczos_orth_z) against dense linear algebra,
the orthogonalised sweep on the HIP backend against exact diagonalisation and against the CPU baseline library's host
statement of the same method, and a chain length where only size-independent facts can be asserted."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):          # (the file is also run as a script: the child process of the last test)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import excited_common as xc                              # noqa: E402
from hubbardtn_amd import abi, engine, models, mps       # noqa: E402
from ref_planner import TaskList                         # noqa: E402

pytestmark = pytest.mark.gpu


def _rand_z(rng, n):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def _operator(rng, m, nc):
    """Y = H X + X K^T on X[m, nc]: one grouped-GEMM stage, two segments per tile.  Diagonals ~ sqrt(index) make the low
    end of the spectrum well separated (a restarted Lanczos of dimension 23 converges in a few cycles)."""
    H = 0.05 * _rand_z(rng, m * m).reshape(m, m)
    H = H + H.conj().T + np.diag(10.0 * np.sqrt(np.linspace(0.0, 1.0, m)))
    K = 0.05 * _rand_z(rng, nc * nc).reshape(nc, nc)
    K = K + K.conj().T + np.diag(3.0 * np.sqrt(np.linspace(0.0, 1.0, nc)))
    tl = TaskList()
    tl.block(0, 1, 0, m, nc, m)
    tl.gemm(0, 2, 0, m, abi.OP_N, 0, 0, m, abi.OP_N, m, 1.0)          # H (buf 2) . X (buf 0)
    tl.gemm(0, 0, 0, m, abi.OP_N, 3, 0, nc, abi.OP_N, nc, 1.0)        # X (buf 0) . K^T (buf 3)
    return H, K, tl.finalize()


def _solve(hip_ops, H, K, tasks, x0, kd, tol, max_restart, Q=None, nf=0, plain=False):
    m, nc = H.shape[0], K.shape[0]
    n = m * nc
    V = hip_ops.zeros_z((kd + 2) * n)
    V[0:n] = hip_ops.to_device(x0)
    # column-major storage: H as H.T.reshape(-1); K^T as K.reshape(-1)
    stages = [([None, None, hip_ops.to_device(H.T.reshape(-1).copy()), hip_ops.to_device(K.reshape(-1).copy())] + [None] * 4,
               hip_ops.upload_tasks(tasks))]
    if plain:
        eig, nmv, res = hip_ops.lanczos(stages, 0, 1, V, n, kd, tol, max_restart)
    else:
        Qd = None if Q is None else hip_ops.to_device(np.ascontiguousarray(Q).reshape(-1))
        eig, nmv, res = hip_ops.lanczos_orth(stages, 0, 1, V, n, kd, tol, max_restart, Qd, nf)
    return eig, nmv, res, hip_ops.to_host(V[0:n])


def _random_rows(rng, nf, n):
    q, _ = np.linalg.qr(_rand_z(rng, n * nf).reshape(n, nf))
    return np.ascontiguousarray(q.T)            # rows orthonormal: Q Q^H = 1


def test_frozen_rows_small_against_dense(hip_ops):
    """n = 3000: the eigenvalue of P A P on the complement of Q (dense, numpy) at the Lanczos tolerance, |Q^H x| <= 1e-12;
    Q = the lowest eigenvectors -> the next eigenvalue"""
    rng = np.random.default_rng(61)
    m, nc, kd, tol = 100, 30, 23, 1e-10
    H, K, tasks = _operator(rng, m, nc)
    n = m * nc
    A = np.kron(np.eye(nc), H) + np.kron(K, np.eye(m))
    w, U = np.linalg.eigh(A)
    scale = max(abs(w[0]), abs(w[-1]))
    x0 = _rand_z(rng, n)
    for nf in (1, 3, 8):
        Q = _random_rows(rng, nf, n)
        # the frozen vectors are the stored rows f_r = Q[r] (<f_r, x> = sum conj(Q[r]) x): columns of Q^T
        Bc = np.linalg.qr(Q.T, mode="complete")[0][:, nf:]                 # orthonormal basis of their complement
        ref = np.linalg.eigvalsh(Bc.conj().T @ A @ Bc)[0]
        eig, nmv, res, x = _solve(hip_ops, H, K, tasks, x0, kd, tol, 60, Q, nf)
        print("random Q", nf, "eig", eig, "ref", ref, "matvecs", nmv, "res", res, "|Q^H x|", np.linalg.norm(Q.conj() @ x))
        assert res < tol
        assert abs(eig - ref) <= tol * scale
        assert np.linalg.norm(Q.conj() @ x) <= 1e-12 and abs(np.linalg.norm(x) - 1.0) <= 1e-12
        Ql = np.ascontiguousarray(U[:, :nf].T)                             # frozen vectors = the lowest eigenvectors
        eig, nmv, res, x = _solve(hip_ops, H, K, tasks, x0, kd, tol, 60, Ql, nf)
        print("lowest eigenvectors", nf, "eig", eig, "next", w[nf], "matvecs", nmv, "res", res)
        assert abs(eig - w[nf]) <= tol * scale
        assert np.linalg.norm(Ql.conj() @ x) <= 1e-12


def test_frozen_rows_large_stay_orthogonal(hip_ops):
    """n = 200704 (the size of a chi ~ 1000 two-site tensor): |Q^H x| <= 1e-12 and the eigenvalue is the Rayleigh quotient
    of the returned vector"""
    rng = np.random.default_rng(62)
    m = nc = 448
    H, K, tasks = _operator(rng, m, nc)
    n = m * nc
    x0 = _rand_z(rng, n)
    for nf in (1, 3, 8):
        Q = _random_rows(rng, nf, n)
        eig, nmv, res, x = _solve(hip_ops, H, K, tasks, x0, 23, 1e-8, 6, Q, nf)
        X = x.reshape(nc, m).T
        rq = np.vdot(X, H @ X + X @ K.T).real
        print("n", n, "nf", nf, "eig", eig, "rayleigh", rq, "matvecs", nmv, "res", res, "|Q^H x|", np.linalg.norm(Q.conj() @ x))
        assert np.linalg.norm(Q.conj() @ x) <= 1e-12 and abs(np.linalg.norm(x) - 1.0) <= 1e-12
        assert abs(eig - rq) <= 1e-10 * max(abs(rq), 1.0)


@pytest.mark.parametrize("m,nc", [(100, 30), (448, 448)])
def test_no_frozen_rows_is_htn_lanczos_z_bit_for_bit(hip_ops, m, nc):
    rng = np.random.default_rng(63)
    H, K, tasks = _operator(rng, m, nc)
    x0 = _rand_z(rng, m * nc)
    a = _solve(hip_ops, H, K, tasks, x0, 23, 1e-9, 4, plain=True)
    b = _solve(hip_ops, H, K, tasks, x0, 23, 1e-9, 4, None, 0)
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3])


def test_row_limit_fails_loudly(hip_ops):
    rng = np.random.default_rng(64)
    H, K, tasks = _operator(rng, 40, 4)
    Q = _random_rows(rng, 9, 160)
    with pytest.raises(abi.HtnError, match="krylovdim \\+ n_frozen <= 31"):
        _solve(hip_ops, H, K, tasks, _rand_z(rng, 160), 23, 1e-9, 2, Q, 9)


@pytest.mark.parametrize("pset", [0, 1])
def test_hip_engine_levels_against_ed_and_the_cpu_statement(hip_ops, pset):
    """the cases of test_excited_cpu.py on the HIP backend: every level against ED to 1e-8; against the CPU baseline library
    from the same starts: energies to 1e-8, matvec counts per bond within the allowance of tests/test_fullsize_gpu.py (the
    product counts the speculatively enqueued step of every restart cycle, and one step either way for a residual that
    meets the tolerance within rounding)"""
    from cpu_ops import CpuOps
    t, u = xc.PARAMS[pset]
    ref = xc.ed_levels(8, t, u)
    cpu = CpuOps()
    got = {}
    for tgt, n in xc.CASES:
        hs, hE = xc.sector_states(hip_ops, 8, t, u, tgt, n)
        cs, cE = xc.sector_states(cpu, 8, t, u, tgt, n)
        got[tgt] = hE
        for k in range(n):
            assert len(hs[k].stats) == len(cs[k].stats)
            for a, b in zip(hs[k].stats, cs[k].stats):
                cycles = -(-b.n_matvec // 20)
                print(tgt, k, "bond", a.bond, a.direction, "E", a.energy, b.energy, "matvecs", a.n_matvec, b.n_matvec)
                assert abs(a.energy - b.energy) <= 1e-8 * max(abs(b.energy), 1.0)
                assert -1 <= a.n_matvec - b.n_matvec <= cycles + 1
        for j in range(n):
            for k in range(j):
                assert abs(hs[j].overlap(hs[k])) <= 1e-10
    xc.compare_levels(got, ref)


def test_hip_truncated_states_stay_orthogonal_within_the_truncation(hip_ops):
    L = 16
    states, _ = xc.sector_states(hip_ops, L, [1.0], [4.0], (L, 0), 3, chi_full=60, sweeps=4)
    for j in range(3):
        tw = sum(s.trunc_weight for s in states[j].stats[-(2 * L - 3):])
        for k in range(j):
            ov = abs(states[j].overlap(states[k]))
            print("truncated", j, k, ov, "bound", np.sqrt(2 * tw) + 1e-10)
            assert ov <= np.sqrt(2 * tw) + 1e-10


def run_l32():
    """L = 32, U/t = 4, chi grown to 256: ground state, first excited singlet, lowest triplet, N +- 1 -> plain JSON-able dict"""
    from hubbardtn_amd.device import HipOps
    ops = HipOps(0)
    L, t, u = 32, [1.0], [4.0]
    H = models.hamiltonian(models.OB_Sim(t, u), L)

    def run(target, attach, seed):
        bonds, tens = mps.random_mps(L, target, 8, seed=seed)
        eng = engine.DMRG2(ops, H, bonds, tens, chi_full=64, krylovdim=20, lanczos_tol=1e-10)
        eng.set_orthogonal(attach)
        for chi, nsw in ((64, 2), (128, 2), (256, 2)):
            eng.chi_full = chi
            for _ in range(nsw):
                E = eng.sweep()
        tw = sum(s.trunc_weight for s in eng.stats[-(2 * L - 3):])
        return eng, float(E), float(tw)
    g, E0, tw0 = run((L, 0), [], 5)
    x, E1, tw1 = run((L, 0), [g], 6)
    tr, Et, _ = run((L, 2), [], 7)
    _, Ep, _ = run((L + 1, 1), [], 8)
    _, Em, _ = run((L - 1, 1), [], 9)
    ov = x.overlap(g)
    return {"E0": E0.hex(), "E1": E1.hex(), "Et": Et.hex(), "Ep": Ep.hex(), "Em": Em.hex(), "tw1": tw1.hex(),
            "ov": [float(ov.real).hex(), float(ov.imag).hex()]}


def test_l32_size_independent_facts_and_poison_bits(hip_ops):
    """no ED at L = 32: variational order inside the sector, the overlap within the truncation bound, spin gap > 0, charge
    gap > spin gap (half filling: gapless spin sector with an O(1/L) finite-size gap, the Mott gap on top), and the same bits
    from a child process whose device pool hands out NaN-filled blocks (HTN_DEBUG_POISON=1, pattern of test_debug_gpu.py)"""
    r = run_l32()
    f = {k: float.fromhex(v) for k, v in r.items() if k != "ov"}
    ov = abs(complex(float.fromhex(r["ov"][0]), float.fromhex(r["ov"][1])))
    spin_gap, charge_gap = f["Et"] - f["E0"], f["Ep"] + f["Em"] - 2 * f["E0"]
    print("E0", f["E0"], "E1 - E0", f["E1"] - f["E0"], "spin gap", spin_gap, "charge gap", charge_gap, "overlap", ov,
          "bound", np.sqrt(2 * f["tw1"]) + 1e-10)
    assert f["E1"] - f["E0"] >= -1e-8 * abs(f["E0"])
    assert ov <= np.sqrt(2 * f["tw1"]) + 1e-10
    assert spin_gap > 0 and charge_gap > spin_gap
    env = dict(os.environ, HTN_DEBUG_POISON="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == r


if __name__ == "__main__":
    print(json.dumps(run_l32()))
