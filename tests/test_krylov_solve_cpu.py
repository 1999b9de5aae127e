"""htn_krylov_solve_z as the CPU baseline library exports it (the host statement of the method, htn::Backend::krylov_solve, on
host pointers): the cases, the gates and the matvec counts of the GPU kernel test."""
import ctypes as C

import numpy as np

import krylov_solve_common as ks
from cpu_ops import CpuOps
from hubbardtn_amd import abi


def _solve(lib, p, kd, z, tol, max_restart, guess):
    n = p["n"]
    t = ks.tasks_for(n)
    tiles, segs = np.ascontiguousarray(t.tiles), np.ascontiguousarray(t.segs)
    Hf = np.ascontiguousarray(p["H"].T.reshape(-1))           # column major
    V = np.zeros((max(kd, 2) + 2) * n, dtype=np.complex128)
    V[:n] = p["b"]
    X = np.zeros(n, dtype=np.complex128)
    if guess is not None:
        X[:] = guess
    arr = (abi.GemmLaunch * 1)()
    arr[0].bufs[2] = Hf.ctypes.data
    arr[0].tiles, arr[0].segs, arr[0].n_tiles = tiles.ctypes.data, segs.ctypes.data, t.ntiles
    nrm, res, nmv = C.c_double(0.0), C.c_double(0.0), C.c_int32(0)
    z = complex(z)
    rc = lib.htn_krylov_solve_z(arr, 1, 0, 1, V.ctypes.data, n, kd, z.real, z.imag, tol, max_restart, X.ctypes.data,
                                1 if guess is not None else 0, None, 0, abi.EXCHANGE_FN(), None, C.byref(nrm), C.byref(res),
                                C.byref(nmv), None, None)
    abi.check(lib, rc, "htn_krylov_solve_z")
    return nrm.value, res.value, nmv.value, X.copy(), V[:n].copy()


def test_cases_gates_and_matvec_counts_on_the_host_statement():
    lib = CpuOps().lib
    ks.run_cases(lambda p, kd, z, tol, mr, guess: _solve(lib, p, kd, z, tol, mr, guess))


def test_the_numpy_model_solves_the_cases():
    for name in "abdf":
        p = ks.problem(name)
        x = ks.model_of(name)[0]
        assert np.linalg.norm(p["b"] - (p["z"] * x - p["H"] @ x)) <= ks.GATE * np.linalg.norm(p["b"]), name


def test_decisions_are_deterministic():
    lib = CpuOps().lib
    p = ks.problem("b")
    a = _solve(lib, p, p["kd"], p["z"], ks.TOL, p["max_restart"], None)
    b = _solve(lib, p, p["kd"], p["z"], ks.TOL, p["max_restart"], None)
    assert a[:3] == b[:3] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
