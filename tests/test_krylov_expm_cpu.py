"""htn_krylov_expm_z as the CPU baseline library exports it (the host statement of the method, htn::Backend::krylov_expm, on
host pointers): the cases and the accuracy gate of the GPU kernel test."""
import ctypes as C

import numpy as np

import krylov_expm_common as kc
from cpu_ops import CpuOps
from hubbardtn_amd import abi


def _solve(lib, p, kd, dt, tol, max_restart):
    n = p["n"]
    t = kc.tasks_for(n)
    tiles, segs = np.ascontiguousarray(t.tiles), np.ascontiguousarray(t.segs)
    Hf = np.ascontiguousarray(p["H"].T.reshape(-1))           # column major
    V = np.zeros((max(kd, 2) + 2) * n, dtype=np.complex128)
    V[:n] = p["x0"]
    arr = (abi.GemmLaunch * 1)()
    arr[0].bufs[2] = Hf.ctypes.data
    arr[0].tiles, arr[0].segs, arr[0].n_tiles = tiles.ctypes.data, segs.ctypes.data, t.ntiles
    g, a0, nmv, err = C.c_double(0.0), C.c_double(0.0), C.c_int32(0), C.c_double(0.0)
    dt = complex(dt)
    rc = lib.htn_krylov_expm_z(arr, 1, 0, 1, V.ctypes.data, n, kd, dt.real, dt.imag, tol, max_restart, None, 0, abi.EXCHANGE_FN(), None,
                               C.byref(g), C.byref(a0), C.byref(nmv), C.byref(err), None, None)
    abi.check(lib, rc, "htn_krylov_expm_z")
    return g.value, a0.value, nmv.value, err.value, V[:n].copy()


def test_cases_and_accuracy_gate_on_the_host_statement():
    lib = CpuOps().lib
    worst = {}
    kc.run_cases(lambda p, kd, dt, tol, mr: _solve(lib, p, kd, dt, tol, mr),
                 report=lambda name, ex, eg: worst.__setitem__(name, max(worst.get(name, 0.0), ex, eg)))
    print("largest error per case (CPU baseline library):", worst, "overall", max(worst.values()))


def test_tridiagonal_decisions_are_deterministic():
    lib = CpuOps().lib
    p = kc.problem("b")
    a = _solve(lib, p, p["kd"], p["dt"], kc.TOL, p["max_restart"])
    b = _solve(lib, p, p["kd"], p["dt"], kc.TOL, p["max_restart"])
    assert a[:4] == b[:4] and np.array_equal(a[4], b[4])
