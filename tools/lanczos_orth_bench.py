"""cost of the frozen rows of htn_lanczos_orth_z, measured, and of carrying attached states through a sweep.

Part 1 (kernel level): vectors of n = 200704 elements (the two-site tensor of a chi ~ 1000 bond), H_eff replaced by the
cheap two-segment operator of tests/test_excited_gpu.py so that the vector kernels dominate; tol = 0 makes every solve
run krylovdim x (max_restart + 1) steps.  Reported: wall time per Lanczos step for htn_lanczos_z and for
htn_lanczos_orth_z with n_frozen = 0, 1, 4, 8 (the difference to n_frozen = 0 is the price of the rows; the matvec is the
same in all of them).
Part 2 (engine level): L = 32, U/t = 4, chi = 256, profile mode (stages synchronised): seconds per sweep in the Lanczos
stage (which contains building and orthonormalising the projector rows) and in the environment stage (which contains moving
the overlap environments) with 0, 1 and 3 attached states."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                                             # noqa: E402
from hubbardtn_amd import engine, models, mps            # noqa: E402
from hubbardtn_amd.device import HipOps                  # noqa: E402
import test_excited_gpu as tx                            # noqa: E402


def kernel_part(ops, kd=23, restarts=3):
    rng = np.random.default_rng(1)
    m = nc = 448
    n = m * nc
    H, K, tasks = tx._operator(rng, m, nc)
    x0 = ops.to_device(tx._rand_z(rng, n))
    Q = ops.to_device(tx._random_rows(rng, 8, n).reshape(-1))
    stages = [([None, None, ops.to_device(H.T.reshape(-1).copy()), ops.to_device(K.reshape(-1).copy())] + [None] * 4,
               ops.upload_tasks(tasks))]
    V = ops.zeros_z((kd + 2) * n)
    rows = []
    for label, nf, plain in (("htn_lanczos_z", 0, True), ("orth nf=0", 0, False), ("orth nf=1", 1, False), ("orth nf=4", 4, False),
                             ("orth nf=8", 8, False)):
        best = None
        for rep in range(5):
            V[0:n] = x0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if plain:
                eig, nmv, res = ops.lanczos(stages, 0, 1, V, n, kd, 0.0, restarts)
            else:
                eig, nmv, res = ops.lanczos_orth(stages, 0, 1, V, n, kd, 0.0, restarts, Q, nf)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        rows.append((label, nmv, best))
    return rows


def engine_part(ops, L=32, chi=256):
    H = models.hamiltonian(models.OB_Sim([1.0], [4.0]), L)

    def state(seed, attach, sweeps, profile=False):
        bonds, tens = mps.random_mps(L, (L, 0), 8, seed=seed)
        eng = engine.DMRG2(ops, H, bonds, tens, chi_full=chi, krylovdim=20, lanczos_tol=1e-10)
        eng.set_orthogonal(attach)
        for _ in range(sweeps):
            eng.sweep()
        eng.profile = profile
        return eng
    found, out = [], []
    for na in (0, 1, 2, 3):
        eng = state(40 + na, found, 3)
        eng.profile = True
        eng.stats.clear()
        eng.sweep()
        st = eng.stats
        out.append((na, sum(s.t_lanczos for s in st), sum(s.t_env for s in st), sum(s.t_total for s in st), sum(s.n_matvec for s in st)))
        eng.profile = False
        found.append(eng)
    return out


if __name__ == "__main__":
    ops = HipOps(0)
    kernel_part(ops, restarts=0)          # warm-up: code objects, pools
    print("part 1: n = 200704, krylovdim 23, 4 cycles; best of 5; wall time of the library call")
    for label, nmv, dt in kernel_part(ops):
        print(f"  {label:14s} {nmv:4d} steps  {dt * 1e3:8.2f} ms  {dt / nmv * 1e6:7.1f} us per step")
    print("part 2: L = 32, chi = 256, one profiled sweep (61 bond updates) after 3 sweeps")
    for na, tl, te, tt, nmv in engine_part(ops):
        print(f"  attached {na}: lanczos stage {tl:.4f} s  env stage {te:.4f} s  total {tt:.4f} s  matvecs {nmv}")
