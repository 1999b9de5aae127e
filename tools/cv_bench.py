"""What a correction-vector sweep costs at the headline size (a measurement tool, not part of bench.py).

Grows the state bench.py prepares (L = 64, U/t = 4, chi = 1024 by default: the same random start, growth schedule and warm-up
sweeps) and measures, in one process on one device:
  * one ground-state sweep() and its matvec count, for scale;
  * cv_sweep at z = E0 + 1.0 + 0.1i of x started from b = c+_{L/2} psi0 (truncdim chi, tol 1e-8, krylovdim 30), twice, with
    the matvec counts and the largest relative residual;
  * htn_krylov_combine2_z against the two htn_krylov_combine_z-style launches it replaces (X <- X + sum y V: the general axpy
    kernel; V[0] <- sum rho V: htn_krylov_combine_z) at the theta size of the centre bond, m = 30, HIP events, 200 repeats.
One JSON line at the end.

    python tools/cv_bench.py [--L 64] [--chi 1024] [--omega 1.0] [--eta 0.1] [--tol 1e-8] [--out profiles/cv_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def combine_bench(ops, n, m, reps=200):
    import torch
    rng = np.random.default_rng(5)
    V = ops.to_device(rng.standard_normal((m + 1) * n) + 1j * rng.standard_normal((m + 1) * n))
    X = ops.to_device(rng.standard_normal(n) + 1j * rng.standard_normal(n))
    y = (rng.standard_normal(m) + 1j * rng.standard_normal(m)) / m
    rho = (rng.standard_normal(m + 1) + 1j * rng.standard_normal(m + 1)) / m
    yd = ops.to_device(y)

    def fused():
        ops.krylov_combine2(V, n, m, y, rho, X, 1, n)

    def two():
        ops.axpys(X, V, n, m, yd, 1.0, n)
        ops.krylov_combine(V, n, m + 1, rho, n)

    out = {}
    for name, fn in (("combine2_us", fused), ("two_launches_us", two)):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name] = e0.elapsed_time(e1) * 1e3 / reps
    out["n"], out["m"] = n, m
    out["bytes_read_combine2"], out["bytes_read_two"] = (m + 2) * n * 16, (2 * m + 2) * n * 16
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--U", type=float, default=4.0)
    ap.add_argument("--chi", type=int, default=1024)
    ap.add_argument("--grow", type=str, default="16x8,32x4,64x4,128x2,256x2,512x2")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--omega", type=float, default=1.0)
    ap.add_argument("--eta", type=float, default=0.1)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    from hubbardtn_amd import api, engine, models, mps
    from hubbardtn_amd.device import HipOps
    ops = HipOps(0)
    L = args.L
    H = models.hamiltonian(models.OB_Sim([1.0], [args.U], 0.0, 1, 1, 2.0, 8), L)
    bonds, tens = mps.random_mps(L, (L, 0), 4, seed=1234)
    eng = engine.DMRG2(ops, H, bonds, tens, chi_full=16, lanczos_tol=1e-6)
    for item in [x for x in args.grow.split(",") if x]:
        chi, nsw = (int(v) for v in item.split("x"))
        if chi >= args.chi:
            continue
        eng.chi_full = chi
        for _ in range(nsw):
            eng.sweep()
    eng.chi_full = args.chi
    for _ in range(args.warmup):
        E = eng.sweep()
    print(f"grown: chi={args.chi} E/L={E / L:.12f}", file=sys.stderr)

    def timed(fn):
        ops.sync()
        t0 = time.perf_counter()
        r = fn()
        ops.sync()
        return time.perf_counter() - t0, r

    out = {"L": L, "chi": args.chi, "omega": args.omega, "eta": args.eta, "tol": args.tol}
    k0 = len(eng.stats)
    out["ground_sweep_s"], E0 = timed(eng.sweep)
    out["ground_sweep_matvecs"] = int(sum(s.n_matvec for s in eng.stats[k0:]))
    b = api.apply_operator(api.FiniteMPS(eng, L), "c+", L // 2).engine
    b.move_centre(0)
    x = b.copy()
    x.chi_full, x.cutoff, x.krylovdim, x.lanczos_tol, x.maxrestart = args.chi, 0.0, 30, args.tol, 50
    x.set_orthogonal([b])
    z = E0 + args.omega + 1j * args.eta
    for tag in ("first", "second"):
        k0 = len(x.stats)
        out[f"cv_sweep_{tag}_s"], (bx, amp) = timed(lambda: x.cv_sweep(z))
        st = x.stats[k0:]
        out[f"cv_sweep_{tag}_matvecs"] = int(sum(s.n_matvec for s in st))
        out[f"cv_sweep_{tag}_residual"] = float(max(s.residual for s in st))
        out[f"cv_sweep_{tag}_trunc_weight"] = float(max(s.trunc_weight for s in st))
        out[f"cv_sweep_{tag}_bx"] = [bx.real, bx.imag]
        out[f"cv_sweep_{tag}_amplitude"] = amp
    n = max(s.theta_size for s in x.stats)
    x.set_orthogonal([])
    out["combine"] = combine_bench(ops, int(n), 30)
    for k, v in out.items():
        print(f"{k}: {v}", file=sys.stderr)
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
