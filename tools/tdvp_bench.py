"""One two-site TDVP sweep beside one ground-state sweep from the same state (a measurement tool, not part of bench.py).

Grows the headline state the way bench.py does (L = 64, U/t = 4, chi = 1024 by default: the same random start, growth schedule
and warm-up sweeps), downloads it, and times tdvp_sweep(dt) (htn_tdvp2_sweep: 2L-2 bond exponentials + 2L-4 backward one-site
exponentials) and sweep() (htn_dmrg2_sweep: 2L-3 eigen-solves) from two engines built on those tensors.  Prints both times,
both matvec counts, the seconds per matvec of each and the stage split of a profiled sweep each (stages bracketed by stream
syncs, which perturbs the total).

Then the tail of one solve at a given vector length n and basis size m, HIP events around a batch of repeats: the ONE launch of
the exponential (htn_krylov_combine_z) against the five stream operations with which the eigen-solver assembles its Ritz vector
-- H2D copy of the coefficients from pinned memory, memset of the scratch row, k_axpys (htn_axpys_z), the squared norm, the scaling
into row 0 (htn_scale_inv_sqrt_z).  The norm is taken by htn_dots_z here (partial sums + a one-block reduction: two small kernels)
where the solver's k_norm_partial / k_scale_by_norm pair reduces inside the scaling kernel: the stand-in has one tiny launch more.
The solver's two host drains per tail are outside the events and not counted.  One JSON line at the end.

    python tools/tdvp_bench.py [--L 64] [--chi 1024] [--dt 0.05] [--tol 1e-10] [--sweeps 2] [--tail-n 200704] [--tail-m 8,16,30]
    python tools/tdvp_bench.py --tail-only
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def tail_bench(ops, n, m, reps=200):
    """-> (ms per combine launch, ms per five-operation Ritz tail) at vector length n, m basis rows"""
    import numpy as np
    torch = ops.torch
    rng = np.random.default_rng(5)
    V = ops.to_device((rng.standard_normal((m + 2) * n) + 1j * rng.standard_normal((m + 2) * n)) / np.sqrt(2.0 * n))
    c = rng.standard_normal(m) + 1j * rng.standard_normal(m)
    c /= np.linalg.norm(c)
    h_y = torch.from_numpy(c.copy()).pin_memory()
    ycoef, nrm = ops.zeros_z(m), ops.zeros_z(1)
    xrow = V[(m + 1) * n:(m + 2) * n]

    def combine():
        ops.krylov_combine(V, n, m, c, n)

    def ritz():
        ycoef.copy_(h_y, non_blocking=True)
        xrow.zero_()
        ops.axpys(xrow, V, n, m, ycoef, 1.0, n)
        ops.dots(xrow, n, 1, xrow, n, nrm)
        ops.scale_inv_sqrt(V, xrow, nrm, n)

    out = []
    for fn in (combine, ritz):
        for _ in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ops.sync()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out[0], out[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--U", type=float, default=4.0)
    ap.add_argument("--chi", type=int, default=1024)
    ap.add_argument("--grow", type=str, default="16x8,32x4,64x4,128x2,256x2,512x2")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sweeps", type=int, default=2)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--tail-n", type=int, default=200704)
    ap.add_argument("--tail-m", type=str, default="8,16,30")
    ap.add_argument("--tail-only", action="store_true")
    args = ap.parse_args()
    from hubbardtn_amd import engine, models, mps
    from hubbardtn_amd.device import HipOps
    ops = HipOps(0)
    tails = []
    for m in [int(x) for x in args.tail_m.split(",") if x]:
        t_c, t_r = tail_bench(ops, args.tail_n, m)
        print(f"tail n={args.tail_n} m={m}: combine {1e3 * t_c:.2f} us  five-operation Ritz tail {1e3 * t_r:.2f} us", file=sys.stderr)
        tails.append({"n": args.tail_n, "m": m, "combine_us": 1e3 * t_c, "ritz_tail_us": 1e3 * t_r})
    if args.tail_only:
        print(json.dumps({"tails": tails}))
        return
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
    eng.chi_full, eng.lanczos_tol = args.chi, args.tol
    for _ in range(args.warmup):
        E = eng.sweep()
    print(f"grown: chi={args.chi} E/L={E / L:.12f} max bond dim {max(eng.bond_dims())}", file=sys.stderr)
    tables = [dict(b.dims) for b in eng.bonds]
    sites = [eng.download_site(i) for i in range(L)]

    def fresh():
        return engine.DMRG2(ops, eng.cmpo, tables, sites, chi_full=args.chi, lanczos_tol=args.tol, maxrestart=8)

    def timed(e, fn, n):
        fn()                                   # plans and pool warm
        ops.sync()
        e.stats.clear()
        t0 = time.perf_counter()
        for _ in range(n):
            Ex = fn()
        ops.sync()
        return (time.perf_counter() - t0) / n, Ex, sum(s.n_matvec for s in e.stats) / n

    def split(e, fn):
        e.profile = True
        e.stats.clear()
        fn()
        st = list(e.stats)
        e.profile = False
        return {"solve": sum(s.t_lanczos for s in st), "svd": sum(s.t_svd for s in st), "env": sum(s.t_env for s in st),
                "plan": sum(s.t_plan for s in st), "matvecs": sum(s.n_matvec for s in st)}

    ev, gs = fresh(), fresh()
    t_ev, E_ev, mv_ev = timed(ev, lambda: ev.tdvp_sweep(args.dt), args.sweeps)
    t_gs, E_gs, mv_gs = timed(gs, gs.sweep, args.sweeps)
    s_ev, s_gs = split(ev, lambda: ev.tdvp_sweep(args.dt)), split(gs, gs.sweep)
    print(f"tdvp sweep   {t_ev:.4f} s  matvecs {mv_ev:.0f}  {1e3 * t_ev / mv_ev:.4f} ms/matvec  E/L={E_ev / L:.12f}  stages (profiled): "
          f"exponentials {s_ev['solve']:.4f}  SVD {s_ev['svd']:.4f}  environments {s_ev['env']:.4f}  plan {s_ev['plan']:.4f}", file=sys.stderr)
    print(f"ground sweep {t_gs:.4f} s  matvecs {mv_gs:.0f}  {1e3 * t_gs / mv_gs:.4f} ms/matvec  E/L={E_gs / L:.12f}  stages (profiled): "
          f"Lanczos {s_gs['solve']:.4f}  SVD {s_gs['svd']:.4f}  environments {s_gs['env']:.4f}  plan {s_gs['plan']:.4f}", file=sys.stderr)
    print(json.dumps({"L": L, "chi": args.chi, "dt": args.dt, "tol": args.tol, "tdvp_sweep_s": t_ev, "ground_sweep_s": t_gs,
                      "tdvp_matvecs": mv_ev, "ground_matvecs": mv_gs, "tdvp_ms_per_matvec": 1e3 * t_ev / mv_ev,
                      "ground_ms_per_matvec": 1e3 * t_gs / mv_gs, "tdvp_stages_s": s_ev, "ground_stages_s": s_gs, "tails": tails}))


if __name__ == "__main__":
    main()
