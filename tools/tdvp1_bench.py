"""One one-site TDVP sweep beside one two-site TDVP sweep from the same state (a measurement tool, not part of bench.py).

Grows the headline state the way bench.py does (L = 64, U/t = 4, chi = 1024 by default: the same random start, growth schedule
and warm-up sweeps), downloads it, and times tdvp1_sweep(dt) (htn_tdvp1_sweep: 2L-1 one-site exponentials, 2L-2 QR gauge moves
and 2L-2 zero-site exponentials on the bonds) and tdvp_sweep(dt) (htn_tdvp2_sweep: 2L-2 bond exponentials with their SVDs and
2L-4 backward one-site exponentials) from two engines built on those tensors: median of --sweeps timed sweeps after one
warm-up sweep each, both matvec counts, and the stage split of one profiled sweep each (stages bracketed by stream syncs, which
perturbs the total; "svd" is the QR + absorption for the one-site sweep).  One JSON line at the end.

    python tools/tdvp1_bench.py [--L 64] [--chi 1024] [--dt 0.05] [--tol 1e-10] [--sweeps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--U", type=float, default=4.0)
    ap.add_argument("--chi", type=int, default=1024)
    ap.add_argument("--grow", type=str, default="16x8,32x4,64x4,128x2,256x2,512x2")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sweeps", type=int, default=5)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--tol", type=float, default=1e-10)
    args = ap.parse_args()
    from hubbardtn_amd import engine, models, mps
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
        ts, mv = [], []
        for _ in range(n):
            e.stats.clear()
            t0 = time.perf_counter()
            Ex = fn()
            ops.sync()
            ts.append(time.perf_counter() - t0)
            mv.append(sum(s.n_matvec for s in e.stats))
        return statistics.median(ts), Ex, statistics.median(mv), ts

    def split(e, fn):
        e.profile = True
        e.stats.clear()
        fn()
        st = list(e.stats)
        e.profile = False
        return {"solve": sum(s.t_lanczos for s in st), "svd": sum(s.t_svd for s in st), "env": sum(s.t_env for s in st),
                "plan": sum(s.t_plan for s in st), "matvecs": sum(s.n_matvec for s in st)}

    one, two = fresh(), fresh()
    t1, E1, mv1, all1 = timed(one, lambda: one.tdvp1_sweep(args.dt), args.sweeps)
    t2, E2, mv2, all2 = timed(two, lambda: two.tdvp_sweep(args.dt), args.sweeps)
    s1, s2 = split(one, lambda: one.tdvp1_sweep(args.dt)), split(two, lambda: two.tdvp_sweep(args.dt))
    print(f"one-site sweep {t1:.4f} s  matvecs {mv1:.0f}  E/L={E1 / L:.12f}  stages (profiled): exponentials {s1['solve']:.4f}  "
          f"QR + absorption {s1['svd']:.4f}  environments {s1['env']:.4f}  plan {s1['plan']:.4f}", file=sys.stderr)
    print(f"two-site sweep {t2:.4f} s  matvecs {mv2:.0f}  E/L={E2 / L:.12f}  stages (profiled): exponentials {s2['solve']:.4f}  "
          f"SVD {s2['svd']:.4f}  environments {s2['env']:.4f}  plan {s2['plan']:.4f}", file=sys.stderr)
    print(json.dumps({"L": L, "chi": args.chi, "dt": args.dt, "tol": args.tol, "sweeps": args.sweeps, "tdvp1_sweep_s": t1,
                      "tdvp2_sweep_s": t2, "tdvp1_matvecs": mv1, "tdvp2_matvecs": mv2, "tdvp1_all_s": all1, "tdvp2_all_s": all2,
                      "tdvp1_stages_s": s1, "tdvp2_stages_s": s2, "max_bond_dim": max(one.bond_dims())}))


if __name__ == "__main__":
    main()
