"""One-site against two-site sweep time from the same state (a measurement tool, not part of bench.py).

Grows the headline state the way bench.py does (L = 64, U/t = 4, chi = 1024 by default: the same random start, growth
schedule and warm-up sweeps), downloads it, and times three one-site sweeps (htn_dmrg1_sweep) and three two-site sweeps
(htn_dmrg2_sweep) from two engines built on those tensors.  Prints both times, then both stage splits from a profiled
sweep each (stages bracketed by stream syncs, which perturbs the total): Lanczos / QR + absorption / environments for the
one-site sweep, Lanczos / SVD / environments for the two-site one.  One JSON line at the end.

    python tools/dmrg1_bench.py [--L 64] [--chi 1024] [--sweeps 3]
"""
import argparse
import json
import os
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
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--lanczos-tol", type=float, default=1e-10)
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
    eng.chi_full, eng.lanczos_tol = args.chi, args.lanczos_tol
    for _ in range(args.warmup):
        E = eng.sweep()
    print(f"grown: chi={args.chi} E/L={E / L:.12f} max bond dim {max(eng.bond_dims())}", file=sys.stderr)
    tables = [dict(b.dims) for b in eng.bonds]
    sites = [eng.download_site(i) for i in range(L)]

    def fresh():
        return engine.DMRG2(ops, eng.cmpo, tables, sites, chi_full=args.chi, lanczos_tol=args.lanczos_tol)

    def timed(e, fn, n):
        fn()                                   # plans and pool warm
        ops.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            Ex = fn()
        ops.sync()
        return (time.perf_counter() - t0) / n, Ex

    def split(e, fn, n_updates):
        e.profile = True
        e.stats.clear()
        fn()
        st = e.stats[-n_updates:]
        e.profile = False
        return {"lanczos": sum(s.t_lanczos for s in st), "gauge": sum(s.t_svd for s in st), "env": sum(s.t_env for s in st),
                "plan": sum(s.t_plan for s in st), "matvecs": sum(s.n_matvec for s in st)}

    one, two = fresh(), fresh()
    t1, E1 = timed(one, one.sweep1, args.sweeps)
    t2, E2 = timed(two, two.sweep, args.sweeps)
    s1 = split(one, one.sweep1, 2 * L - 2)
    s2 = split(two, two.sweep, 2 * L - 3)
    print(f"one-site sweep {t1:.4f} s  E/L={E1 / L:.12f}   stages (profiled sweep): Lanczos {s1['lanczos']:.4f}  QR+absorb "
          f"{s1['gauge']:.4f}  environments {s1['env']:.4f}  plan {s1['plan']:.4f}  matvecs {s1['matvecs']}", file=sys.stderr)
    print(f"two-site sweep {t2:.4f} s  E/L={E2 / L:.12f}   stages (profiled sweep): Lanczos {s2['lanczos']:.4f}  SVD "
          f"{s2['gauge']:.4f}  environments {s2['env']:.4f}  plan {s2['plan']:.4f}  matvecs {s2['matvecs']}", file=sys.stderr)
    print(json.dumps({"L": L, "chi": args.chi, "one_site_sweep_s": t1, "two_site_sweep_s": t2, "E_one_site_per_site": E1 / L,
                      "E_two_site_per_site": E2 / L, "one_site_stages_s": s1, "two_site_stages_s": s2}))


if __name__ == "__main__":
    main()
