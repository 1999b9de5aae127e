"""What the two-site energy variance costs at the headline size (a measurement tool, not part of bench.py; the twin of
tools/greens_bench.py).

Grows the state bench.py prepares (L = 64, U/t = 4, chi = 1024 by default: the same random start, growth schedule and warm-up
sweeps) and times, in one process on one device:
  * one two-site sweep, for scale;
  * engine.DMRG2.variance(): the first call (it plans the moves and the item lists) and later, planned calls;
  * a timed call, whose laps are closed by stream syncs: theta + H_eff applies / projection launches / non-optimising moves.
Also the variance of that state next to the largest discarded weight of its last sweep.  One JSON line at the end.

    python tools/variance_bench.py [--L 64] [--chi 1024] [--out profiles/variance_bench.json]
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
    ap.add_argument("--out", type=str, default="")
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

    out = {"L": L, "chi": args.chi, "dim_widest": max(b.dim_full for b in eng.bonds)}
    k0 = len(eng.stats)
    out["sweep_s"], _ = timed(eng.sweep)
    out["trunc_weight_max"] = float(max(s.trunc_weight for s in eng.stats[k0:]))
    out["trunc_weight_sum"] = float(sum(s.trunc_weight for s in eng.stats[k0:]))
    out["variance_first_s"], v = timed(eng.variance)
    out["variance_planned_s"] = min(timed(eng.variance)[0] for _ in range(3))
    t_timed, vt = timed(lambda: eng.variance(timed=True))
    out["variance_timed_s"] = t_timed
    out["split_apply_s"], out["split_projection_s"], out["split_moves_s"] = vt.split
    out["variance_total"], out["variance_site_sum"], out["variance_bond_sum"] = v.total, float(v.site.sum()), float(v.bond.sum())
    out["energy"], out["energy_sweep"] = v.energy, eng.energy
    out["sweep_after_s"], _ = timed(eng.sweep)
    for k, val in out.items():
        print(f"{k}: {val}", file=sys.stderr)
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
