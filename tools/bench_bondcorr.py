"""What the bond-operator correlators cost at the headline size (a measurement tool, not part of bench.py; the twin of
tools/bench_sample.py).

Grows the state bench.py prepares (L = 64, U/t = 4, chi = 1024 by default: the same random start, growth schedule and warm-up
sweeps) and times, in one process on one device, alternating over --repeats rounds:
  * one two-site sweep, for scale;
  * engine.DMRG2.correlator("hop"): the two-point pass (two channels), the yardstick;
  * engine.DMRG2.bond_correlator(kind) for "bond", "dimer", "spair": the first call (it plans the probes) and planned calls,
    and separately the planned cost of the disjoint strings alone and of the overlap strings (same bond, shared site).
Every timed window ends in a device synchronise (the calls download their table).  Reported per kind: the number of device
passes (strings), seconds, and the ratio to one channel of the two-point pass.  One JSON line at the end.

    python tools/bench_bondcorr.py [--L 64] [--chi 1024] [--repeats 3] [--out profiles/bondcorr_bench.json]
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import numpy as np
    from hubbardtn_amd import bondcorr, engine, models, mps
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

    kinds = ("bond", "dimer", "spair")
    out = {"L": L, "chi": args.chi, "dim_widest": max(b.dim_full for b in eng.bonds), "repeats": args.repeats}
    out["sweep_s"], _ = timed(eng.sweep)
    out["hop_first_s"], _ = timed(lambda: eng.correlator("hop"))
    tabs = {k: bondcorr.strings(eng.sym, k) for k in kinds}
    for k in kinds:
        out[f"{k}_first_s"], C = timed(lambda: eng.bond_correlator(k))
        out[f"{k}_passes"] = [len(t) for t in tabs[k]]
        out[f"{k}_hermitian_dev"] = float(np.abs(C - C.conj().T).max())
    samples = {}
    for _ in range(args.repeats):                                 # planned calls, alternating
        samples.setdefault("hop_s", []).append(timed(lambda: eng.correlator("hop"))[0])
        for k in kinds:
            samples.setdefault(f"{k}_s", []).append(timed(lambda: eng.bond_correlator(k))[0])
            samples.setdefault(f"{k}_disjoint_s", []).append(timed(lambda: eng._string_values(tabs[k][2], 4))[0])
            samples.setdefault(f"{k}_shared_s", []).append(timed(lambda: eng._string_values(tabs[k][1], 3))[0])
            samples.setdefault(f"{k}_same_s", []).append(timed(lambda: eng._string_values(tabs[k][0], 2))[0])
    for name, v in samples.items():
        out[name] = float(np.median(v))
        out[name + "_spread"] = float(max(v) - min(v))
    per_channel = out["hop_s"] / 2.0                              # "hop" is two channels (hop+ / hop-)
    out["two_point_channel_s"] = per_channel
    for k in kinds:
        out[f"{k}_over_channel"] = out[f"{k}_s"] / per_channel
        out[f"{k}_disjoint_over_channel"] = out[f"{k}_disjoint_s"] / per_channel
        out[f"{k}_over_sweep"] = out[f"{k}_s"] / out["sweep_s"]
    for k, val in out.items():
        print(f"{k}: {val}", file=sys.stderr)
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
