"""What perfect sampling costs at the headline size (a measurement tool, not part of bench.py; the twin of
tools/variance_bench.py).

Grows the state bench.py prepares (L = 64, U/t = 4, chi = 1024 by default: the same random start, growth schedule and warm-up
sweeps) and times, in one process on one device:
  * one two-site sweep, for scale;
  * engine.DMRG2.sample(): the first call (it plans the item lists of every site) and planned calls at batch sizes 1, 16, 64
    and 256, as seconds per sample (the yardstick for "batched is worth it" is batch = 1 on the same build);
  * the library's own split of a planned call into host planning and device passes.
The shares of the probe, choose and close kernels come from a kernel trace of a run of their own: --trace does the growth and
one planned call at --trace-batch and nothing else, to be run under a kernel tracer.  One JSON line at the end.

    python tools/bench_sample.py [--L 64] [--chi 1024] [--samples 256] [--out profiles/bench_sample.json]
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
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--batches", type=str, default="1,16,64,256")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-batch", type=int, default=64)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import numpy as np
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

    rng = np.random.default_rng(0)
    if args.trace:
        u = rng.random((args.trace_batch, L))
        eng.sample(u, batch=args.trace_batch)
        eng.sample(u, batch=args.trace_batch)
        print(json.dumps({"trace": True, "batch": args.trace_batch}))
        return
    out = {"L": L, "chi": args.chi, "dim_widest": max(b.dim_full for b in eng.bonds), "samples": args.samples}
    out["sweep_s"], _ = timed(eng.sweep)
    out["first_call_s"], (occ, logp, split) = timed(lambda: eng.sample(rng.random((1, L)), batch=1, timed=True))
    out["first_call_plan_s"] = split[0]
    per = {}
    for b in (int(x) for x in args.batches.split(",")):
        n = max(b, min(args.samples, 16 * b))                 # (batch 1 is timed on 16 samples, not on all of them)
        u = rng.random((n, L))
        best, sp = None, None
        for _ in range(2):
            t, (occ, logp, split) = timed(lambda: eng.sample(u, batch=b, timed=True))
            if best is None or t < best:
                best, sp = t, split
        per[b] = best / n
        out[f"batch{b}_s_per_sample"] = best / n
        out[f"batch{b}_plan_s"], out[f"batch{b}_device_s"] = sp
        out[f"batch{b}_mean_logp"] = float(logp.mean())
    out["mean_N"] = float(np.asarray(eng.sym.site_electrons)[occ].sum(axis=1).mean())
    out["best_batch"] = min(per, key=per.get)
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
