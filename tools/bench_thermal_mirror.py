"""One sweep under G against two sweeps under K: what the two schemes of api.thermal_greens_function cost and how far each is from its
own run at twice the bond dimension (a measurement tool, not part of bench.py).

One-band chain, U/t = 4, mu = U / 2 (half filling), --L physical sites, cooled once per bond dimension to --beta with truncdim(chi),
then t = 0 ... --tmax in steps of --dt with op = "c+" at the middle site, both schemes from the same cooled state (the calls leave it
alone).  Per scheme and bond dimension:
  * wall seconds per interval (its sweeps and its transition pass, closed by a device sync): the first interval, which plans, and the
    median of the others but the last;
  * the stage split of the last interval's sweeps, run with the engine's profile switch (stages bracketed by stream syncs: that interval
    is slower and is left out of the median);
  * discarded weight per time (bra, ket) and the largest bond dimension each evolved state reached;
  * api.purification_defect of the cooled state.
With two bond dimensions (--chi 256,512) each scheme's largest |C_chi - C_2chi| over x, at every time, is its error estimate at the
smaller one; --against takes the JSON of an earlier run at the larger one instead.  One JSON line per bond dimension (C included),
written to --out-dir as they finish.

    python tools/bench_thermal_mirror.py [--L 16] [--beta 2] [--chi 256,512] [--dt 0.1] [--tmax 2] [--schemes idle,mirror] [--cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_scheme(api, engine, ops, psi, times, alg, scheme):
    sync = getattr(ops, "sync", lambda: None)
    sweep, transition = engine.DMRG2.tdvp_sweep, engine.DMRG2.transition
    marks, engines, profiled = [], [], []
    last = len(times) - 1

    def spy_sweep(self, dt):
        if not any(e is self for e in engines):
            engines.append(self)
        self.profile = len(marks) == last                  # (marks holds one entry per finished time: the last interval is profiled)
        k0 = len(self.stats)
        out = sweep(self, dt)
        if self.profile:
            profiled.extend(self.stats[k0:])
        self.bench_dim = max(getattr(self, "bench_dim", 0), max(self.bond_dims()))
        return out

    def spy_transition(self, op, ket):
        out = transition(self, op, ket)
        sync()
        marks.append(time.perf_counter())
        return out
    engine.DMRG2.tdvp_sweep, engine.DMRG2.transition = spy_sweep, spy_transition
    try:
        sync()
        t0 = time.perf_counter()
        res = api.thermal_greens_function(psi, times, alg, op="c+", ancilla=scheme)
    finally:
        engine.DMRG2.tdvp_sweep, engine.DMRG2.transition = sweep, transition
    steps = np.diff(marks)
    return {"scheme": scheme, "states_evolved": len(engines), "setup_and_t0_s": marks[0] - t0, "first_interval_s": float(steps[0]),
            "interval_s": float(np.median(steps[1:-1])) if len(steps) > 2 else float("nan"), "profiled_interval_s": float(steps[-1]),
            "total_s": marks[-1] - t0,
            "stages_s": {"exponentials": sum(s.t_lanczos for s in profiled), "svd": sum(s.t_svd for s in profiled),
                         "environments": sum(s.t_env for s in profiled), "plan": sum(s.t_plan for s in profiled),
                         "matvecs": sum(s.n_matvec for s in profiled)},
            "max_bond_dim": [int(e.bench_dim) for e in engines], "trunc_weight": res["trunc_weight"].tolist(),
            "C_re": res["C"].real.tolist(), "C_im": res["C"].imag.tolist()}


def deviation(a, b):
    """largest |C_a - C_b| over x, per time"""
    Ca, Cb = (np.array(r["C_re"]) + 1j * np.array(r["C_im"]) for r in (a, b))
    return np.abs(Ca - Cb).max(axis=1).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=16)
    ap.add_argument("--U", type=float, default=4.0)
    ap.add_argument("--beta", type=float, default=2.0)
    ap.add_argument("--dbeta", type=float, default=0.05)
    ap.add_argument("--chi", type=str, default="256,512")
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--tmax", type=float, default=2.0)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--schemes", type=str, default="idle,mirror")
    ap.add_argument("--against", type=str, default="", help="JSON line of an earlier run at the larger bond dimension")
    ap.add_argument("--out-dir", type=str, default="")
    ap.add_argument("--cpu", action="store_true", help="the CPU baseline library (small sizes: a check of the tool)")
    args = ap.parse_args()
    from hubbardtn_amd import api, engine, models
    if args.cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from cpu_ops import CpuOps
        ops = CpuOps()
    else:
        from hubbardtn_amd.device import HipOps
        ops = HipOps(0)
    sync = getattr(ops, "sync", lambda: None)
    sim = models.OB_Sim([1.0], [args.U], 0.5 * args.U, 1, 1, 2.0, 8)
    times = [round(args.dt * k, 10) for k in range(int(round(args.tmax / args.dt)) + 1)]
    done = {}
    for chi in [int(x) for x in args.chi.split(",") if x]:
        alg = api.TDVP2(trscheme=api.truncdim(chi), tol=args.tol)
        psi = api.thermal_state(sim, args.L, ops=ops)
        sync()
        t0 = time.perf_counter()
        cooled = api.cool(psi, [args.beta], alg, dbeta=args.dbeta)
        sync()
        out = {"L": args.L, "U": args.U, "beta": args.beta, "dbeta": args.dbeta, "chi": chi, "dt": args.dt, "tol": args.tol, "times": times,
               "cool_s": time.perf_counter() - t0, "cool_trunc_weight": float(cooled["trunc_weight"][0]),
               "energy": float(cooled["energy"][0]), "cooled_max_bond_dim": int(max(psi.bond_dimensions())),
               "purification_defect": float(api.purification_defect(psi).total), "schemes": {}}
        print(f"chi {chi}: cooled in {out['cool_s']:.1f} s, max bond dim {out['cooled_max_bond_dim']}, defect "
              f"{out['purification_defect']:.3e}", file=sys.stderr, flush=True)
        for scheme in [s for s in args.schemes.split(",") if s]:
            r = out["schemes"][scheme] = run_scheme(api, engine, ops, psi, times, alg, scheme)
            print(f"chi {chi} {scheme}: {r['interval_s']:.3f} s per interval (first {r['first_interval_s']:.3f}), stages {r['stages_s']}, "
                  f"max bond dim {r['max_bond_dim']}, discarded weight at the last time {r['trunc_weight'][-1]}", file=sys.stderr, flush=True)
        done[chi] = out
        line = json.dumps(out)
        if args.out_dir:
            os.makedirs(args.out_dir, exist_ok=True)
            with open(os.path.join(args.out_dir, f"thermal_mirror_L{args.L}_chi{chi}.json"), "w") as f:
                f.write(line + "\n")
        print(line, flush=True)
    ref = None
    if args.against:
        with open(args.against) as f:
            ref = json.loads(f.readline())
    chis = sorted(done)
    if ref is None and len(chis) > 1:
        ref = done[chis[-1]]
    if ref is not None:
        for chi in chis:
            if chi >= ref["chi"]:
                continue
            for scheme, r in done[chi]["schemes"].items():
                if scheme in ref["schemes"]:
                    dev = deviation(r, ref["schemes"][scheme])
                    print(json.dumps({"chi": chi, "against_chi": ref["chi"], "scheme": scheme, "deviation_per_time": dev,
                                      "deviation_at_last_time": dev[-1], "deviation_max": max(dev)}), flush=True)


if __name__ == "__main__":
    main()
