"""What G(x, t) costs at the headline size (a measurement tool, not part of bench.py).

Grows the state bench.py prepares (L = 64, U/t = 4, chi = 1024 by default: the same random start, growth schedule and warm-up
sweeps) and times, in one process on one device:
  * api.apply_operator(psi, "c+", L // 2): the copy, the centre moves and htn_mps_apply_op itself (first call: it plans);
  * engine.DMRG2.transition("c+", phi): first call (plans 3L overlap steps and L pairings) and later calls;
  * one tdvp_sweep of the applied state (truncdim chi), twice: the first grows the fused bonds into Schmidt form;
  * correlator("hop"), first and later calls, for scale.
Also the bond growth of the applied state: multiplets and `dim` of the widest bond of the source, of the applied state, and of
the applied state after its first and second TDVP sweep.  One JSON line at the end.

    python tools/greens_bench.py [--L 64] [--chi 1024] [--dt 0.05] [--tol 1e-10] [--out profiles/greens_bench.json]
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
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--tol", type=float, default=1e-10)
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

    def widest(e):
        bs = e.bonds
        return {"multiplets": max(sum(b.dims.values()) for b in bs), "dim": max(b.dim_full for b in bs)}

    out = {"L": L, "chi": args.chi, "dt": args.dt, "tol": args.tol, "source_bonds": widest(eng)}
    out["ground_sweep_s"], _ = timed(eng.sweep)
    psi = api.FiniteMPS(eng, L)
    out["apply_operator_first_s"], phi = timed(lambda: api.apply_operator(psi, "c+", L // 2))
    out["apply_operator_again_s"], _ = timed(lambda: api.apply_operator(psi, "c+", L // 2))
    work = eng.copy()
    work.move_centre(L // 2)
    out["apply_op_call_first_s"], _ = timed(lambda: work.apply_op(L // 2, "c+"))          # (plans of `work`: a fresh cache)
    out["apply_op_call_again_s"], _ = timed(lambda: work.apply_op(L // 2, "c+"))
    out["applied_bonds"] = widest(phi.engine)
    out["applied_norm2"] = phi.engine.applied_norm2
    ket = phi.engine
    out["move_centre_to_0_s"], _ = timed(lambda: ket.move_centre(0))
    out["applied_bonds_after_move"] = widest(ket)
    out["transition_first_s"], C0 = timed(lambda: eng.transition("c+", ket))
    ts = [timed(lambda: eng.transition("c+", ket))[0] for _ in range(3)]
    out["transition_again_s"] = min(ts)
    out["C0_at_site"] = [C0[L // 2].real, C0[L // 2].imag]
    ket.chi_full, ket.cutoff, ket.lanczos_tol, ket.maxrestart = args.chi, 0.0, args.tol, 8
    out["tdvp_sweep_first_s"], _ = timed(lambda: ket.tdvp_sweep(args.dt))
    out["applied_bonds_after_sweep_1"] = widest(ket)
    out["tdvp_sweep_second_s"], _ = timed(lambda: ket.tdvp_sweep(args.dt))
    out["applied_bonds_after_sweep_2"] = widest(ket)
    out["transition_after_sweeps_first_s"], _ = timed(lambda: eng.transition("c+", ket))
    out["transition_after_sweeps_again_s"] = min(timed(lambda: eng.transition("c+", ket))[0] for _ in range(3))
    out["correlator_hop_first_s"], G = timed(lambda: eng.correlator("hop"))
    out["correlator_hop_again_s"] = min(timed(lambda: eng.correlator("hop"))[0] for _ in range(3))
    out["trace_G"] = float(G.trace().real)
    for k, v in out.items():
        print(f"{k}: {v}", file=sys.stderr)
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
