"""Generates tests/golden/plan_digests.json: SHA-256 digests of what the launch balancer (htn_balance_tiles of the CPU baseline
library) returns for fixed task lists, so that a refactor of the planner or the balancer is pinned to what the library emitted
when the file was written.

Inputs (tests/gemm_cases.py): three random lists -- the two whose K loops are cut and one that stays whole -- and the H_eff
apply lists (htn_plan_apply_dump, stages 0 and 1) of every bond of the nnn_nn and poly chains after one sweep, each balanced
for 256 and for 7 compute units.  Tile records hold integers only, and so does the slab count hashed after them: the file does
not depend on compiler or machine (the recoupling coefficients, which do at the last bit, are compared with
tests/ref_planner.py by tests/test_cengine_cpu.py).

Run on the commit whose output is to be pinned:  python tests/golden/make_plan_digests.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from cpu_ops import CpuOps                # noqa: E402
import gemm_cases                         # noqa: E402


def main():
    dig = gemm_cases.plan_digests(CpuOps())
    out = os.path.join(HERE, "plan_digests.json")
    with open(out, "w") as f:
        json.dump(dig, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, len(dig), "entries")


if __name__ == "__main__":
    main()
