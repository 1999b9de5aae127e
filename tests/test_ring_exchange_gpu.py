"""The panel exchange of k_jacobi_ring: the direct form (columns leave from registers in the last cross step of a round, the
two directions are received independently, the received columns bring their squared norms) against the staged form it replaced
(HTN_RING_STAGED_SEND=1), bit for bit.

Neither form changes which rotations happen, their order or their operands, so S, G' and the sweep counts must be IDENTICAL --
not close.  The switch, HTN_RING_NO_XCD and HTN_DEBUG_POISON are read once per process: each runs in a fresh child (this file
as a script), which reports SHA-256 digests of the raw result bytes; HTN_RING_TWO_PARTNER is read per call.

Shapes (m0 x n0, full rank; planning rule in tests/test_ring_two_partner_gpu.py), the smallest that reach each branch:
  100 x 100   w = 25, P = 2: the only workgroups are the first (its top panel stays) and the last (its top becomes its bottom),
              each receives one panel with all waves
  128 x 128   w = 32, P = 2, full panels: every group of 16 lanes owns a column
  202 x 202   w = 15, P = 7: interior workgroups (both panels leave, both directions come in), last panel of 7 columns
  197 x 197   w = 15, P = 7, last panel of 2 columns: nt != nb, bottom columns that no rotation touches in the last step
  300 x 280   280 rows per column: the 64-lane form (one column per wave, two columns per wave in a receiving half)
  100 x 100 and 202 x 202 in one call: two blocks in one launch
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {
    "100": [(100, 100, 100)],
    "128": [(128, 128, 128)],
    "202": [(202, 202, 202)],
    "197": [(197, 197, 197)],
    "300x280": [(300, 280, 280)],
    "100+202": [(100, 100, 100), (202, 202, 202)],
}
SEED = 61


def _digest(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def run_cases(ops, keep=False):
    """every case with one partner per step (key "one") and with two ("two"): digests of S and G', the sweep counts; with
    keep, the default form's arrays as well"""
    from test_ring_two_partner_gpu import _run
    out, arrays = {}, {}
    old = os.environ.get("HTN_RING_TWO_PARTNER")
    try:
        for name, shapes in CASES.items():
            out[name] = {}
            for key in ("one", "two"):
                if key == "two":
                    os.environ["HTN_RING_TWO_PARTNER"] = "1"
                else:
                    os.environ.pop("HTN_RING_TWO_PARTNER", None)
                mats, desc, Gp, S, inf = _run(ops, shapes, seed=SEED)
                out[name][key] = {"S": _digest(S), "G": _digest(Gp), "sweeps": [int(x) for x in inf]}
                if keep and key == "one":
                    arrays[name] = (mats, desc, Gp, S, inf)
    finally:
        if old is None:
            os.environ.pop("HTN_RING_TWO_PARTNER", None)
        else:
            os.environ["HTN_RING_TWO_PARTNER"] = old
    return (out, arrays) if keep else out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from hubbardtn_amd.device import HipOps
    ops = HipOps(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    print("RESULT " + json.dumps([run_cases(ops) for _ in range(reps)]))
    sys.exit(0)


pytestmark = pytest.mark.gpu


def _child(env_name, reps=1):
    env = dict(os.environ)
    env.pop("HTN_RING_TWO_PARTNER", None)
    env[env_name] = "1"
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(reps)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.fixture(scope="module")
def direct(hip_ops):
    return run_cases(hip_ops, keep=True)


@pytest.fixture(scope="module")
def staged():
    return _child("HTN_RING_STAGED_SEND")[0]


@pytest.fixture(scope="module")
def dense():
    return _child("HTN_RING_NO_XCD")[0]


@pytest.fixture(scope="module")
def poisoned():
    return _child("HTN_DEBUG_POISON", reps=2)


@pytest.mark.parametrize("case", list(CASES))
def test_direct_exchange_is_the_staged_exchange_bit_for_bit(direct, staged, case):
    assert all(s > 0 for s in direct[0][case]["one"]["sweeps"]), direct[0][case]
    assert direct[0][case]["one"] == staged[case]["one"]


@pytest.mark.parametrize("case", list(CASES))
def test_dense_placement_changes_nothing(direct, dense, case):
    """HTN_RING_NO_XCD=1: the hand-off through memory (write-through stores) instead of one XCD's L2"""
    assert direct[0][case]["one"] == dense[case]["one"]


@pytest.mark.parametrize("case", list(CASES))
def test_two_partner_step_with_either_exchange(direct, staged, case):
    """the two-partner step keeps the staged send and takes the direct receive"""
    assert all(s > 0 for s in direct[0][case]["two"]["sweeps"]), direct[0][case]
    assert direct[0][case]["two"] == staged[case]["two"]


@pytest.mark.parametrize("case", list(CASES))
def test_direct_exchange_matches_lapack(direct, case):
    """the comparisons and bars of tests/test_ring_two_partner_gpu.py (13 sweeps for the 64-lane form, as there)"""
    from test_ring_two_partner_gpu import _check
    _check(CASES[case], *direct[1][case], max_sweeps=13 if case == "300x280" else 12)


@pytest.mark.parametrize("case", list(CASES))
def test_poisoned_pool_changes_nothing(direct, poisoned, case):
    """HTN_DEBUG_POISON=1, the schedule twice in one process: no read of memory the kernels did not write, nothing left over
    from the call before (flags, mailboxes, epochs)"""
    assert len(poisoned) == 2
    for rep in poisoned:
        assert rep[case] == direct[0][case]
