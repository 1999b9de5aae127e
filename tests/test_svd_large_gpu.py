"""The three multi-workgroup Jacobi SVD paths -- the ring (k_jacobi_ring), the pair visits (k_jacobi_pairs_gram +
k_jacobi_check + k_jacobi_finish, HTN_SVD_PAIRS=1) and the tall visits (k_jacobi_tall_visit + k_jacobi_check) -- at the
shapes and edge spectra of tests/svd_large_cases.py, against an extended-precision truth.  Every call is made twice from
the same packed buffers: same bytes in G, Vj, S, info and the return value; the NaN gaps behind every region stay
untouched; info >= 0 and at least one outer sweep of the large-block path.

HTN_SVD_PAIRS is read once per process: ONE fresh child (this file as a script) runs every ring call through the pair
visits and leaves its arrays in a file; the parent checks them with the same checks.

max_sweeps = 40 as the engine passes it: the unpreconditioned tall blocks need at most 18 sweeps at these column counts.

Measured on an MI355X, worst |S - truth| / sigma_max over the blocks of a call (bar 1.42e-14 = 64 eps, the floor of ref_of;
7.26e-14 on the (40, 40) cluster, where numpy.linalg.svd itself is 7.3e-15 off), sweeps in brackets:

                     ring (48, 202)   ring (40, 280)   ring (40, 40) x 7   tall 600 x 24   pairs, same three blocks
  graded             2.9e-15 [8]      2.1e-15 [7]      1.6e-15 [8]         1.7e-15 [18]    1.0e-15 1.1e-15 1.1e-15 [8 7 8]
  multiplets         4.9e-16 [5]      5.3e-16 [5]      4.1e-16 [4]         2.1e-15 [14]    4.9e-16 9.7e-16 7.4e-16 [5 5 5]
  cluster            3.5e-15 [5]      2.7e-15 [5]      3.0e-15 [5]         2.2e-15 [4]     4.5e-15 3.7e-15 4.0e-15 [5 5 5]
   with the old rule 4.2e-13          3.5e-13          3.9e-13             2.1e-13         3.8e-13 4.2e-13 3.8e-13  (FAILED)
  rank0              0 [1]            0 [1]            0 [1]               0 [1]           0 0 0 [1 1 1]
  rank1              8.2e-17 [1]      6.1e-17 [1]      2.1e-17 [1]         2.9e-16 [2]     8.2e-17 6.1e-17 2.1e-17 [1 1 1]
  rank_half          5.6e-15 [7]      7.9e-15 [6]      8.2e-15 [6]         8.9e-16 [14]    5.6e-15 7.9e-15 8.2e-15 [7 6 6]
  zero_columns       3.8e-15 [8]      3.0e-15 [8]      3.9e-15 [7]         2.1e-15 [14]    2.5e-15 1.1e-15 1.2e-15 [7 8 7]
  orthogonal         --               --               5.6e-17 [1], 1 eps  5.7e-17 [1], 0.5 eps    pairs: 5.6e-17 [1], 1 eps
  scaled 2^0, +-100  3.0e-15 [8 8 8]  1.9e-15 [8 8 8]  2.2e-15 [8 8 8]     1.3e-15 [18 18 18]      1.3e-15 1.1e-15 4.4e-16
  column_graded      --               --               --                  relative 6.1e-16 [4] (twin 1.7e-15, bar 1.7e-14)
  shape calls: ring16 7.9e-15 [8 8 8], ring16_split 2.5e-15 [7 8 7], ring64 3.1e-15 [8 8 7], tall 1.9e-15 [3 16 18 12 9];
  pairs: ring16 3.7e-15 [7 7 8], ring16_split 1.3e-15 [7 8 8], ring64 7.4e-16 [8 8 7].  S of the scaled blocks / 2^+-100 is
  bit-identical to the unscaled block's on every path.

[cluster] (s_i = 1 + i 1e-13) failed on all three paths with the rule they shared, done = mx <= max(tol^2, 0.1 tol), each
in its own copy (the "old rule" row: measured with the parent commit's kernels and these tests): the sweep saw squared
cosines of 1e-24 and was taken for the last, but inside a cluster it rotates by angles of order one, which carry the
cosines over at first order.  jacobi_last_sweep (htn_svd_cols.h) is now the one statement of the rule for all four paths:
the visits and the ring keep the largest tan^2 a sweep rotated by beside its largest squared cosine (integer maxima on the
bit patterns, as before) and also ask for tan^2 x mx <= tol^2.  Every figure and every sweep count of the other rows is
what it was before the change, bit-repeat included; so are `used` and `info` of all 78 htn_jacobi_svd_z calls that
test_kernels_gpu.py, test_ring_two_partner_gpu.py, test_ring_exchange_gpu.py, test_tall_svd_gpu.py and test_svd_one_gpu.py
make in their own process (31 of them on the large paths): no count moved.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _twice(ops, lc, name):
    call = lc.CALLS[name]
    P = lc.pack(call)
    first, second = lc.run_large(ops, call, P), lc.run_large(ops, call, P)
    same = [what for what, a, b in zip(("G", "Vj", "S", "info"), first, second) if not lc.same_bytes(a, b)]
    if first[4] != second[4]:
        same.append("return value")
    return call, P, first, same


if __name__ == "__main__":          # the child of test_pair_visits: every ring call with HTN_SVD_PAIRS=1 -> one .npz
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import svd_large_cases as lc
    from hubbardtn_amd.device import HipOps
    assert os.environ.get("HTN_SVD_PAIRS") == "1"
    ops = HipOps(0)
    out = {}
    for name in lc.RING_CALLS:
        call, P, first, differs = _twice(ops, lc, name)
        for what, a in zip(("G", "Vj", "S", "info"), first):
            out[f"{name}/{what}"] = a
        out[f"{name}/used"] = np.int64(first[4])
        out[f"{name}/differs"] = np.array(",".join(differs))
    np.savez(sys.argv[1], **out)
    print("RESULT written", len(lc.RING_CALLS))
    sys.exit(0)


import svd_large_cases as lc        # noqa: E402

pytestmark = pytest.mark.gpu


def _check(call, P, result, path):
    """the checks of svd_cases.check in its large-path mode, then what belongs to single blocks; prints every figure first"""
    print(f"{path} {call.name}: info {result[3].tolist()}, outer sweeps {result[4]}")
    figs, used = lc.check(call, P, result, large=True)
    worst = max(figs.values(), key=lambda f: f[0] / f[1])
    print(f"{path} {call.name}: worst |S - truth| / sigma_max {worst[0]:.3e} against its bar {worst[1]:.3e}; "
          f"sweeps {result[3].tolist()}, outer sweeps {used}")
    lc.scale_report(call, figs)
    for b in call.blocks:
        if b.colgraded:
            twin = lc.relative_deviation(lc.twin_of(b), b)
            got = lc.relative_deviation(figs[b.name][2], b)
            print(f"{path} {b.name}: relative, worst singular value: kernel {got:.3e}, twin {twin:.3e}, "
                  f"bar {max(10 * twin, 64 * lc.EPS):.3e}")
            assert twin <= 1e-10, "the twin is no yardstick"
            assert got <= max(10 * twin, 64 * lc.EPS), (b.name, got, twin)
    return figs


def _run_twice_and_check(hip_ops, name, path):
    call, P, first, differs = _twice(hip_ops, lc, name)
    _check(call, P, first, path)
    assert not differs, (name, differs, "differs between two calls from the same input")


@pytest.mark.parametrize("name", [n for n in lc.SHAPE_CALLS if lc.CALLS[n].ring()])
def test_ring_shapes(hip_ops, name):
    """graded over 12 decades, three blocks per launch (svd_large_cases.EXPECT): the 16-lane form at E = 13, at its last row
    count and at w = 25; seven workgroups with interior ones, ragged and empty panels (split = 1); the 64-lane form at its
    first row count, with P = 3 and at 512 rows"""
    _run_twice_and_check(hip_ops, name, "ring")


def test_tall_shapes(hip_ops):
    """plain blocks above 512 rows, five in one call: 513 x 2 (one pair), 520 x 17 (a last panel of one column), 600 x 24,
    600 x 12 with accumulate (J unitary, G' = M J), 530 x 9 without (its Vj region keeps the sentinel).  Wide tall blocks
    need more than 513 columns and stay with tests/test_tall_svd_gpu.py."""
    _run_twice_and_check(hip_ops, "tall", "tall")


@pytest.mark.parametrize("name", lc.SPECTRUM_CALLS)
def test_edge_spectra(hip_ops, name):
    """exact multiplets, a cluster 1e-13 apart, exact rank 0 / 1 / half, planted zero columns, already orthogonal columns
    (one sweep, S to 4 eps of every entry: what the complex128 twin allows, test_svd_large_cpu.py -- for the QRCP carrier
    after a pivoted QR), powers of two and the column-graded block (relative accuracy), each on one carrier per path:
    QRCP (48, 202) (ring, 16 lanes), QRCP (40, 280) (ring, 64 lanes), QRCP (40, 40) with split = 1 (ring, seven
    workgroups), plain 600 x 24 (tall)."""
    _run_twice_and_check(hip_ops, name, "tall" if name.endswith("_tall") else "ring")


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pairs") / "pairs.npz")
    env = dict(os.environ)
    env["HTN_SVD_PAIRS"] = "1"
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RESULT written" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", lc.RING_CALLS)
def test_pair_visits(pairs, name):
    """the blocks of the ring tests through k_jacobi_pairs_gram: panels of 8 columns, 16 x 16 Gram visits, one launch per
    tournament round, k_jacobi_check after every outer sweep"""
    call = lc.CALLS[name]
    result = tuple(pairs[f"{name}/{what}"] for what in ("G", "Vj", "S", "info")) + (int(pairs[f"{name}/used"]),)
    _check(call, lc.pack(call), result, "pairs")
    assert str(pairs[f"{name}/differs"]) == "", (name, str(pairs[f"{name}/differs"]))
