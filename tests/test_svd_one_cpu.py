"""The cases and checks of tests/svd_cases.py on a machine without a GPU: an independent, correct implementation of the C-ABI
call (emul.NumpyOps.jacobi_svd: LAPACK) passes every bar, every contract check and every NaN-gap check, and the
extended-precision truth is affordable.  Not asserted of the emulator: the bit-repeat, `info` (it reports 1 for every block)
and the two RELATIVE accuracy properties -- the column-graded block and the 4 eps of an already orthogonal block (LAPACK
measures 6 eps there) -- for which the complex128 twin of the truth loop stands as the candidate."""
import time

import numpy as np
import pytest

import svd_cases as sc
from emul import NumpyOps


@pytest.mark.parametrize("name", sc.SHAPE_CALLS + sc.SPECTRUM_CALLS)
def test_numpy_emulator_passes_every_check(name):
    call = sc.CALLS[name]
    P = sc.pack(call)
    t0 = time.time()
    figs = sc.check(call, P, sc.run(NumpyOps(seed=1), call, P), check_info=False, check_relative=False)
    sc.scale_report(call, figs)
    print(f"{name}: {len(call.blocks)} blocks, truth and checks {time.time() - t0:.2f} s")


def test_truth_recovers_planted_spectra():
    """the truth loop against spectra known by construction (U diag(s) W^H with orthonormal factors, rounded to double: the
    singular values move by a few eps sigma_max at most), without LAPACK in between"""
    for cname, _, _ in sc.CARRIERS:
        b = sc.CALLS["multiplets"].blocks[[c[0] for c in sc.CARRIERS].index(cname)]
        truth = sc.ref_of(b)[0]
        want = np.zeros(b.n)
        want[:len(sc.MULTIPLETS)] = sc.MULTIPLETS
        dev = float(np.abs(truth - want).max())
        print(f"{b.name}: |truth - planted| {dev:.3e}")
        assert dev <= 64 * sc.EPS
    b = sc.CALLS["orthogonal"].blocks[0]
    d = np.sort(b.diag)[::-1]
    assert np.all(np.abs(sc.ref_of(b)[0] - d) <= sc.EPS * d)        # the polished block: norms are d to a fraction of eps


def test_twin_on_the_column_graded_block():
    """M = B D with unit columns in B and D over 12 decades: one-sided Jacobi gives every singular value to high RELATIVE
    accuracy.  The complex128 twin of the truth loop measures what double arithmetic leaves: 1.5e-15 here; the GPU test
    holds the kernel to max(10 x twin, 64 eps).  LAPACK's values are only absolutely accurate (printed)."""
    b = sc.CALLS["column_graded"].blocks[0]
    twin = sc.relative_deviation(sc.twin_of(b), b)
    lap = sc.relative_deviation(np.linalg.svd(b.M, compute_uv=False), b)
    print(f"column graded: twin {twin:.3e}, numpy.linalg.svd {lap:.3e} (relative, worst singular value)")
    assert twin <= 1e-10, "above this the twin is no yardstick and the GPU assertion is left out"
    ref, sig, bar = sc.ref_of(b)
    assert np.abs(sc.twin_of(b) - ref).max() <= bar * sig


def test_twin_on_the_already_orthogonal_blocks():
    """columns of an isometry times a positive diagonal d: nothing to rotate, S is d to 4 eps of every entry"""
    for b in sc.CALLS["orthogonal"].blocks:
        d = np.sort(b.diag)[::-1]
        got, sweeps = sc.hestenes(b.M, dtype=np.complex128, tol=sc.TOL, zero_rel=1e-15, max_sweeps=sc.MAX_SWEEPS)
        print(f"{b.name}: twin against the diagonal, worst {np.abs(got / d - 1).max() / sc.EPS:.2f} eps, sweeps {sweeps}")
        assert sweeps == 1 and np.all(np.abs(got - d) <= 4 * sc.EPS * d)


def test_copy_case_and_emulator_zero_scale():
    """the case of the staging-copy test: NumpyOps.batched_copy writes 0 where inv_norm meets a scale entry of exactly 0.0
    and leaves the padding rows and gaps NaN"""
    dst0, src, idx, scl, items, spans = sc.copy_case()
    ref = dst0.copy()
    NumpyOps().batched_copy(ref, src, idx, scl, items, len(items), 0.7)
    assert sorted({(int(i["op"]), int(i["gather_dim"]), int(i["scale_dim"]), int(i["inv_norm"])) for i in items}) == sorted(sc.COPY_CFG)
    sc.check_copy(dst0, ref, ref, items, spans)
