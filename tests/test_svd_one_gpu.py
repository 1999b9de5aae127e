"""The one-workgroup Jacobi SVD kernel (k_jacobi_svd) at every lane-group instance, switch point and edge spectrum of
tests/svd_cases.py, against an extended-precision truth, and the staging copy of the same translation unit
(k_batched_copy) beyond one trip of its grid.  Every call is made twice from the same input: same bytes."""
import numpy as np
import pytest

import svd_cases as sc
from emul import NumpyOps

pytestmark = pytest.mark.gpu


def _run_twice_and_check(hip_ops, name):
    call = sc.CALLS[name]
    P = sc.pack(call)
    first = sc.run(hip_ops, call, P)
    second = sc.run(hip_ops, call, P)
    figs = sc.check(call, P, first)
    worst = max(figs.values(), key=lambda f: f[0] / f[1])
    print(f"{name}: worst |S - truth| / sigma_max {worst[0]:.3e} against its bar {worst[1]:.3e}; sweeps {first[3].tolist()}")
    for what, a, b in zip(("G", "Vj", "S", "info"), first, second):
        assert sc.same_bytes(a, b), (name, what, "differs between two calls from the same input")
    # the return value counts the outer sweeps of the large-block path: 0 says that no block left k_jacobi_svd
    assert first[4] == 0 and second[4] == 0, (name, first[4], second[4])
    return call, figs


@pytest.mark.parametrize("name", sc.SHAPE_CALLS)
def test_every_instance_and_switch_point(hip_ops, name):
    """the smallest shapes that select each jacobi_sweeps_pad<GS, E>, jacobi_sweeps<GS> and qrcp_mgs<GS> (svd_cases.EXPECT),
    in LDS and in global memory, graded over 12 decades"""
    _run_twice_and_check(hip_ops, name)


@pytest.mark.parametrize("name", [n for n in sc.SPECTRUM_CALLS if n != "column_graded"])
def test_edge_spectra(hip_ops, name):
    """exact multiplets, a cluster 1e-13 apart, exact rank 0 / 1 / half, planted zero columns, already orthogonal columns
    (one sweep, S to 4 eps of every entry) and powers of two, each on a plain 300 x 12, a QRCP (12, 300) and a QRCP (40, 40)
    block.

    [cluster] (s_i = 1 + i 1e-13) is the case that found a defect.  With the stopping rule done = mx <= max(tol^2, 0.1 tol)
    alone the kernel stopped after ONE sweep, |S - truth| / sigma_max = 1.47e-13 (plain 300 x 12), 1.40e-13 (QRCP (12, 300)),
    4.47e-13 (QRCP (40, 40)) against the bar 1.42e-14: the sweep saw squared cosines of 1e-24, but inside a cluster it
    rotates by angles of order one, which carry the cosines over at first order.  jacobi_last_sweep (htn_svd_cols.h) now
    also asks for (largest tan^2 rotated by) x mx <= tol^2; measured on an MI355X with it: 5.9e-16, 2.1e-15, 5.0e-15 in
    4, 4, 5 sweeps, and the sweep count of every other case of this module is what it was.  Every other spectrum stays
    below 3.1e-15."""
    call, figs = _run_twice_and_check(hip_ops, name)
    sc.scale_report(call, figs)


def test_column_graded_relative_accuracy(hip_ops):
    """M = B D, B 200 x 12 with unit columns, D over 12 decades: one-sided Jacobi can give every singular value to high
    RELATIVE accuracy.  Yardstick: the same Hestenes loop in complex128 on the CPU (the twin), worst relative deviation
    from the truth 1.49e-15; the kernel must stay within max(10 x twin, 64 eps) = 1.49e-14.  Measured on an MI355X: 1.36e-15
    in four sweeps (numpy.linalg.svd on the same block: 6.1e-16)."""
    call, figs = _run_twice_and_check(hip_ops, "column_graded")
    b = call.blocks[0]
    twin = sc.relative_deviation(sc.twin_of(b), b)
    got = sc.relative_deviation(figs[b.name][2], b)
    print(f"column graded: kernel {got:.3e}, twin {twin:.3e}, bar {max(10 * twin, 64 * sc.EPS):.3e} (relative, worst singular value)")
    assert twin <= 1e-10, "the twin is no yardstick"
    assert got <= max(10 * twin, 64 * sc.EPS)


def test_batched_copy_beyond_one_trip_of_the_grid(hip_ops):
    """items of 256, 257, 4096 (exactly one trip of 256 threads x 16 workgroups), 4270 and 50000 elements, ldd = rows + 3,
    into a NaN-filled dst: every element to 4 eps of NumpyOps.batched_copy, padding rows and gaps untouched, and a scale
    entry of exactly 0.0 under inv_norm gives 0"""
    dst0, src, idx, scl, items, spans = sc.copy_case()
    ref = dst0.copy()
    NumpyOps().batched_copy(ref, src, idx, scl, items, len(items), 0.7)
    dst = hip_ops.to_device(dst0)
    hip_ops.batched_copy(dst, hip_ops.to_device(src), hip_ops.to_device(idx), hip_ops.to_device(scl),
                         hip_ops.to_device(items), len(items), 0.7)
    sc.check_copy(dst0, hip_ops.to_host(dst), ref, items, spans)
