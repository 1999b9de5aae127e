"""The cases of tests/svd_large_cases.py on a machine without a GPU and without the library: every case builds and its
EXPECT row holds (asserted when the module is imported), its truth converges and is affordable, and the stopping rule the
multi-workgroup paths used is shown to be wrong on a cluster by the complex128 twin of the truth loop."""
import time

import numpy as np
import pytest

import svd_large_cases as lc


def test_every_case_is_on_its_path():
    """the geometry rules restated in svd_large_cases.geometry() put every block where EXPECT says, and the same shapes
    without the test mode / the host descriptors / the QRCP flag would not be there"""
    for name in lc.SHAPE_CALLS:
        for b, ((shape, split), want) in zip(lc.CALLS[name].blocks, lc.EXPECT[name]):
            assert b.M.shape == shape and b.instance() == want
            assert lc.geometry(b.kind, shape, split, host=False)[0] == "one"
    assert lc.geometry("qrcp", (40, 40))[0] == "one" and lc.geometry("qrcp", (41, 50))[0] == "one"
    assert lc.geometry("plain", (512, 19))[0] == "one" and lc.geometry("plain", (513, 2))[0] == "tall"
    # the switch of the ring's lane groups, and the window: 96 x 96 fills it exactly
    assert lc.geometry("qrcp", (40, 256))[1] == 16 and lc.geometry("qrcp", (36, 257))[1] == 64
    assert lc.geometry("qrcp", (97, 96))[0] == "one" and lc.geometry("qrcp", (96, 97))[0] == "ring"
    assert set(lc.RING_CALLS) | {n for n in lc.CALLS if n.endswith("tall")} == set(lc.CALLS)
    for spec in lc.SPECTRA:
        assert any(n.startswith(spec + "_") for n in lc.SPECTRUM_CALLS), spec


@pytest.mark.parametrize("name", list(lc.CALLS))
def test_truth_converges_and_is_affordable(name):
    t0 = time.time()
    for b in lc.CALLS[name].blocks:
        t1 = time.time()
        ref, sig, bar = lc.ref_of(b)
        print(f"{b.name} {b.M.shape} {b.instance()}: sigma_max {sig:.3e}, bar {bar:.3e}, truth {time.time() - t1:.2f} s")
        assert len(ref) == b.n and np.isfinite(ref.astype(np.float64)).all() and bar < 1e-12
        if b.rank is not None:
            assert int((ref > 1e-11 * sig).sum()) == b.rank if sig > 0 else b.rank == 0
    assert time.time() - t0 < 30.0, "the truths of one call must stay affordable"


@pytest.mark.parametrize("name", lc.CLUSTER_CALLS)
def test_old_rule_misses_the_bar_on_a_cluster_and_the_new_rule_meets_it(name):
    """s_i = 1 + i 1e-13 on every carrier.  A sweep sees squared cosines of 1e-24, far below 0.1 tol = 1e-15, and by the old
    rule (svd_large_cases.last_sweep_old) it is the last; but it rotated by angles of order one, which carry the cosines
    over at first order.  jacobi_last_sweep (last_sweep) also asks for tan^2 x mx <= tol^2 and goes on.  The twin is plain
    column-pair Jacobi in complex128, not the kernels' panel order or Gram visits: it shows the rule, not the kernels."""
    (b,) = lc.CALLS[name].blocks
    ref, sig, bar = lc.ref_of(b)
    old, sw_old = lc.twin_stopped(b, lc.last_sweep_old)
    new, sw_new = lc.twin_stopped(b, lc.last_sweep)
    dev_old, dev_new = float(np.abs(old - ref).max()) / sig, float(np.abs(new - ref).max()) / sig
    print(f"{b.name} {b.M.shape}: old rule {dev_old:.3e} in {sw_old} sweeps, new rule {dev_new:.3e} in {sw_new} sweeps, bar {bar:.3e}")
    assert dev_old > bar, "the old rule is not shown wrong by this case"
    assert dev_new <= bar and sw_new > sw_old


def test_rules_agree_off_the_clusters():
    """on the graded carriers, whose rotations are small once the cosines are, both rules stop at the same sweep: the new
    rule costs nothing there"""
    for name in lc.SPECTRUM_CALLS:
        if name.startswith("graded_"):
            (b,) = lc.CALLS[name].blocks
            (old, sw_old), (new, sw_new) = lc.twin_stopped(b, lc.last_sweep_old), lc.twin_stopped(b, lc.last_sweep)
            print(f"{b.name}: {sw_old} sweeps by the old rule, {sw_new} by the new")
            assert sw_old == sw_new and lc.same_bytes(old, new)


def test_twin_on_the_already_orthogonal_blocks():
    """what the GPU test asserts of an already orthogonal block -- one sweep, S to 4 eps of every entry -- is what plain
    double arithmetic allows: on the tall carrier directly, on the QRCP carrier after a pivoted QR in numpy
    (svd_large_cases.qrcp_twin), whose R^H is what the ring and the pair visits rotate"""
    seen = 0
    for name in lc.SPECTRUM_CALLS:
        if not name.startswith("orthogonal_"):
            continue
        (b,) = lc.CALLS[name].blocks
        d = np.sort(b.diag)[::-1]
        X = lc.qrcp_twin(b.M) if b.kind == "qrcp" else b.M
        got, sweeps = lc.hestenes(X, dtype=np.complex128, tol=lc.TOL, zero_rel=1e-15, max_sweeps=lc.MAX_SWEEPS)
        print(f"{b.name}: twin against the diagonal, worst {np.abs(got / d - 1).max() / lc.EPS:.2f} eps, sweeps {sweeps}")
        assert sweeps == 1 and np.all(np.abs(got - d) <= 4 * lc.EPS * d)
        seen += 1
    assert seen == 2        # (40, 40) with split = 1 and 600 x 24; the other carriers have more columns than rows


def test_twin_on_the_column_graded_tall_block():
    """B D, B 600 x 12 with unit columns, D over 12 decades: the twin's relative deviation is the yardstick of the GPU test"""
    (b,) = lc.CALLS["column_graded_tall"].blocks
    twin = lc.relative_deviation(lc.twin_of(b), b)
    lap = lc.relative_deviation(np.linalg.svd(b.M, compute_uv=False), b)
    print(f"column graded 600 x 12: twin {twin:.3e}, numpy.linalg.svd {lap:.3e} (relative, worst singular value)")
    assert twin <= 1e-10, "above this the twin is no yardstick"


def test_qrcp_twin_is_a_pivoted_qr():
    (b,) = lc.CALLS["graded_r16"].blocks
    X = lc.qrcp_twin(b.M)
    assert X.shape == (b.m, b.n)
    ref, sig, bar = lc.ref_of(b)
    assert np.abs(np.linalg.svd(X, compute_uv=False) - ref).max() <= bar * sig
    assert abs(np.linalg.norm(X) - np.linalg.norm(b.M)) <= 64 * lc.EPS * sig           # the QR preserves the Frobenius norm