"""Two-point correlation functions on the device: the trace-dot kernel against numpy, the pass against exact diagonalisation,
free fermions and exact sum rules, gauge independence / read-only behaviour, the poison switch.  Only the product library is
loaded; references are computed on the host without it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import correlator_common as cc
from hubbardtn_amd import abi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- kernel -----------------------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.float64).copy()).cuda()


def _run_trdots(lib, A, B, items, n_out):
    dA, dB = _dev(A), _dev(B)
    n = len(items)
    dI = torch.from_numpy(items.view(np.uint8).copy()).cuda() if n else None
    scratch = torch.empty(2 * max(int(lib.htn_trdots_scratch_elems(n)), 1), dtype=torch.float64, device="cuda")
    out = torch.full((2 * max(n_out, 1),), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    abi.check(lib, lib.htn_block_trdots_z(dA.data_ptr(), dB.data_ptr(), dI.data_ptr() if n else None, n, out.data_ptr(), n_out,
                                          scratch.data_ptr(), st), "htn_block_trdots_z")
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.complex128)[:n_out].copy()


def _ragged_case(rng, n_out, shapes, per_out_empty=()):
    """items over a list of (rows, cols) shapes, leading dimensions larger than the extents, complex weights; every shape is
    used at least once, several items share a result, the results in per_out_empty get none"""
    A = rng.standard_normal(60000) + 1j * rng.standard_normal(60000)
    B = rng.standard_normal(60000) + 1j * rng.standard_normal(60000)
    targets = [o for o in range(n_out) if o not in per_out_empty]
    items = np.zeros(3 * len(shapes), dtype=abi.TRDOT_DT)
    pa = pb = 3
    ref = np.zeros(n_out, dtype=np.complex128)
    scale = np.zeros(n_out)
    for q in range(len(items)):
        r, c = shapes[q % len(shapes)]
        lda, ldb = r + int(rng.integers(0, 5)), c + int(rng.integers(0, 5))
        o = targets[int(rng.integers(0, len(targets)))] if q >= len(targets) else targets[q]
        w = complex(rng.standard_normal(), rng.standard_normal())
        items[q] = (pa, pb, r, c, lda, ldb, o, (0, 0, 0), w.real, w.imag)
        Ab = A[pa + np.arange(r)[:, None] + lda * np.arange(c)[None, :]]
        Bb = B[pb + np.arange(c)[:, None] + ldb * np.arange(r)[None, :]]
        ref[o] += w * np.sum(Ab * Bb.T)
        scale[o] += abs(w) * np.linalg.norm(Ab) * np.linalg.norm(Bb)
        pa += lda * c + 7
        pb += ldb * r + 5
    assert pa < len(A) and pb < len(B)
    return A, B, items, ref, scale


SHAPES = [(1, 1), (1, 37), (37, 1), (33, 17), (64, 64), (130, 5)]


@pytest.mark.parametrize("n_out,empty", [(1, ()), (40, (0, 7, 39))])
def test_block_trdots_kernel_against_numpy(n_out, empty):
    lib = abi.load_library()
    rng = np.random.default_rng(5 + n_out)
    A, B, items, ref, scale = _ragged_case(rng, n_out, SHAPES, empty)
    got = _run_trdots(lib, A, B, items, n_out)
    again = _run_trdots(lib, A, B, items, n_out)
    assert np.array_equal(got.view(np.float64), again.view(np.float64))            # bit-identical
    for o in range(n_out):
        if o in empty:
            assert got[o] == 0.0
    err = np.abs(got - ref)
    print("trdots max error / scale", float((err / np.maximum(scale, 1e-300)).max()))
    assert np.all(err <= 1e-13 * scale)


def test_block_trdots_kernel_without_items_writes_zeros():
    lib = abi.load_library()
    got = _run_trdots(lib, np.zeros(4, dtype=np.complex128), np.zeros(4, dtype=np.complex128), np.zeros(0, dtype=abi.TRDOT_DT), 5)
    assert np.array_equal(got, np.zeros(5, dtype=np.complex128))
    assert lib.htn_trdots_scratch_elems(0) >= 0 and lib.htn_trdots_scratch_elems(10) >= 10


# ---- the pass ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ed_ref():
    return {case: cc.ed_correlators(cc.ED_L, *cc.ED_CASES[case]) for case in cc.ED_CASES}


@pytest.mark.parametrize("case", list(cc.ED_CASES))
def test_all_kinds_against_exact_diagonalisation(hip_ops, ed_ref, case):
    E0, ref = ed_ref[case]
    eng = cc.ed_engine(hip_ops, case)
    assert abs(eng.energy - E0) < 1e-9
    cc.compare_with_ed(eng, ref)


# measured once with tests/correlator_common.free_fermion_deviations on the CPU baseline library (same run: L = 12, truncdim 200,
# 8 sweeps): the deviation of the truncated state from the closed forms
FREE_FERMION_CPU = {"hop": 2.7104e-6, "nn": 3.2667e-6, "ss": 1.8008e-6}


def test_free_fermions_against_the_closed_form(hip_ops):
    """U = 0, L = 12, half filling, truncdim 200: G against 2 sum_k phi_k(i) phi_k(j), nn and ss against their Wick contractions.
    The state is truncated, so the bound is measured, not derived: the CPU baseline library gives for the same run
        hop 2.7104e-6    nn 3.2667e-6    ss 1.8008e-6                              (FREE_FERMION_CPU)
    and ten times that is asserted here (the factor covers the different summation order of the two backends)."""
    dev = cc.free_fermion_deviations(hip_ops)
    print("free fermions: deviations", dev, "CPU baseline", FREE_FERMION_CPU)
    for k, d in dev.items():
        assert d <= 10.0 * FREE_FERMION_CPU[k], (k, d)


def test_sum_rules_with_blocks_beyond_one_tile(hip_ops):
    eng, bonds = cc.check_sum_rules(hip_ops, L=12, cap=40, target=(8, 2))
    assert max(max(b.values()) for b in bonds) == 40               # blocks larger than one 32 x 32 tile, no multiple of it


def test_gauge_independence_read_only_and_plan_cache_keys(hip_ops):
    cc.check_gauge_and_readonly(hip_ops)


_CHILD = """
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import correlator_common as cc
from hubbardtn_amd.device import HipOps
eng = cc.ed_engine(HipOps(0), "half")
print("RESULT " + json.dumps({k: eng.correlator(k).view(np.float64).tobytes().hex() for k in cc.KINDS}))
"""


def test_poison_switch_changes_no_bit(hip_ops):
    """HTN_DEBUG_POISON=1 (fresh child process) fills every pool block with NaN before it is handed out: a result that read
    memory nobody wrote would differ from the run without the switch (or be NaN); results without a contribution are written
    by the kernel, not assumed to be zero"""
    eng = cc.ed_engine(hip_ops, "half")
    plain = {k: eng.correlator(k) for k in cc.KINDS}
    env = dict(os.environ, HTN_DEBUG_POISON="1")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    poisoned = json.loads(line[7:])
    for k in cc.KINDS:
        got = np.frombuffer(bytes.fromhex(poisoned[k]), dtype=np.float64)
        assert np.all(np.isfinite(got)), k
        assert np.array_equal(got, np.ascontiguousarray(plain[k]).view(np.float64).reshape(-1)), k
