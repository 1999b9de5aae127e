"""Local operators applied to a finite MPS on the device: the block-placement kernel against numpy bit for bit, applied states
against the library's correlators and exact diagonalisation, canonical form, the all-sites transition pass, G(x, t) against ED
time evolution, refusals, plan-cache hygiene, the poison switch.  Only the product library is loaded; the bodies are in
applyop_common.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import applyop_common as ac
from hubbardtn_amd import abi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. kernel --------------------------------------------------------------------------------------------------------------------------
def _place_case(rng):
    """one launch: 1 x 1, 1 x 37, 37 x 1, 33 x 31 with both leading dimensions larger than the rows, 300 x 257 (many tiles,
    ragged edges), 200 small items, zero-fill items, negative and zero coefficients; views are disjoint with gaps between them"""
    shapes = [(1, 1), (1, 37), (37, 1), (33, 31), (300, 257)] + [(int(rng.integers(1, 6)), int(rng.integers(1, 6))) for _ in range(200)] \
        + [(1, 1), (40, 3), (65, 33)]
    coefs = list(rng.standard_normal(len(shapes)))
    coefs[1], coefs[2], coefs[3], coefs[5], coefs[6] = -1.5, 0.0, -0.25, 0.0, -2.0
    zero_fill = {4 + k for k in range(3, 200, 7)} | {len(shapes) - 3, len(shapes) - 2, len(shapes) - 1}
    items = np.zeros(len(shapes), dtype=abi.PLACE_DT)
    pd, ps = 5, 3
    for q, (r, c) in enumerate(shapes):
        ldd, lds = r + int(rng.integers(1, 6)), r + int(rng.integers(1, 4))
        items[q] = (pd, -1 if q in zero_fill else ps, r, c, ldd, lds, coefs[q], (0,) * 6)
        pd += ldd * c + 3
        ps += lds * c + 2
    src = rng.standard_normal(ps + 8) + 1j * rng.standard_normal(ps + 8)
    return items, src, pd + 8


def _run_place(lib, items, src, n_dst):
    d_src = torch.from_numpy(src.view(np.float64).copy()).cuda()
    d_dst = torch.full((2 * n_dst,), float("nan"), dtype=torch.float64, device="cuda")
    d_it = torch.from_numpy(items.view(np.uint8).copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    abi.check(lib, lib.htn_block_place_z(d_dst.data_ptr(), d_src.data_ptr(), d_it.data_ptr(), len(items), st), "htn_block_place_z")
    torch.cuda.synchronize()
    return d_dst.cpu().numpy().view(np.complex128).copy()


def test_block_place_kernel_against_numpy_bit_exact():
    lib = abi.load_library()
    items, src, n_dst = _place_case(np.random.default_rng(17))
    got = _run_place(lib, items, src, n_dst)
    again = _run_place(lib, items, src, n_dst)
    assert got.tobytes() == again.tobytes()
    inside = np.zeros(n_dst, dtype=bool)
    for it in items:
        r, c = int(it["rows"]), int(it["cols"])
        idx = int(it["dst_off"]) + np.arange(r)[:, None] + int(it["ldd"]) * np.arange(c)[None, :]
        assert not inside[idx].any()                                                  # (the case's views are disjoint)
        inside[idx] = True
        if it["src_off"] < 0:
            want_re = want_im = np.zeros((r, c))
        else:
            s = src[int(it["src_off"]) + np.arange(r)[:, None] + int(it["lds"]) * np.arange(c)[None, :]]
            want_re, want_im = float(it["coef"]) * s.real, float(it["coef"]) * s.imag      # coef is real: one rounding per component
        g = got[idx]
        assert np.all(np.isfinite(g.real)) and np.all(np.isfinite(g.imag))
        assert np.array_equal(g.real, want_re) and np.array_equal(g.imag, want_im), (r, c)
    assert np.all(np.isnan(got[~inside].real)) and np.all(np.isnan(got[~inside].imag))   # nothing outside the views is written
    assert lib.htn_block_place_z(None, None, None, 0, None) == 0                          # n_items = 0: a no-op that succeeds


# ---- 2 .. 8 -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ed_ref():
    return ac.EdParticle()


@pytest.mark.parametrize("kind", ac.KINDS)
def test_overlaps_of_applied_states_are_the_correlators(hip_ops, kind):
    ac.check_against_correlators(hip_ops, kind)


@pytest.mark.parametrize("kind", ("su2", "u1"))
def test_applied_states_against_exact_diagonalisation(hip_ops, ed_ref, kind):
    ac.check_against_ed(hip_ops, kind, ed_ref)


@pytest.mark.parametrize("kind", ac.KINDS)
def test_result_is_canonical_and_keeps_its_norm(hip_ops, kind):
    ac.check_canonical(hip_ops, kind)


@pytest.mark.parametrize("kind", ac.KINDS)
def test_transition_equals_the_overlaps_in_any_gauge_and_reads_only(hip_ops, kind):
    ac.check_transition(hip_ops, kind)


def test_transition_with_blocks_beyond_one_tile(hip_ops):
    """L = 8 at a bond cap of 64 in `dim` units (blocks that are no multiple of the 32 x 32 tiles of the placement and trace-dot
    kernels, a truncated state): the pass against the L overlaps of the applied states"""
    from hubbardtn_amd import engine, models, mps
    L = 8
    H = models.hamiltonian(models.OB_Sim([1.0], [4.0]), L)
    bonds, tens = mps.random_mps(L, (L, 0), 8, seed=7)
    eng = engine.DMRG2(hip_ops, H, bonds, tens, chi_full=64, lanczos_tol=1e-12)
    for _ in range(3):
        eng.sweep()
    ket = eng.copy()
    ket.move_centre(3)
    ket = ket.apply_op(3, "c+")
    ref = np.array([a.overlap(ket) for a in ac.applied_states(eng, "c+")])
    got = eng.transition("c+", ket)
    d = float(np.abs(got - ref).max())
    print("transition L = 8, chi 64: max deviation", d, "scale", float(np.abs(ref).max()))
    assert d <= 1e-12 and np.abs(ref).max() > 0.1


def test_greens_function_against_ed_time_evolution(hip_ops, ed_ref):
    """L = 6, U = 4, half filling, c+ on site 2, t = 0 .. 1 in steps of 0.05, nothing truncated, TDVP tolerance 1e-10: the CPU
    baseline library gives max |C - C_ED| = 1.24e-10 (applyop_common.GREENS_CPU_DEV, test_applyop_cpu.py prints it); the HIP
    library runs the same host decisions with another summation order and must stay below max(1e-9, 10 x that value)."""
    ac.check_greens(hip_ops, ed_ref, max(1e-9, 10.0 * ac.GREENS_CPU_DEV))


def test_refusals_leave_the_source_usable(hip_ops):
    from hubbardtn_amd.device import HipOps
    ac.check_refusals(hip_ops, lambda: HipOps(0))


def test_sweep_after_the_new_calls_plans_what_it_planned_without_them(hip_ops):
    ac.check_cache_hygiene(hip_ops)


_CHILD = """
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import applyop_common as ac
from hubbardtn_amd.device import HipOps
eng = ac.ground_engine(HipOps(0), "su2")
ket = ac.evolved_ket(eng, "c+")
print("RESULT " + json.dumps(eng.transition("c+", ket).view(np.float64).tobytes().hex()))
"""


def test_poison_switch_leaves_the_transition_finite_and_equal(hip_ops):
    """HTN_DEBUG_POISON=1 (fresh child process): every pool block is NaN before it is handed out, so a placement that left a
    sub-block unwritten, or a pairing that read one, would show"""
    eng = ac.ground_engine(hip_ops, "su2")
    plain = eng.transition("c+", ac.evolved_ket(eng, "c+"))
    env = dict(os.environ, HTN_DEBUG_POISON="1")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    got = np.frombuffer(bytes.fromhex(json.loads(line[7:])), dtype=np.complex128)
    print("poisoned pool: max deviation of the transition amplitudes", float(np.abs(got - plain).max()))
    assert np.all(np.isfinite(got.view(np.float64))) and np.array_equal(got, plain)
