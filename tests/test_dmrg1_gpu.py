"""One-site DMRG on the HIP library: the batched QR / LQ kernel (htn_qr_blocks_z) against numpy's Householder QR, the
one-site sweep against exact diagonalisation and against the CPU baseline library from the same uploaded state, and a
poisoned-pool child process that must reproduce a sweep bit for bit.

Bars of the kernel cases: 10 x what numpy.linalg.qr (LAPACK Householder) leaves on the same input, floor 256 eps (the
convention of test_krylov_steps_gpu.py); the 12-decade blocks must meet the orthogonality bar of a well-conditioned block of
their shape.  The R buffer holds a sentinel before every call, so what the kernel writes and what it leaves alone both show."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dmrg1_common as d1
import qr_cases as qc
from hubbardtn_amd import abi, engine, models, mps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_sweep1():
    """the child's workload: grow L = 16 to chi 64 with two-site sweeps, then two one-site sweeps -> hex floats"""
    from hubbardtn_amd.device import HipOps
    ops = HipOps(0)
    L = 16
    H = models.hamiltonian(models.OB_Sim([1.0, 0.1], [4.0]), L)            # range 2: the Z stage of the one-site apply runs
    bonds, tens = mps.random_mps(L, (L, 0), 4, seed=11)
    eng = engine.DMRG2(ops, H, bonds, tens, chi_full=64, lanczos_tol=1e-11)
    E2 = [float(eng.sweep()) for _ in range(2)]
    E1 = [float(eng.sweep1()) for _ in range(2)]
    site = eng.site_vector(0)
    return {"E2": [e.hex() for e in E2], "E1": [e.hex() for e in E1],
            "ritz": [float(s.energy).hex() for s in eng.stats[-(2 * L - 2):]],
            "site0": [float(x).hex() for x in np.concatenate([site.real, site.imag])[:64]]}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    print("RESULT " + json.dumps(run_sweep1()))
    sys.exit(0)


pytestmark = pytest.mark.gpu
CASES = qc.cases()


def _run_qr(ops, mats, trans):
    flat, desc, rsize = qc.pack(mats, trans)
    A = ops.to_device(flat)
    R = ops.to_device(np.full(rsize, qc.R_SENTINEL))          # not zeros: what the kernel does not write must show
    dd = ops.to_device(desc)
    ops.qr_blocks(A, R, dd, desc, len(mats))
    ops.sync()
    return ops.to_host(A), ops.to_host(R), desc


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_qr_blocks_against_numpy(hip_ops, name, trans):
    """Every case of qr_cases.py (panel widths 16 .. 1 with their boundary row counts, up to three projection rounds, graded
    and dependent columns) against the bars of the module's head; R's zero triangle written by the kernel, its padding and
    the gaps between blocks untouched (qc.check_padding); exact zeros on R's diagonal at the planted dependent columns.
    Measured on the MI355X, orthogonality / residual of the kernel (every bar is the floor, 256 eps = 5.7e-14; LAPACK's own
    figures in brackets): 7664 x 21 at w = 1: 4.4e-16 / 1.1e-16 (8.9e-16 / 3.4e-16); 3825 x 140 at w = 1, two rounds:
    6.7e-16 / 1.3e-16 (6.7e-16 / 7.0e-16); 12 decades, 1000 x 40 at w = 4: 4.4e-16 / 3.3e-16 (6.7e-16 / 7.8e-16) and
    2000 x 30 at w = 2: 4.4e-16 / 2.8e-16 (1.1e-15 / 5.0e-16).  The slowest case, 3825 x 140, takes 0.3 s with both runs."""
    mats = CASES[name]
    flat, rflat, desc = _run_qr(hip_ops, mats, trans)
    qc.check(name, trans, mats, flat, rflat, desc, well_conditioned_orth_bar=qc.orth_bar(name, mats))
    flat2, rflat2, _ = _run_qr(hip_ops, mats, trans)
    assert flat.tobytes() == flat2.tobytes() and rflat.tobytes() == rflat2.tobytes(), "two runs differ in bits"


def test_qr_blocks_refuses_bad_descriptors(hip_ops):
    flat, desc, rsize = qc.pack([np.ones((5, 3), dtype=np.complex128)], 0)
    desc[0]["m"], desc[0]["n"] = 3, 5
    with pytest.raises(abi.HtnError, match="m >= n"):
        hip_ops.qr_blocks(hip_ops.to_device(flat), hip_ops.zeros_z(64), hip_ops.to_device(desc), desc, 1)


@pytest.mark.parametrize("shapes", [[(abi.QR_MAX_M + 1, 4)], [(10, 4), (abi.QR_MAX_M + 1, 4)]], ids=["alone", "second_of_two"])
@pytest.mark.parametrize("trans", [0, 1])
def test_qr_blocks_refuses_a_block_above_the_row_limit(hip_ops, shapes, trans):
    """m = HTN_QR_MAX_M + 1 with valid buffers: refused with the row limit in the message, and nothing is launched -- A and
    R are bit-identical afterwards, also for the block before the one that is too tall"""
    rng = np.random.default_rng(77)
    flat, desc, rsize = qc.pack([rng.normal(size=s) + 1j * rng.normal(size=s) for s in shapes], trans)
    A, R = hip_ops.to_device(flat), hip_ops.to_device(np.full(rsize, qc.R_SENTINEL))
    with pytest.raises(abi.HtnError, match=rf"{abi.QR_MAX_M + 1} rows.*holds {abi.QR_MAX_M}\b"):
        hip_ops.qr_blocks(A, R, hip_ops.to_device(desc), desc, len(shapes))
    hip_ops.sync()
    assert hip_ops.to_host(A).tobytes() == flat.tobytes(), "A was written by a refused call"
    assert np.all(hip_ops.to_host(R) == qc.R_SENTINEL), "R was written by a refused call"


@pytest.mark.parametrize("symname", d1.SYMS)
def test_one_site_sweeps_converge_to_exact_diagonalisation(hip_ops, symname):
    e = d1.loose_state(hip_ops, symname)
    before = d1.tables(e)
    E, ritz = d1.converge_onesite(e)
    ref = d1.ed_energy(symname)
    print(symname, "E", repr(E), "ED", repr(ref), "diff", abs(E - ref), "updates", len(ritz))
    assert all(b <= a + 1e-12 for a, b in zip(ritz, ritz[1:])), "a Ritz value rose"
    assert abs(E - ref) <= 1e-10
    assert d1.tables(e) == before and e.centre() == 0
    assert d1.isometry_defects(e) <= 1e-12
    assert abs(e.bond_energies()[0] - E) <= 1e-10


def test_gauge_moves_on_tall_blocks_keep_the_state(hip_ops):
    """tall_state's L = 14 chain at its cap of 150 per sector (the largest factorised block has m = 600 rows: panel width 8):
    the centre goes from site I0 to the right end and back to site 0 by update_site(optimise=False).  Every returned
    <x|H_eff|x> equals the first to 1e-11 relative, the left isometries at the turning point and the right ones at the end
    are orthonormal to 1e-12, |<moved|untouched twin>| = 1 to 1e-12, and a second run leaves the same bits on site I0."""
    import tall_state as ts
    e = d1.assert_tall_gauge_round_trip(hip_ops)
    e2, _, _ = d1.tall_gauge_round_trip(hip_ops)
    assert e.site_vector(ts.I0).tobytes() == e2.site_vector(ts.I0).tobytes(), "two runs differ in bits"


@pytest.fixture(scope="module")
def uploaded_state():
    """L = 16, chi = 64 grown on the CPU library and downloaded: both libraries start from these tensors"""
    from cpu_ops import CpuOps
    cpu = CpuOps()
    L = 16
    H = models.hamiltonian(models.OB_Sim([1.0], [4.0]), L)
    bonds, tens = mps.random_mps(L, (L, 0), 4, seed=21)
    g = engine.DMRG2(cpu, H, bonds, tens, chi_full=64, lanczos_tol=1e-8)
    for _ in range(2):
        g.sweep()
    return cpu, H, d1.tables(g), [g.download_site(i) for i in range(L)]


def test_hip_and_cpu_libraries_agree_from_the_same_state(hip_ops, uploaded_state):
    cpu, H, bonds, tens = uploaded_state
    a = engine.DMRG2(hip_ops, H, bonds, tens, chi_full=64, lanczos_tol=1e-12)
    b = engine.DMRG2(cpu, H, bonds, tens, chi_full=64, lanczos_tol=1e-12)
    n = a.site_vector(0).size
    rng = np.random.default_rng(3)
    x = rng.normal(size=n) + 1j * rng.normal(size=n)
    ya, yb = a.apply_heff1(0, x), b.apply_heff1(0, x)
    rel = np.linalg.norm(ya - yb) / np.linalg.norm(yb)
    Ea, Eb = a.sweep1(), b.sweep1()
    print("heff1 rel", rel, "E hip", repr(Ea), "E cpu", repr(Eb), "diff", abs(Ea - Eb))
    assert rel <= 1e-12
    assert abs(Ea - Eb) <= 1e-9


def test_poisoned_pool_reproduces_the_one_site_sweep_bit_for_bit(hip_ops):
    base = run_sweep1()
    env = dict(os.environ)
    env["HTN_DEBUG_POISON"] = "1"
    env["PYTHONPATH"] = ROOT + os.pathsep + os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    other = json.loads(line[len("RESULT "):])
    assert all(np.isfinite(float.fromhex(x)) for x in other["E1"] + other["ritz"])
    assert other == base
