"""One-site TDVP on the HIP library: the bodies of test_tdvp1_cpu.py with the same gates (the zero-site apply runs on the grouped
GEMM kernel, the backward step on the Krylov exponential's kernels), the HIP library against the CPU baseline library from the
same uploaded L = 16, chi = 64 state, two runs bit for bit, and a poisoned-pool child process that must reproduce them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tdvp1_common as t1
from hubbardtn_amd import engine, models, mps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grown_state(ops):
    """L = 16 grown to chi = 64 by two two-site sweeps under a range-2 Hamiltonian (the Z stage of both applies runs)"""
    L = 16
    H = models.hamiltonian(models.OB_Sim([1.0, 0.1], [4.0]), L)
    bonds, tens = mps.random_mps(L, (L, 0), 4, seed=11)
    eng = engine.DMRG2(ops, H, bonds, tens, chi_full=64, lanczos_tol=1e-11)
    for _ in range(2):
        eng.sweep()
    return eng


def run_tdvp1():
    """the child's workload: two one-site TDVP sweeps of the grown state and one zero-site apply -> hex floats"""
    from hubbardtn_amd.device import HipOps
    eng = grown_state(HipOps(0))
    eng.krylovdim, eng.lanczos_tol, eng.maxrestart = 30, 1e-12, 8
    E = [float(eng.tdvp1_sweep(0.05)) for _ in range(2)]
    recs = eng.stats[-(2 * eng.L - 2):]
    eng.evolve_site_move(0, +1, 0.025, -0.025)
    n0 = eng.bond_size(1)
    y = eng.apply_heff0(1, np.arange(1, n0 + 1) * (1.0 - 0.5j))
    site = eng.site_vector(0)
    return {"E": [e.hex() for e in E], "alpha": [float(s.energy).hex() for s in recs], "matvecs": [s.n_matvec for s in recs],
            "log_norm": float(eng.log_norm).hex(), "y": [float(v).hex() for v in np.concatenate([y.real, y.imag])],
            "site0": [float(x).hex() for x in np.concatenate([site.real, site.imag])[:64]]}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    print("RESULT " + json.dumps(run_tdvp1()))
    sys.exit(0)


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", t1.CASES)
def test_heff0_is_heff1_between_the_isometries(hip_ops, case):
    t1.body_heff0_identity(hip_ops, case)


def test_heff0_on_sectors_wider_than_one_quadrant(hip_ops):
    t1.body_heff0_identity(hip_ops, "SU2U1", chi=300, sweeps=2, wider_than=16)


def test_energy_norm_and_tables_are_conserved_under_a_cap(hip_ops):
    t1.body_conservation(hip_ops)


def test_a_step_is_reversible(hip_ops):
    t1.body_reversibility(hip_ops)


def test_splitting_error_against_exact_diagonalisation(hip_ops):
    """the gate comes from the CPU baseline library's figures (tdvp1_common.CPU_ED_ERRORS), not from this run"""
    t1.check_ed_errors(t1.ed_errors(hip_ops))


def test_imaginary_time_reaches_the_one_site_dmrg_energy(hip_ops):
    t1.body_imaginary_time(hip_ops)


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
    return cpu, H, t1.tables(g), [g.download_site(i) for i in range(L)]


def test_hip_and_cpu_libraries_agree_from_the_same_state(hip_ops, uploaded_state):
    """zero-site apply on the middle bond to 1e-13 relative, one sweep of dt = 0.05: energy to 1e-12, overlap of the two results
    to 1e-10"""
    cpu, H, bonds, tens = uploaded_state

    def fresh(ops):
        return engine.DMRG2(ops, H, bonds, tens, chi_full=64, krylovdim=30, lanczos_tol=1e-12, maxrestart=8)
    # The zero-site apply needs a left environment, i.e. gauge moves, and the QR of a centre is only as reproducible between two
    # libraries as the centre is well conditioned (a capped state is not).  So the CPU library carries the centre to site k
    # first and BOTH libraries start from that download: sites 0 .. k-1 are isometries, every QR on the way to site k factors an
    # isometry (R = 1) and reproduces it to rounding.  The right environment of bond k is the one the constructor built from
    # the uploaded tensors, with the centre on site k in the place of a right isometry: not a physical environment, but the
    # same numbers in both libraries, which is what a comparison of the two applies needs.
    k = 8
    pre = fresh(cpu)
    for i in range(k):
        pre.update_site(i, +1, optimise=False, record=False)
    moved = [pre.download_site(i) for i in range(pre.L)]

    def at_k(ops):
        e = engine.DMRG2(ops, H, bonds, moved, chi_full=64, krylovdim=30, lanczos_tol=1e-12, maxrestart=8)
        for i in range(k):
            e.update_site(i, +1, optimise=False, record=False)
        return e
    a, b = at_k(hip_ops), at_k(cpu)
    n0 = b.bond_size(k)
    assert n0 >= 32 and len(b.bond(k).dims) >= 6              # (several sectors of different dimensions)
    rng = np.random.default_rng(3)
    x = rng.normal(size=n0) + 1j * rng.normal(size=n0)
    ya, yb = a.apply_heff0(k, x), b.apply_heff0(k, x)
    rel = np.linalg.norm(ya - yb) / np.linalg.norm(yb)
    a, b = fresh(hip_ops), fresh(cpu)
    Ea, Eb = a.tdvp1_sweep(0.05), b.tdvp1_sweep(0.05)
    down = engine.DMRG2(cpu, H, t1.tables(a), [a.download_site(i) for i in range(a.L)], chi_full=64)
    ov = abs(down.overlap(b))
    print("heff0 rel", rel, "E hip", repr(Ea), "E cpu", repr(Eb), "diff", abs(Ea - Eb), "1 - overlap", 1.0 - ov)
    assert rel <= 1e-13
    assert abs(Ea - Eb) <= 1e-12
    assert 1.0 - ov <= 1e-10


def test_two_runs_and_a_poisoned_pool_agree_bit_for_bit(hip_ops):
    base = run_tdvp1()
    assert run_tdvp1() == base, "two runs differ in bits"
    env = dict(os.environ)
    env["HTN_DEBUG_POISON"] = "1"
    env["PYTHONPATH"] = ROOT + os.pathsep + os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    other = json.loads(line[len("RESULT "):])
    assert all(np.isfinite(float.fromhex(v)) for v in other["E"] + other["alpha"] + other["y"])
    assert other == base
