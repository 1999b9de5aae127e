"""Two-site energy variance on the MI355X: the gfx950 projection kernel (htn_block_nullproj_z) against numpy, and
htn_mps_variance on the HIP library against the dense ||(H - E) psi||^2 and against the CPU baseline library.  The bodies are
in variance_common.py.  `python tests/test_variance_gpu.py` is the child process of the poison test."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L16, CHI16 = 16, 64


def state16(ops):
    """L = 16, U = 4, grown to truncdim(64) by two two-site sweeps from a fixed random start; centre on site 0"""
    from hubbardtn_amd import engine, models, mps
    H = models.hamiltonian(models.OB_Sim([1.0], [4.0]), L16)
    bonds, tens = mps.random_mps(L16, (L16, 0), 4, seed=11)
    eng = engine.DMRG2(ops, H, bonds, tens, chi_full=CHI16, lanczos_tol=1e-10)
    eng.sweep()
    eng.sweep()
    return eng, H


def hexes(v):
    return {"site": [float(x).hex() for x in v.site], "bond": [float(x).hex() for x in v.bond], "energy": float(v.energy).hex(),
            "total": float(v.total).hex()}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from hubbardtn_amd.device import HipOps
    print("RESULT " + json.dumps(hexes(state16(HipOps(0))[0].variance())))
    sys.exit(0)

import variance_common as vc      # noqa: E402
from cpu_ops import CpuOps        # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng16(hip_ops):
    return state16(hip_ops)


def test_projection_kernel_against_numpy(hip_ops):
    vc.check_kernel(vc.hip_run(hip_ops))


def test_projection_kernel_removes_the_leak_of_an_inexact_isometry(hip_ops):
    vc.check_kernel_leak(vc.hip_run(hip_ops))


@pytest.mark.parametrize("kind", vc.KINDS)
def test_variance_is_exact_for_a_nearest_neighbour_mpo(hip_ops, kind):
    """test 1 of test_variance_cpu.py on the HIP library, same dense reference; measured on the CPU library: 1.3e-16
    (variance_common.EXACT_CPU_DEV), so the bar here is max(1e-12, 10 x 1.3e-16) = 1e-12"""
    dev = vc.check_exact(hip_ops, kind)
    assert dev <= max(1e-12, 10.0 * vc.EXACT_CPU_DEV), dev


def test_hip_and_cpu_library_agree_entry_by_entry(hip_ops, eng16):
    """both libraries run from the same uploaded L = 16, chi = 64 state; bar: 10 x the measured deviation
    (variance_common.HIP_CPU_DEV)"""
    from hubbardtn_amd import engine
    eng, H = eng16
    tensors = [eng.download_site(i) for i in range(L16)]
    bonds = [dict(b.dims) for b in eng.bonds]
    cpu = engine.DMRG2(CpuOps(), H, bonds, tensors, chi_full=CHI16)
    vh, vc_ = eng.variance(), cpu.variance()
    dev = max(float(np.abs(vh.site - vc_.site).max()), float(np.abs(vh.bond - vc_.bond).max()))
    print("variance HIP vs CPU library: total", vh.total, vc_.total, "max entry deviation", dev, "energy", vh.energy - vc_.energy)
    assert vh.total > 1e-8
    assert dev <= 10.0 * vc.HIP_CPU_DEV, dev


def test_second_call_repeats_the_first_bit_for_bit(hip_ops, eng16):
    eng, _ = eng16
    a, b = eng.variance(), eng.variance()
    assert hexes(a) == hexes(b)


def test_poisoned_pool_gives_the_same_bits(hip_ops, eng16):
    """HTN_DEBUG_POISON=1 in a child process: every block the pool hands out is NaN first; the results are the same bits"""
    env = dict(os.environ, HTN_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    assert json.loads(line[len("RESULT "):]) == hexes(eng16[0].variance())


def test_state_untouched_and_applied_state_on_the_device(hip_ops):
    vc.check_untouched(hip_ops)
    vc.check_applied(hip_ops, "U1U1")
