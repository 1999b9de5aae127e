"""Two-site TDVP on the MI355X: the bodies of test_tdvp_cpu.py on the HIP library (the Krylov exponential is the device
driver htn_krylov_expm_z there), the trajectory of the quench against the CPU baseline library's, and the debug switches."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):          # (the file is also run as a script: the child processes of the last test)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import tdvp_common as tc                                 # noqa: E402

pytestmark = pytest.mark.gpu


def test_l2_is_exact(hip_ops):
    tc.body_l2_exact(hip_ops)


def test_conservation_and_trajectory_against_the_cpu_library(hip_ops):
    """test 2 on the device, and its trajectory (energy, d_i, echo per sweep) equals the CPU baseline library's to 1e-8"""
    from cpu_ops import CpuOps
    drift, gpu = tc.body_conservation(hip_ops)
    _, cpu = tc.body_conservation(CpuOps())
    worst = max(max(abs(a[0] - b[0]), np.abs(a[1] - b[1]).max(), abs(a[2] - b[2])) for a, b in zip(gpu, cpu))
    print("GPU drift", drift, "largest GPU - CPU difference along the trajectory", worst)
    assert worst <= 1e-8


def test_reversibility(hip_ops):
    tc.body_reversibility(hip_ops)


def test_second_order_against_ed(hip_ops):
    tc.body_second_order(hip_ops)


def test_imaginary_time_reaches_the_ground_state(hip_ops):
    tc.body_imaginary_time(hip_ops)


def test_log_norm_l2(hip_ops):
    tc.body_log_norm_l2(hip_ops)


def test_truncation(hip_ops):
    tc.body_truncation(hip_ops)


def test_spinful_mode(hip_ops):
    tc.body_spinful(hip_ops)


def test_refusals(hip_ops):
    tc.body_refusals(hip_ops)


def test_api_time_evolve(hip_ops):
    tc.body_api_time_evolve(hip_ops)


def _trajectory_hex():
    from hubbardtn_amd.device import HipOps
    _, traj = tc.body_conservation(HipOps(0), sweeps=6)
    out = []
    for E, d, echo in traj:
        out.append([float(E).hex()] + [float(x).hex() for x in d] + [float(echo.real).hex(), float(echo.imag).hex()])
    return out


def test_debug_switches_leave_the_trajectory_bit_identical():
    """HTN_DEBUG_POISON=1 (every pool block starts as NaN) and HTN_DEBUG_EVENT_WAITS=1 (event waits instead of record polling):
    the quench trajectory in fresh child processes, bit for bit"""
    runs = []
    for extra in ({}, {"HTN_DEBUG_POISON": "1"}, {"HTN_DEBUG_EVENT_WAITS": "1"}):
        env = dict(os.environ, **extra)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trajectory"], env=env, capture_output=True, text=True,
                           timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert runs[0] == runs[1], "HTN_DEBUG_POISON changed the bits"
    assert runs[0] == runs[2], "HTN_DEBUG_EVENT_WAITS changed the bits"


if __name__ == "__main__" and "--trajectory" in sys.argv:
    print(json.dumps(_trajectory_hex()))
