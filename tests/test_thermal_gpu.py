"""Finite temperature on the MI355X: the bodies of test_thermal_cpu.py on the HIP library, with the same bounds, against dense
grand-canonical exact diagonalisation (not against the CPU run)."""
import pytest

import thermal_common as th

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("L", [3, 4])
@pytest.mark.parametrize("mode,case", th.COMBOS)
def test_beta_zero_is_exact(hip_ops, mode, case, L):
    th.body_beta0(hip_ops, mode, case, L)


@pytest.mark.parametrize("L", [3, 4])
@pytest.mark.parametrize("mode,case", th.COMBOS)
def test_cooling_without_truncation_against_ed(hip_ops, mode, case, L):
    th.body_cooling(hip_ops, mode, case, L)


def test_small_steps_keep_both_seed_sweeps(hip_ops):
    th.body_small_steps(hip_ops)


def test_continuation(hip_ops):
    th.body_continuation(hip_ops)


def test_truncating_run(hip_ops):
    th.body_truncating(hip_ops)


def test_refusals(hip_ops):
    from hubbardtn_amd.device import HipOps
    th.body_refusals(hip_ops, lambda: HipOps(0))
