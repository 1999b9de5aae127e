"""Bond updates whose coupled-sector block is above 512 rows in both orientations, on the CPU baseline backend: the
planner stages such a block like any other non-QRCP block (mode A) instead of refusing it.  The product's planner and
sweep driver, the CPU library's Jacobi SVD on the staged descriptors."""
import numpy as np
import pytest

import tall_state as ts
from cpu_ops import CpuOps


@pytest.fixture(scope="module")
def cpu_ops():
    return CpuOps()


def test_update_of_a_bond_with_a_block_above_512_in_both_orientations(cpu_ops):
    eng = ts.centred_engine(cpu_ops, krylovdim=6, maxrestart=1)
    blocks = ts.coupled_blocks(eng, ts.I0)
    assert ts.largest_block(blocks) > 512          # the case under test, not a smaller block
    ref = ts.schmidt_reference(blocks)
    E0 = eng.update_bond(ts.I0, +1, "right", optimise=False, record=False, cutoff=0.0)
    assert np.isfinite(E0)
    ts.assert_spectrum_matches(eng.spectrum(ts.I0 + 1), ref)
    ts.assert_left_isometry(eng, ts.I0)
    # the centre now sits on site I0 + 1: an optimising update of the same bond is variational w.r.t. <theta|H|theta>
    E1 = eng.update_bond(ts.I0, -1, "left", optimise=True, record=False, cutoff=0.0)
    assert E1 <= E0 + 1e-10 * abs(E0), (E1, E0)
