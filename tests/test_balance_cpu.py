"""The launch balancer of the grouped GEMM (htn_balance_tiles: spatial and split-K tile cuts, placement-aware order) checked on
the host through the CPU baseline library: what it returns must be the same work as what it was given -- every output element
covered once, every K slab of a cut tile in exactly one part, a workspace slab range of its own per cut tile -- and, tile for
tile, what the library returned when tests/golden/plan_digests.json was written."""
import json
import os

import numpy as np
import pytest

import gemm_cases as gc
from cpu_ops import CpuOps
from emul import NumpyOps

GEOMETRY = ("c_off", "buf_c", "ldc", "m", "n", "row0", "col0", "seg_begin", "seg_count", "pad0", "pad1")
TILE = 32


@pytest.fixture(scope="module")
def cpu_ops():
    return CpuOps()


@pytest.fixture(scope="module")
def problems():
    """per case: the list, its operands and the emulator's result of the list as planned -- computed once, only read"""
    out = {}
    for case in gc.SPLIT_CASES + [gc.WHOLE_CASE]:
        rng, tasks, out_size = gc.case_tasks(case)
        src0 = rng.standard_normal(gc.NEL) + 1j * rng.standard_normal(gc.NEL)
        src2 = rng.standard_normal(gc.NEL) + 1j * rng.standard_normal(gc.NEL)
        ref = np.zeros(out_size, dtype=np.complex128)
        emu = NumpyOps()
        emu.grouped_gemm([src0, ref, src2] + [None] * 5, emu.upload_tasks(tasks))
        out[case] = (tasks, src0, src2, ref)
    return out


def _source_of(tiles_in):
    """(buf_c, c_off, tile row, tile column) -> input tile: the planner's tiles start at multiples of the tile edge"""
    return {(int(t["buf_c"]), int(t["c_off"]), int(t["row0"]) // TILE, int(t["col0"]) // TILE): t for t in tiles_in}


def _check_same_work(tiles_in, out, slots):
    src = _source_of(tiles_in)
    assert len(src) == len(tiles_in)
    # the rectangles of the parts with part == 0 tile every input tile, hence every block, exactly once
    cover = {k: np.zeros((int(t["m"]), int(t["n"])), dtype=np.int32) for k, t in src.items()}
    groups = {}
    for t in out:
        k = (int(t["buf_c"]), int(t["c_off"]), int(t["row0"]) // TILE, int(t["col0"]) // TILE)
        s = src[k]
        assert int(t["ldc"]) == int(s["ldc"]) and int(t["pad1"]) == int(s["pad1"])
        r0, c0 = int(t["row0"]) - int(s["row0"]), int(t["col0"]) - int(s["col0"])
        assert r0 >= 0 and c0 >= 0 and r0 + int(t["m"]) <= int(s["m"]) and c0 + int(t["n"]) <= int(s["n"])
        if int(t["part"]) == 0:
            cover[k][r0:r0 + int(t["m"]), c0:c0 + int(t["n"])] += 1
        if int(t["nparts"]) > 1:
            groups.setdefault(int(t["ticket"]), []).append(t)
        else:
            assert int(t["part"]) == 0
            assert (int(t["seg_begin"]), int(t["seg_count"]), int(t["pad0"])) == (int(s["seg_begin"]), int(s["seg_count"]), int(s["pad0"]))
    for c in cover.values():
        assert (c == 1).all()
    # the parts of one ticket: one rectangle, the GEMM segments of its tile in order and without gaps, the COPY segments
    # with the last part; a workspace slab range per ticket, disjoint from every other
    ranges = []
    for ticket, parts in groups.items():
        parts.sort(key=lambda t: int(t["part"]))
        np_ = int(parts[0]["nparts"])
        assert [int(t["part"]) for t in parts] == list(range(np_))
        rect = {tuple(int(t[f]) for f in ("buf_c", "c_off", "row0", "col0", "m", "n", "nparts", "ws_slot")) for t in parts}
        assert len(rect) == 1
        s = src[(int(parts[0]["buf_c"]), int(parts[0]["c_off"]), int(parts[0]["row0"]) // TILE, int(parts[0]["col0"]) // TILE)]
        pos = int(s["seg_begin"])
        for t in parts[:-1]:
            assert int(t["seg_begin"]) == pos and int(t["pad0"]) == 0 and int(t["seg_count"]) >= 0
            pos += int(t["seg_count"])
        last = parts[-1]
        assert int(last["seg_begin"]) == pos and int(last["pad0"]) == int(s["pad0"])
        assert pos + int(last["seg_count"]) == int(s["seg_begin"]) + int(s["seg_count"])
        assert int(last["seg_count"]) >= int(last["pad0"])
        ranges.append((int(parts[0]["ws_slot"]), np_))
    ranges.sort()
    for (a, na), (b, _) in zip(ranges, ranges[1:]):
        assert a + na <= b
    assert all(a >= 0 for a, _ in ranges) and slots == sum(n for _, n in ranges)


@pytest.mark.parametrize("n_cus", gc.N_CUS + (100,))
@pytest.mark.parametrize("case", gc.SPLIT_CASES)
def test_long_tiles_are_cut_into_the_same_work(cpu_ops, problems, case, n_cus):
    """256 CUs: eight XCD queues; 100 and 7 are no multiple of 8: one queue.  A K cut needs a tile longer than 1.25 x the
    balanced share of a CU (balance_tiles, cap_k): with 7 CUs that share is a seventh of the whole list, which no tile of
    these lists reaches, so there only the spatial cut shows; 100 CUs give K parts on the one-queue path."""
    tasks, src0, src2, ref = problems[case]
    tiles_in = tasks.tiles[:tasks.ntiles]
    out, slots = gc.balance(cpu_ops.lib, tiles_in, n_cus)
    assert len(out) > len(tiles_in)                                               # something was split
    if n_cus != 7:
        assert int(out["nparts"].max()) >= 2 and slots > 0
    _check_same_work(tiles_in, out, slots)
    # the numpy emulator on the balanced list agrees with the list as planned
    chk = np.zeros_like(ref)
    NumpyOps().grouped_gemm([src0, chk, src2] + [None] * 5, (out, len(out), tasks.segs))
    assert np.abs(chk - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("n_cus", gc.N_CUS)
def test_short_tiles_stay_whole(cpu_ops, problems, n_cus):
    tasks, src0, src2, ref = problems[gc.WHOLE_CASE]
    tiles_in = tasks.tiles[:tasks.ntiles]
    out, slots = gc.balance(cpu_ops.lib, tiles_in, n_cus)
    assert slots == 0 and len(out) == len(tiles_in) and int(out["nparts"].max()) == 1 and not out["part"].any()
    rows = lambda a: sorted(tuple(int(t[f]) for f in GEOMETRY) for t in a)
    assert rows(out) == rows(tiles_in)                                            # a permutation of the input
    _check_same_work(tiles_in, out, slots)
    chk = np.zeros_like(ref)
    NumpyOps().grouped_gemm([src0, chk, src2] + [None] * 5, (out, len(out), tasks.segs))
    assert np.abs(chk - ref).max() <= 1e-12 * np.abs(ref).max()


def test_balanced_lists_are_what_the_golden_digests_pin(cpu_ops):
    """the three random lists and the H_eff apply lists of two short chains, balanced for 256 and 7 CUs: SHA-256 of the tile
    records (integers only) against tests/golden/plan_digests.json (tests/golden/make_plan_digests.py)"""
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "plan_digests.json")))
    got = gc.plan_digests(cpu_ops)
    assert sorted(got) == sorted(gold)
    assert [k for k in gold if got[k] != gold[k]] == []
