"""TEST INFRASTRUCTURE: grouped-GEMM task lists shared by the kernel tests (tests/test_kernels_gpu.py), the tests of the launch
balancer (tests/test_balance_cpu.py) and the generator of their pinned digests (tests/golden/make_plan_digests.py)."""
import ctypes as C
import hashlib

import numpy as np

from hubbardtn_amd import abi, engine, models, mps
from ref_planner import EnvLayout, TaskList


def random_tasks(rng, nblocks, maxdim, maxk, nbuf_elems):
    """random grouped-GEMM problem exercising all ops, ragged sizes, COPY segments, empty blocks"""
    tl = TaskList()
    out_off = 0
    for b in range(nblocks):
        m, n = int(rng.integers(1, maxdim)), int(rng.integers(1, maxdim))
        ld = m + int(rng.integers(0, 3))
        tl.block(b, 1, out_off, m, n, ld)
        out_off += ld * n
        for s in range(int(rng.integers(0, 5))):
            alpha = complex(rng.standard_normal(), rng.standard_normal())
            if rng.random() < 0.2:
                ldb = m + int(rng.integers(0, 4))
                off = int(rng.integers(0, nbuf_elems - ldb * n - 1))
                tl.copy(b, 0, off, ldb, alpha)
                continue
            k = int(rng.integers(1, maxk))
            op_a, op_b = int(rng.integers(0, 3)), int(rng.integers(0, 3))
            lda = (m if op_a == abi.OP_N else k) + int(rng.integers(0, 3))
            ldb = (k if op_b == abi.OP_N else n) + int(rng.integers(0, 3))
            sa = lda * (k if op_a == abi.OP_N else m)
            sb = ldb * (n if op_b == abi.OP_N else k)
            a_off = int(rng.integers(0, nbuf_elems - sa - 1))
            b_off = int(rng.integers(0, nbuf_elems - sb - 1))
            tl.gemm(b, 0, a_off, lda, op_a, 2, b_off, ldb, op_b, k, alpha)
    return tl.finalize(), out_off


NEL = 400_000                        # elements of the operand buffers the random lists index into
# (seed, nblocks, maxdim, maxk): the two lists of test_grouped_gemm_split_k_across_workgroups_matches_numpy, whose long K
# loops the balancer must cut, and one of one-quadrant tiles with a few slabs each, which it must leave whole
SPLIT_CASES = [(5, 12, 70, 900), (6, 3, 140, 2500)]
WHOLE_CASE = (7, 6, 17, 30)
N_CUS = (256, 7)                     # the chip; a count that is no multiple of 8 (one XCD queue: the NX = 1 path)


def case_tasks(case):
    """-> (rng after the list was drawn, tasks, out_size) of one (seed, nblocks, maxdim, maxk)"""
    seed, nblocks, maxdim, maxk = case
    rng = np.random.default_rng(seed)
    tasks, out_size = random_tasks(rng, nblocks, maxdim, maxk, NEL)
    return rng, tasks, out_size


def balance(lib, tiles, n_cus):
    """(balanced tile records, workspace slabs) of htn_balance_tiles for the tile records `tiles`"""
    src = np.ascontiguousarray(tiles, dtype=abi.TILE_DT)
    n_out = C.c_int32(0)
    lib.htn_balance_tiles(src.ctypes.data, len(src), n_cus, None, 0, C.byref(n_out))
    out = np.zeros(max(n_out.value, 1), dtype=abi.TILE_DT)
    slots = lib.htn_balance_tiles(src.ctypes.data, len(src), n_cus, out.ctypes.data, len(out), C.byref(n_out))
    assert slots >= 0
    return out[:n_out.value], slots


def poly_model():
    """the polyacetylene parameter set (two bands)"""
    t = np.array([[0.000, 3.803, -0.548, 0.000], [3.803, 0.000, 2.977, -0.501]])
    U = np.array([[10.317, 6.264, 0.000, 0.000], [6.264, 10.317, 6.162, 0.000]])
    J = np.array([[0.000, 0.123, 0.000, 0.000], [0.123, 0.000, 0.113, 0.000]])
    return models.MB_Sim(t, U, J, 1, 1, 2.5, 20)


def apply_plan_lists(ops):
    """{name: tile records} of the H_eff apply (htn_plan_apply_dump, stages 0 and 1) on every bond of the nnn_nn and poly chains
    of test_cxx_apply_plans_are_byte_identical_to_the_python_statement after its one sweep"""
    L = 8
    out = {}
    for model, H in (("nnn_nn", models.hamiltonian(models.OB_Sim([1.0, 0.3], [4.0, 0.5]), L)),
                     ("poly", models.hamiltonian(poly_model(), L // 2))):
        bonds, tens = mps.random_mps(L, (L, 0), 5, seed=2)
        eng = engine.DMRG2(ops, H, bonds, tens, chi_full=60)
        eng.sweep()
        for i in range(L - 1):
            Ll = EnvLayout.build("L", eng.bonds[i], H[i].left)
            Rl = EnvLayout.build("R", eng.bonds[i + 2], H[i + 1].right)
            if eng.lib.htn_mps_env_size(eng.handle, 0, i) != Ll.size or eng.lib.htn_mps_env_size(eng.handle, 1, i + 2) != Rl.size:
                continue        # environment of an older bond table (the sweep moved on): no plan of this state
            for stage in (0, 1):
                out[f"apply/{model}/bond{i}/stage{stage}"] = eng.plan_apply_dump(i, stage)[0]
    return out


def plan_digests(ops):
    """{name: SHA-256 of the balanced tile records (integers only) and the slab count} over random lists x apply lists x N_CUS"""
    lists = {"random/" + "_".join(map(str, case)): (lambda t: t.tiles[:t.ntiles])(case_tasks(case)[1])
             for case in SPLIT_CASES + [WHOLE_CASE]}
    lists.update(apply_plan_lists(ops))
    dig = {}
    for name, tiles in sorted(lists.items()):
        for n_cus in N_CUS:
            out, slots = balance(ops.lib, tiles, n_cus)
            dig[f"{name}/cus{n_cus}"] = hashlib.sha256(out.tobytes() + np.int32(slots).tobytes()).hexdigest()
    return dig
