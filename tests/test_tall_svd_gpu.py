"""The SVD path for coupled blocks above 512 rows in both orientations on the MI355X: htn_jacobi_svd_z's streamed
multi-CU block Jacobi (k_jacobi_tall_visit) against numpy, next to the small-block and QRCP large-block paths in one
call; the engine's bond update on such a block against numpy and against the CPU baseline; a grown chain that reaches
such blocks."""
import numpy as np
import pytest

import tall_state as ts
from hubbardtn_amd import abi, engine, models, mps

pytestmark = pytest.mark.gpu


def _rand_z(rng, n):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def _matrix(rng, m, n, s):
    r = len(s)
    U, _ = np.linalg.qr(_rand_z(rng, m * r).reshape(m, r))
    W, _ = np.linalg.qr(_rand_z(rng, n * r).reshape(n, r))
    return (U * s) @ W.conj().T


def _batch():
    """(desc, mats, kinds): small blocks, one QRCP large block, the tall cases"""
    rng = np.random.default_rng(17)
    cases = []          # (m, n, flags, pad, singular values)
    graded = lambda r, dec: 10.0 ** (-dec * np.arange(r) / max(r - 1, 1))      # noqa: E731
    cases.append(("small", 64, 64, abi.SVD_ACCUMULATE, graded(64, 12)))
    cases.append(("small", 130, 90, 0, graded(90, 10)))
    cases.append(("qrcp", 230, 230, abi.SVD_QRCP, graded(230, 12)))             # G0 230 x 230: the large-block path
    cases.append(("tall", 520, 530, 0, graded(520, 12)))
    cases.append(("tall", 700, 1100, 0, graded(700, 12)))                       # mode A, wide: 400 columns go to zero
    cases.append(("tall", 600, 800, abi.SVD_ACCUMULATE, graded(600, 10)))       # mode B: J (800 x 800) accumulated
    s = graded(1030, 12)
    s[100:110] = s[100] * (1.0 + 1e-9 * np.arange(10))                          # a tight cluster
    cases.append(("tall", 1030, 1030, 0, np.sort(s)[::-1]))
    s = np.zeros(300)
    s[:] = graded(300, 8)
    cases.append(("tall", 800, 700, 0, s))                                       # rank 300
    desc = np.zeros(len(cases), dtype=abi.SVD_DT)
    go = vo = so = 0
    mats = []
    for i, (kind, m, n, flags, sv) in enumerate(cases):
        if kind == "qrcp":
            M = _matrix(rng, m, n, sv)                  # G0 = M (m0 x n0); result: n0 x r, right singular vectors x Sigma
            r = min(m, n)
            desc[i] = (go, vo, so, n, r, flags, m)
            go, vo, so = go + m * n, vo + ((n + 63) // 64 * 64) * r, so + r
        else:
            M = _matrix(rng, m, n, sv)
            desc[i] = (go, vo, so, m, n, flags, 0)
            go, vo, so = go + m * n, vo + (n * n if flags & abi.SVD_ACCUMULATE else 0), so + n
        mats.append(M)
    return desc, mats, [c[0] for c in cases], (go, vo, so)


def _run(hip_ops, desc, mats, sizes):
    go, vo, so = sizes
    dG = hip_ops.to_device(np.concatenate([M.T.reshape(-1) for M in mats]))
    dV, dS, info = hip_ops.zeros_z(vo), hip_ops.empty_f64(so), hip_ops.empty_i32(len(mats))
    max_m = int(max(max(d["m"], d["pad"]) for d in desc))
    # no preconditioning: a random 1030 x 1030 block graded over 12 decades needs ~50 outer sweeps (the one-CU kernel needs
    # ~45 on a 500 x 500 one), above the engine's default cap of 40
    used = hip_ops.jacobi_svd(dG, dV, dS, hip_ops.to_device(desc), len(mats), max_m, 80, 1e-14, info, desc_host=desc)
    return used, hip_ops.to_host(dG), hip_ops.to_host(dV), hip_ops.to_host(dS), hip_ops.to_host(info)


def test_tall_blocks_match_numpy_beside_small_and_qrcp_blocks(hip_ops):
    desc, mats, kinds, sizes = _batch()
    used, Gp, J, S, inf = _run(hip_ops, desc, mats, sizes)
    assert inf.min() >= 0, inf
    print("sweeps per block:", list(zip(kinds, inf.tolist())), "outer sweeps of the multi-CU paths:", used)
    for i, M in enumerate(mats):
        d = desc[i]
        ref = np.linalg.svd(M, compute_uv=False)
        big = ref >= 1e-6 * ref[0]
        if kinds[i] == "qrcp":
            n0, r = int(d["m"]), int(d["n"])
            out = Gp[d["g_off"]:d["g_off"] + n0 * r].reshape(r, n0).T
            s = S[d["s_off"]:d["s_off"] + r]
        else:
            m, n = int(d["m"]), int(d["n"])
            out = Gp[d["g_off"]:d["g_off"] + m * n].reshape(n, m).T
            s = S[d["s_off"]:d["s_off"] + n]
        got = np.sort(s)[::-1][:ref.size]
        assert np.abs(got[big] / ref[big] - 1).max() < 1e-8, (i, kinds[i])
        assert np.abs(got - ref).max() <= 1e-12 * ref[0], (i, kinds[i])
        live = s > 1e-13 * ref[0]
        Q = out[:, live] / s[live]
        assert np.abs(Q.conj().T @ Q - np.eye(live.sum())).max() < 1e-12, (i, kinds[i])      # orthonormal columns
        if d["flags"] & abi.SVD_ACCUMULATE and kinds[i] != "qrcp":
            n = int(d["n"])
            j = J[d["v_off"]:d["v_off"] + n * n].reshape(n, n).T
            assert np.abs(j.conj().T @ j - np.eye(n)).max() < 1e-12, (i, kinds[i])          # J unitary
            assert np.abs(M @ j - out).max() < 1e-12 * ref[0], (i, kinds[i])                # X' = M J
    # a second call on the same input is bit-identical (fixed-order Gram sums, no atomics on data)
    used2, Gp2, J2, S2, inf2 = _run(hip_ops, desc, mats, sizes)
    assert used2 == used and np.array_equal(inf2, inf) and np.array_equal(S2, S) and np.array_equal(Gp2, Gp)
    assert np.array_equal(J2, J)


def test_tall_block_without_host_descriptors_is_an_error(hip_ops):
    rng = np.random.default_rng(3)
    m, n = 600, 600
    desc = np.zeros(1, dtype=abi.SVD_DT)
    desc[0] = (0, 0, 0, m, n, 0, 0)
    dG = hip_ops.to_device(_rand_z(rng, m * n))
    dV, dS, info = hip_ops.zeros_z(1), hip_ops.empty_f64(n), hip_ops.empty_i32(1)
    with pytest.raises(abi.HtnError, match="512"):
        hip_ops.jacobi_svd(dG, dV, dS, hip_ops.to_device(desc), 1, m, 40, 1e-14, info)


def test_engine_update_on_a_tall_block_matches_numpy_and_the_cpu_baseline(hip_ops):
    from cpu_ops import CpuOps
    eng = ts.centred_engine(hip_ops, krylovdim=6, maxrestart=1)
    blocks = ts.coupled_blocks(eng, ts.I0)
    assert ts.largest_block(blocks) > 512
    ref = ts.schmidt_reference(blocks)
    E0 = eng.update_bond(ts.I0, +1, "right", optimise=False, record=False, cutoff=0.0)
    ts.assert_spectrum_matches(eng.spectrum(ts.I0 + 1), ref)
    ts.assert_left_isometry(eng, ts.I0)
    E1 = eng.update_bond(ts.I0, -1, "left", optimise=True, record=False, cutoff=0.0)
    assert E1 <= E0 + 1e-10 * abs(E0)
    # the same two updates on the CPU baseline (same planner, host Jacobi)
    cpu = ts.centred_engine(CpuOps(), krylovdim=6, maxrestart=1)
    cpu.update_bond(ts.I0, +1, "right", optimise=False, record=False, cutoff=0.0)
    E1c = cpu.update_bond(ts.I0, -1, "left", optimise=True, record=False, cutoff=0.0)
    assert abs(E1 - E1c) <= 1e-10 * abs(E1c), (E1, E1c)
    got, want = eng.spectrum(ts.I0 + 1), cpu.spectrum(ts.I0 + 1)
    ts.assert_spectrum_matches(got, {c: np.sort(v)[::-1] for c, v in want.items()})


def test_full_sweeps_through_tall_blocks(hip_ops):
    """whole sweeps (the library's sweep driver) over a chain whose centre bonds carry blocks above 512 in both
    orientations: the energy does not go up, and the centre bond's spectrum matches numpy.  (A chain grown from a small
    state does not serve here: L = 24 grown 16 -> 4096 stays at ~1024 on every bond, far below tall blocks.)"""
    L = 14
    H = models.hamiltonian(models.OB_Sim([1.0], [4.0]), L)
    bonds, tens = mps.random_mps(L, (L, 0), 200, seed=11)
    eng = engine.DMRG2(hip_ops, H, bonds, tens, chi_full=4096, lanczos_tol=1e-8, krylovdim=8, maxrestart=1)
    size, where = ts.largest_coupled_block(eng)
    print(f"largest coupled block {size} on the layout of bond {where}; bond dims {eng.bond_dims()}")
    assert size > 512
    E1 = eng.sweep()
    E2 = eng.sweep()
    size2, _ = ts.largest_coupled_block(eng)
    print(f"after two sweeps: E {E1:.12f} -> {E2:.12f}, largest coupled block {size2}, bond dims {eng.bond_dims()}")
    assert np.isfinite(E2) and E2 <= E1 + 1e-9 * abs(E1), (E1, E2)
    assert size2 > 512
    # centre bond: move the centre onto site i0 and compare a non-optimising update with numpy
    i0 = L // 2 - 1
    for i in range(i0):
        eng.update_bond(i, +1, "right", optimise=False, record=False, cutoff=0.0)
    eng.chi_full = None                 # the update under test keeps every Schmidt value
    blocks = ts.coupled_blocks(eng, i0)
    assert ts.largest_block(blocks) > 512
    ref = ts.schmidt_reference(blocks)
    eng.update_bond(i0, +1, "right", optimise=False, record=False, cutoff=0.0)
    ts.assert_spectrum_matches(eng.spectrum(i0 + 1), ref)
