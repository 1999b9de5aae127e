"""k_jacobi_ring with two partner columns per cross step (HTN_RING_TWO_PARTNER=1) against LAPACK and against the default
one-partner step: even and odd panel widths, ragged last panels, rank-deficient blocks, the 64-lane form (400 rows).

Panel planning of the 16-lane form (m <= 256 rows, mp = 16 ceil(m / 16)): at most min(32, 4608 / mp) columns per panel, cut
to 16 between 17 and 31; P = ceil(n / 2 wcap) workgroups, w = ceil(n / 2P).  Square blocks of n columns: 128 -> w = 32 (P = 2),
160 -> w = 16, 190 -> w = 16 with a last panel of 14, 150 and 180 -> w = 15 (odd, full panels), 202 -> w = 15 with a last
panel of 7, 107 -> w = 27 with a last panel of 26."""
import numpy as np
import pytest

from hubbardtn_amd import abi

pytestmark = pytest.mark.gpu


def _rand_z(rng, n):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def _run(hip_ops, shapes, seed, decades=12.0, rank_cut=0.0):
    """shapes: (m0, n0, rank); returns the matrices, the descriptors, G', S, info"""
    rng = np.random.default_rng(seed)
    desc = np.zeros(len(shapes), dtype=abi.SVD_DT)
    go = vo = so = 0
    mats = []
    for i, (m0, n0, rank) in enumerate(shapes):
        r = min(m0, n0)
        desc[i] = (go, vo, so, n0, r, abi.SVD_QRCP, m0)
        U, _ = np.linalg.qr(_rand_z(rng, m0 * rank).reshape(m0, rank))
        W, _ = np.linalg.qr(_rand_z(rng, n0 * rank).reshape(n0, rank))
        s = 10.0 ** (-decades * np.arange(rank) / max(rank - 1, 1))
        mats.append((U * s) @ W.conj().T)
        go, vo, so = go + m0 * n0, vo + ((n0 + 63) // 64 * 64) * r, so + r
    dG = hip_ops.to_device(np.concatenate([M.T.reshape(-1) for M in mats]))
    dV, dS, info = hip_ops.zeros_z(vo), hip_ops.empty_f64(so), hip_ops.empty_i32(len(shapes))
    used = hip_ops.jacobi_svd(dG, dV, dS, hip_ops.to_device(desc), len(shapes), max(max(x[:2]) for x in shapes), 40, 1e-14,
                              info, desc_host=desc, rank_cut=rank_cut)
    assert used > 0                                   # the large-block path (ring) took the blocks
    return mats, desc, hip_ops.to_host(dG), hip_ops.to_host(dS), hip_ops.to_host(info)


def _check(shapes, mats, desc, Gp, S, inf, max_sweeps=12):
    assert inf.min() >= 0 and inf.max() <= max_sweeps, inf
    for i, (m0, n0, rank) in enumerate(shapes):
        d = desc[i]
        r = min(m0, n0)
        out = Gp[d["g_off"]:d["g_off"] + n0 * r].reshape(r, n0).T
        s = S[d["s_off"]:d["s_off"] + r]
        assert np.isfinite(out).all() and np.isfinite(s).all(), i
        ref = np.linalg.svd(mats[i], compute_uv=False)
        order = np.argsort(-s)
        assert np.abs(s[order] - ref).max() <= 1e-13 * ref[0], i
        big = ref > 1e-6 * ref[0]
        assert np.abs(s[order][big] / ref[big] - 1).max() < 1e-8, i
        live = s > 1e-11 * ref[0] if rank < r else s > 1e-13 * ref[0]
        if rank < r:
            assert live.sum() == rank, i
        Viso = out[:, live] / s[live]
        assert np.abs(Viso.conj().T @ Viso - np.eye(live.sum())).max() < 1e-12, i
        assert np.abs(np.linalg.norm(mats[i] @ Viso, axis=0) - s[live]).max() <= 1e-12 * ref[0], i


@pytest.mark.parametrize("shapes", [[(128, 128, 128), (160, 160, 160)],              # even w, full panels
                                    [(202, 202, 202), (150, 150, 150)],              # odd w (202: ragged last panel)
                                    [(190, 190, 190), (107, 107, 107), (230, 180, 180)]])   # ragged last panels
def test_two_partner_ring_matches_lapack(hip_ops, monkeypatch, shapes):
    monkeypatch.setenv("HTN_RING_TWO_PARTNER", "1")
    _check(shapes, *_run(hip_ops, shapes, seed=41))


@pytest.mark.parametrize("rank_cut", [0.0, 1e-12])
def test_two_partner_ring_rank_deficient(hip_ops, monkeypatch, rank_cut):
    """numerically zero columns inside the tournament (rank_cut = 0) or a tournament sized by the rank the QR found
    (rank_cut > 0: n = rank, ragged panels)"""
    monkeypatch.setenv("HTN_RING_TWO_PARTNER", "1")
    shapes = [(200, 200, 121), (180, 150, 97), (240, 240, 240)]
    _check(shapes, *_run(hip_ops, shapes, seed=43, decades=8.0, rank_cut=rank_cut))


def test_two_partner_ring_400(hip_ops, monkeypatch):
    """400 rows: the 64-lane form (one column per wave) keeps the one-partner step under the switch; beside it a 16-lane block"""
    monkeypatch.setenv("HTN_RING_TWO_PARTNER", "1")
    shapes = [(400, 400, 400), (202, 202, 202)]
    _check(shapes, *_run(hip_ops, shapes, seed=47), max_sweeps=13)


def test_two_partner_agrees_with_one_partner(hip_ops, monkeypatch):
    """the same rotations in another order inside a round: the singular values agree to 1e-12 (relative to sigma_max)"""
    shapes = [(202, 202, 202), (128, 128, 128), (190, 190, 190), (150, 150, 150), (200, 200, 121)]
    monkeypatch.delenv("HTN_RING_TWO_PARTNER", raising=False)
    mats, desc, _, S1, inf1 = _run(hip_ops, shapes, seed=53)
    monkeypatch.setenv("HTN_RING_TWO_PARTNER", "1")
    _, _, _, S2, inf2 = _run(hip_ops, shapes, seed=53)
    assert inf1.min() >= 0 and inf2.min() >= 0, (inf1, inf2)
    for i, (m0, n0, rank) in enumerate(shapes):
        d = desc[i]
        r = min(m0, n0)
        s1 = np.sort(S1[d["s_off"]:d["s_off"] + r])[::-1]
        s2 = np.sort(S2[d["s_off"]:d["s_off"] + r])[::-1]
        assert np.abs(s1 - s2).max() <= 1e-12 * s1[0], i
        assert abs(int(inf1[i]) - int(inf2[i])) <= 1, (i, inf1, inf2)
