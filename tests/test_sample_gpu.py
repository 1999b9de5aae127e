"""Perfect sampling on the device: the sampling step kernels (htn_sample_step_z) against numpy, and the bodies of
test_sample_cpu.py through the HIP library.  Only the product library computes; references are the dense expansion of the stored
state and numpy."""
import numpy as np
import pytest
import torch

import sample_common as sc
from hubbardtn_amd import abi
from hubbardtn_amd.device import HipOps

pytestmark = pytest.mark.gpu

EDGES = (1, 15, 16, 17, 33)
SENT = -7.25                                     # sentinel around and between the views


# ---- 7. the kernels ---------------------------------------------------------------------------------------------------------------------
def _kernel_case(n_site, B, seed):
    """a made-up site: left and right sectors of the edges 1, 15, 16, 17, 33 mixed in one item list, padded leading dimensions, gaps
    between all views.  The last right sector is reached by multiplet 0 alone, one right sector by no sub-block at all."""
    rng = np.random.default_rng(seed)
    nl, nr = list(EDGES), list(EDGES) + [17, 5]
    lonely, orphan = len(nr) - 2, len(nr) - 1
    rho_off, pos = [], 2
    for n in nl:
        rho_off.append(pos)
        pos += n * n + 3
    rho_stride = pos
    out_off, pos = [], 1
    for n in nr:
        out_off.append(pos)
        pos += n * n + 5
    next_stride = pos
    items, a_pos, t_pos, pu, cu = [], 4, 3, 0, 0
    for r in range(len(nr)):
        if r == orphan:
            continue
        first = True
        for s in range(n_site):
            if r == lonely and s != 0:
                continue
            for l in range(len(nl)):
                if r != lonely and rng.random() < 0.35 and not (s == 0 and l == r % len(nl)):
                    continue
                lda = nl[l] + int(rng.integers(0, 4))
                run = abi.sample_units(nr[r], nr[r])
                items.append((rho_off[l], a_pos, t_pos, out_off[r], nl[l], nr[r], lda, s, pu, cu if first else cu + run,
                              float(rng.uniform(0.5, 1.5))))
                first = False
                pu += abi.sample_units(nl[l], nr[r])
                a_pos += lda * nr[r] + 2
                t_pos += nl[l] * nr[r] + 1
        cu += abi.sample_units(nr[r], nr[r])
    items = np.array(items, dtype=abi.SAMPLE_DT)
    A = rng.standard_normal(a_pos + 4) + 1j * rng.standard_normal(a_pos + 4)
    rho = np.full((B, rho_stride), SENT, dtype=np.complex128)
    for b in range(B):
        blocks = []
        for n in nl:
            x = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
            blocks.append(x @ x.conj().T)
        tr = sum(np.trace(x).real for x in blocks)
        for off, n, x in zip(rho_off, nl, blocks):
            rho[b, off:off + n * n] = (x / tr).reshape(-1, order="F")
    return dict(items=items, A=A, rho=rho, rho_stride=rho_stride, next_stride=next_stride, t_stride=t_pos + 2, nr=nr, out_off=out_off,
                lonely=lonely, orphan=orphan, u=rng.permutation((np.arange(B) + rng.random(B)) / B), logp0=rng.standard_normal(B))


def _reference(c, n_site, measure):
    items, A, B = c["items"], c["A"], len(c["rho"])
    T = np.full((B, c["t_stride"]), SENT, dtype=np.complex128)
    nxt = np.full((B, c["next_stride"]), SENT, dtype=np.complex128)
    choice, logp, near = np.zeros(B, dtype=np.int32), c["logp0"].copy(), np.zeros(B, dtype=bool)
    blk = lambda it: A[int(it["a_off"]) + np.arange(it["n_l"])[:, None] + int(it["lda"]) * np.arange(it["n_r"])[None, :]]
    for b in range(B):
        p, Ts = np.zeros(n_site), []
        for it in items:
            n = int(it["n_l"])
            R = c["rho"][b, int(it["rho_off"]):int(it["rho_off"]) + n * n].reshape(n, n, order="F")
            Ab = blk(it)
            Tq = R @ Ab
            Ts.append(Tq)
            T[b, int(it["t_off"]):int(it["t_off"]) + Tq.size] = Tq.reshape(-1, order="F")
            p[int(it["s"])] += float(it["coef"]) * np.real(np.vdot(Ab, Tq))
        tot = p.sum()
        if measure:
            cum = np.cumsum(p)
            target = c["u"][b] * tot
            live = np.nonzero(p > 0.0)[0]
            hit = [s for s in live if cum[s] >= target]
            choice[b] = hit[0] if hit else live[-1]
            near[b] = np.abs(cum[live] - target).min() <= sc.EDGE * tot
            logp[b] += np.log(p[choice[b]] / tot)
            scale = 1.0 / p[choice[b]]
        else:
            choice[b], scale = -1, 1.0 / tot
        for r, n in enumerate(c["nr"]):
            if r == c["orphan"]:
                continue
            acc = np.zeros((n, n), dtype=np.complex128)
            for it, Tq in zip(items, Ts):
                if int(it["out_off"]) == c["out_off"][r] and (not measure or int(it["s"]) == choice[b]):
                    acc += float(it["coef"]) * blk(it).conj().T @ Tq
            nxt[b, c["out_off"][r]:c["out_off"][r] + n * n] = (scale * acc).reshape(-1, order="F")
    return T, nxt, choice, logp, near


@pytest.mark.parametrize("measure", (1, 0))
@pytest.mark.parametrize("B", (1, 5, 64))
@pytest.mark.parametrize("n_site", (3, 4))
def test_sample_step_kernels_against_numpy(hip_ops, n_site, B, measure):
    c = _kernel_case(n_site, B, 100 * n_site + B)
    assert {int(x) for x in c["items"]["n_l"]} == set(EDGES) and set(EDGES) <= {int(x) for x in c["items"]["n_r"]}
    wantT, wantN, wantC, wantL, near = _reference(c, n_site, measure)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def run():
        T = dev(np.full((B, c["t_stride"]), SENT, dtype=np.complex128))
        nxt = dev(np.full((B, c["next_stride"]), SENT, dtype=np.complex128))
        choice = dev(np.full(B + 2, -5, dtype=np.int32))
        logp = dev(np.concatenate([c["logp0"], [SENT, SENT]]))
        hip_ops.sample_step(nxt, dev(c["rho"]), dev(c["A"]), T, c["items"], n_site, B, c["rho_stride"], c["next_stride"], c["t_stride"],
                            dev(c["u"]), measure, choice, logp)
        torch.cuda.synchronize()
        return T.cpu().numpy(), nxt.cpu().numpy(), choice.cpu().numpy(), logp.cpu().numpy()
    T, nxt, choice, logp = run()
    again = run()
    for x, y in zip((T, nxt, choice, logp), again):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))                      # bit-identical
    # nothing outside the views: the sentinels around and between them, the entries behind the batch
    assert np.array_equal(T == SENT, wantT == SENT) and np.array_equal(nxt == SENT, wantN == SENT)
    assert np.all(choice[B:] == -5) and np.all(logp[B:] == SENT)
    ok = ~near
    print("samples left out", int(near.sum()), "of", B)
    assert near.sum() <= max(B // 100, 0)
    assert np.array_equal(choice[:B][ok], wantC[ok])
    dT = np.abs(T - wantT).max() / np.abs(wantT[wantT != SENT]).max()
    dN = np.abs(nxt[ok] - wantN[ok]).max() / np.abs(wantN[wantN != SENT]).max()
    dL = np.abs(logp[:B][ok] - wantL[ok]).max()
    print("T", dT, "rho'", dN, "logp", dL)
    assert dT <= 1e-13 and dN <= 1e-13 and dL <= 1e-12
    # the sector only multiplet 0 reaches: exact zeros for every sample that drew another multiplet
    o, n = c["out_off"][c["lonely"]], c["nr"][c["lonely"]]
    if measure:
        other = choice[:B] != 0
        assert B < 5 or (other.any() and not other.all())               # (the uniforms are stratified over [0, 1): both kinds occur)
        assert np.all(nxt[other, o:o + n * n] == 0.0)
        assert np.all(np.abs(nxt[~other, o:o + n * n]).max(axis=1) > 0.0)
        tr = sum(nxt[:, c["out_off"][r]:c["out_off"][r] + k * k].reshape(B, k, k).diagonal(axis1=1, axis2=2).sum(axis=1)
                 for r, k in enumerate(c["nr"]) if r != c["orphan"])
        assert np.abs(tr - 1.0).max() <= 1e-12                                        # rho' keeps trace 1
    else:
        assert np.all(choice[:B] == -1) and np.array_equal(logp[:B], c["logp0"])


def test_sample_step_refuses_malformed_items(hip_ops):
    c = _kernel_case(3, 2, 1)
    bad = c["items"].copy()
    bad["probe_unit0"][1] += 1
    z = lambda n, dt=torch.complex128: torch.zeros(n, dtype=dt, device="cuda")
    with pytest.raises(abi.HtnError, match="item 1"):
        hip_ops.sample_step(z(2 * c["next_stride"]), z(2 * c["rho_stride"]), z(len(c["A"])), z(2 * c["t_stride"]), bad, 3, 2, c["rho_stride"],
                            c["next_stride"], c["t_stride"], z(2, torch.float64), 1, z(2, torch.int32), z(2, torch.float64))
    bad = c["items"].copy()
    bad["t_off"][-1] = c["t_stride"]                                                 # a view that leaves its stride
    with pytest.raises(abi.HtnError, match="outside its stride"):
        hip_ops.sample_step(z(2 * c["next_stride"]), z(2 * c["rho_stride"]), z(len(c["A"])), z(2 * c["t_stride"]), bad, 3, 2, c["rho_stride"],
                            c["next_stride"], c["t_stride"], z(2, torch.float64), 1, z(2, torch.int32), z(2, torch.float64))


# ---- the pass through the HIP library ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,case", sc.COMBOS)
def test_exact_probabilities(hip_ops, kind, case):
    """as test_sample_cpu.py: exp(logp) = p_ref to 100 x the CPU baseline library's measured deviation (3.3e-13)"""
    sc.check_exact(hip_ops, kind, case)


@pytest.mark.parametrize("kind,case", sc.COMBOS)
def test_choice_rule(hip_ops, kind, case):
    sc.check_choice_rule(hip_ops, kind, case)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_reproducible_and_independent_of_the_batch(hip_ops, kind):
    sc.check_reproducible(hip_ops, kind, "doped")


@pytest.mark.parametrize("kind,case", sc.COMBOS)
def test_marginals_reproduce_site_probabilities(hip_ops, kind, case):
    sc.check_marginals(hip_ops, kind, case)


@pytest.mark.parametrize("kind,case", sc.COMBOS)
def test_statistics(hip_ops, kind, case):
    sc.check_statistics(hip_ops, kind, case)


@pytest.mark.parametrize("mode", sc.tc.MODES)
def test_thermal_state_at_beta_zero(hip_ops, mode):
    sc.check_thermal_beta0(hip_ops, mode)


@pytest.mark.parametrize("mode", ("su2", "u1"))
def test_thermal_state_after_cooling(hip_ops, mode):
    sc.check_thermal_cooled(hip_ops, mode)


def test_refusals(hip_ops):
    sc.check_refusals(hip_ops, lambda: HipOps(0))


def test_a_sweep_after_sampling_plans_what_it_plans_without(hip_ops):
    sc.check_cache_hygiene(hip_ops)
