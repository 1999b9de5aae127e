"""Step-exact tests of the Lanczos kernels (hubbardtn_amd/csrc/htn_krylov.hip) on the MI355X.

With tol = 0 and max_restart = 0 the driver runs exactly `krylovdim` steps and returns the Ritz pair of the k-dimensional
Krylov space, so one call per k pins step k: eigenvalue, residual and Ritz vector are compared with the extended-precision
reference of tests/ref_krylov.py, within max(10 x the float64 statement's own deviation, 256 eps) -- the figures measured
by tests/test_ref_krylov_cpu.py (ref_krylov.F64_DEVIATION), never tuned against GPU output.  A restarted Lanczos heals
itself, so the converged outcome says little about a single kernel; these tests look at every step, every compile-time
row count (4 .. 32), both FZ forms, and at the Krylov basis itself.

WHITE BOX: the ABI documents only V[0:n].  The orthonormality checks read the other rows of V as lanczos_run leaves them
after a k-step call: rows 1 .. k-1 hold the normalised Lanczos vectors, row k the raw (unnormalised) last vector, row 0
the Ritz vector (v_0 = P x0 / |P x0| is known to the test).  Their bar, 64 eps, is derived, not measured: two Gram-Schmidt
passes against an orthonormal basis leave O(eps); a missing second pass shows 1.5e-12.

Run as a script (one fresh child process per process-wide switch) the file repeats the k sweep at n = 3000 and prints JSON.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):          # (the file is also run as a script: the child processes)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ref_krylov as rk                                  # noqa: E402
from emul import NumpyOps                                # noqa: E402
from hubbardtn_amd import abi                            # noqa: E402
from test_ref_krylov_cpu import CASES, case_ks, case_problem, f64_steps     # noqa: E402

pytestmark = pytest.mark.gpu
EPS = rk.EPS
ORTHO_BAR = 64 * EPS


class Problem:
    """operator, start vector, frozen rows, device stages and the reference of one case: built once per module"""

    def __init__(self, ops, case, H=None, K=None, x0=None, Qs=None, variant="one"):
        if H is None:
            H, K, x0, Qs = case_problem(case)
        self.ops, self.case, self.H, self.K, self.x0, self.Qs = ops, case, H, K, x0, Qs
        self.op = rk.SylvesterOp(H, K)
        self.n, self.scale = self.op.n, self.op.norm_bound()
        self.stages = rk.sylvester_stages(ops, H, K, variant)
        self.Qd = {nf: (None if Q is None else ops.to_device(Q.reshape(-1))) for nf, Q in Qs.items()}
        self.x0d = ops.to_device(x0)
        self._ref = {}

    def ref(self, nf, ks):
        if nf not in self._ref:
            self._ref[nf] = rk.krylov_ritz(self.op, self.x0, max(ks), self.Qs[nf], ks=ks)
        return self._ref[nf]

    def run(self, k, nf=0, tol=0.0, max_restart=0, rows=None):
        """one driver call -> eig, n_matvec, res, the first `rows` rows of V on the host (default k + 1)"""
        n, ops = self.n, self.ops
        V = ops.zeros_z((k + 2) * n)
        V[0:n] = self.x0d
        if nf == 0:
            eig, nmv, res = ops.lanczos(self.stages, 0, 1, V, n, k, tol, max_restart)
        else:
            eig, nmv, res = ops.lanczos_orth(self.stages, 0, 1, V, n, k, tol, max_restart, self.Qd[nf], nf)
        rows = k + 1 if rows is None else rows
        return eig, nmv, res, ops.to_host(V[0:rows * n]).reshape(rows, n)


def deviations(p, ref, k, eig, res, x):
    return (abs(eig - ref["theta"][k - 1]) / p.scale, abs(res - ref["res"][k - 1]) / p.scale,
            float(np.linalg.norm(x - ref["x"][k])))


def basis_defect(p, ref, k, nf, Vh):
    """max |v_i^H v_j - delta_ij| over v_0 (known), rows 1 .. k-1 and raw_k / |raw_k|; max |Q v_i|"""
    B = np.concatenate([ref["v0"][None, :], Vh[1:k], Vh[k:k + 1] / np.linalg.norm(Vh[k])])
    g = float(np.abs(B.conj() @ B.T - np.eye(k + 1)).max())
    q = float(np.abs(p.Qs[nf].conj() @ B.T).max()) if nf else 0.0
    return g, q


def check_step(p, nf, k, ks, label=""):
    ref = p.ref(nf, ks)
    eig, nmv, res, Vh = p.run(k, nf)
    dev = deviations(p, ref, k, eig, res, Vh[0])
    bars = [rk.bar(m) for m in rk.F64_DEVIATION[p.case]]
    g, q = basis_defect(p, ref, k, nf, Vh)
    print(label or p.case, "nf", nf, "k", k, "theta %.2e res %.2e x %.2e" % dev, "bars %.1e %.1e %.1e" % tuple(bars),
          "basis %.2e Q %.2e" % (g, q), "bar %.1e" % ORTHO_BAR)
    assert nmv == k
    assert dev[0] <= bars[0] and dev[1] <= bars[1] and dev[2] <= bars[2], (label or p.case, nf, k, dev, bars)
    assert g <= ORTHO_BAR and q <= ORTHO_BAR, (label or p.case, nf, k, g, q)
    return eig, nmv, res, Vh[0]


@pytest.fixture(scope="module")
def p3000(hip_ops):
    return Problem(hip_ops, "n3000")


@pytest.fixture(scope="module")
def pbig(hip_ops):
    return Problem(hip_ops, "n200704")


@pytest.mark.parametrize("nf", rk.NF_LIST)
def test_every_step_at_n3000(p3000, nf):
    """every k = 2 .. 31 - nf: all eight row-count instantiations of the three kernels, FZ and not, upd0 = 0 (j < 2) and
    j - 1, first = true / false, the k_publish_record end of a cycle; Ritz pair and basis"""
    ks = case_ks("n3000", nf)
    for k in ks:
        check_step(p3000, nf, k, ks)


@pytest.mark.parametrize("nf", rk.NF_LIST)
def test_steps_at_n448x448(pbig, nf):
    """the size of a chi ~ 1000 two-site tensor (784 elements per slice: several 256-thread strides)"""
    ks = case_ks("n200704", nf)
    for k in ks:
        check_step(pbig, nf, k, ks)


@pytest.mark.parametrize("n", rk.EDGE_SIZES)
def test_sizes_where_slices_go_wrong(hip_ops, n):
    """256 slices of ceil(n / 256): empty slices, one element per slice, a ragged last slice, several strides per slice.
    n <= k: the Krylov space is exhausted and the invariant-subspace exit must return the lowest eigenvalue of the n x n
    operator (an exact eigenvalue of T up to the bisection's 4e-16 * scale and rounding in T: bar 1e-12 |A|), within
    n + 1 matvecs, with a finite unit vector: the speculative step after the breakdown runs on a zero-norm raw row and must
    not leak into the result."""
    case = "n%d" % n
    if case in CASES:
        p = Problem(hip_ops, case)
    else:
        m, nc = rk.factor(n)
        H, K = rk.make_operator(100 + n, m, nc)
        p = Problem(hip_ops, case, H, K, rk.rand_z(np.random.default_rng(n), n), {0: None})
    for k in (2, 9, 31):
        if n > k:
            check_step(p, 0, k, [2, 9, 31])
            continue
        w = np.linalg.eigvalsh(p.op.dense())
        eig, nmv, res, Vh = p.run(k, 0, rows=1)
        x = Vh[0]
        true_res = float(np.linalg.norm(p.op(x) - eig * x))
        print(case, "k", k, "eig - w0", eig - w[0], "matvecs", nmv, "res", res, "true", true_res, "|x|", np.linalg.norm(x))
        assert abs(eig - w[0]) <= 1e-12 * p.scale
        assert nmv <= n + 1
        assert np.isfinite(x).all() and abs(np.linalg.norm(x) - 1.0) <= 8 * EPS
        assert true_res <= 1e-12 * p.scale


def test_start_vector_that_is_an_eigenvector(hip_ops):
    """breakdown at step 0: at most the step and its speculative successor are enqueued; the vector comes back"""
    H, K, _, _ = case_problem("n63")
    op = rk.SylvesterOp(H, K)
    w, U = np.linalg.eigh(op.dense())
    for which in (0, 5):
        p = Problem(hip_ops, "n63", H, K, U[:, which].copy(), {0: None})
        eig, nmv, res, Vh = p.run(20, 0, tol=1e-10, max_restart=5, rows=1)
        ov = abs(np.vdot(U[:, which], Vh[0]))
        print("eigenvector start", which, "eig - w", eig - w[which], "matvecs", nmv, "res", res, "overlap", ov)
        assert nmv <= 2
        assert abs(eig - w[which]) <= 1e-12 * p.scale and abs(ov - 1.0) <= 1e-12 and np.isfinite(Vh[0]).all()


def test_doubly_degenerate_lowest_eigenvalue(hip_ops):
    """the eigenvalue and the residual against the dense operator (the vector is any unit vector of the eigenplane);
    in exact arithmetic |beta y_k| IS the residual norm, so the two agree to rounding"""
    m, nc = rk.factor(63)
    H, K = rk.make_operator(7, m, nc, degenerate=True)
    p = Problem(hip_ops, "n63", H, K, rk.rand_z(np.random.default_rng(8), 63), {0: None})
    w = np.linalg.eigvalsh(p.op.dense())
    assert w[1] - w[0] <= 64 * EPS * p.scale < w[2] - w[0]
    tol = 1e-10
    eig, nmv, res, Vh = p.run(20, 0, tol=tol, max_restart=50, rows=1)
    x = Vh[0]
    true_res = float(np.linalg.norm(p.op(x) - eig * x))
    print("degenerate: eig - w0", eig - w[0], "matvecs", nmv, "res", res, "true residual", true_res)
    assert res < tol and abs(eig - w[0]) <= tol * p.scale
    assert abs(true_res - res) <= 256 * EPS * p.scale and abs(np.linalg.norm(x) - 1.0) <= 8 * EPS


@pytest.mark.parametrize("kd", [2, 3, 5])
def test_restarts_follow_the_float64_statement(p3000, kd):
    """short cycles, many restarts: eigenvalue to the requested tolerance and the matvec count of NumpyOps.lanczos on the
    same problem (same rules, same stop step).  The product enqueues step j + 1 before it has step j's record, so a run
    that stops before the last step of its cycle has counted one speculative matvec: that is the only difference."""
    tol, mr = 1e-8, 4000
    p = p3000
    w0 = np.linalg.eigvalsh(p.H)[0] + np.linalg.eigvalsh(p.K)[0]
    cpu = NumpyOps()
    V = cpu.zeros_z((kd + 2) * p.n)
    V[0:p.n] = p.x0
    rec = {}
    theta, nmv_cpu, res_cpu = cpu.lanczos(rk.sylvester_stages(cpu, p.H, p.K), 0, 1, V, p.n, kd, tol, mr, record=rec)
    assert res_cpu < tol
    expect = nmv_cpu + (1 if rec["stop"][1] < kd - 1 else 0)
    eig, nmv, res, _ = p.run(kd, 0, tol=tol, max_restart=mr, rows=1)
    print("kd", kd, "eig - w0", eig - w0, "matvecs", nmv, "float64 statement", nmv_cpu, "stop", rec["stop"], "res", res, res_cpu)
    assert res < tol and abs(eig - w0) <= tol * p.scale
    assert nmv == expect


@pytest.mark.parametrize("variant", ["one", "empty_first", "two"])
def test_stage_structure_of_the_matvec(hip_ops, p3000, variant):
    """the record of step j - 1 is published by the first launch of the matvec that has tiles: one stage; an empty stage
    followed by the work; two working stages (Z = H X into a side buffer, then Y = Z + X K^T with a COPY segment)"""
    p = Problem(hip_ops, "n3000", p3000.H, p3000.K, p3000.x0, {0: None}, variant)
    p._ref = p3000._ref
    for k in (2, 5, 17, 31):
        check_step(p, 0, k, case_ks("n3000", 0), label="stages=" + variant)


# ---- process-wide switches: one fresh child process each -------------------------------------------------------------
def sweep_n3000(ops):
    """the k sweep at n = 3000, nf in {0, 3} -> {"nf:k": [eig.hex, n_matvec, res.hex, sha256(x), dtheta, dres, dx, basis, Q]}"""
    p = Problem(ops, "n3000")
    out = {}
    for nf in (0, 3):
        ks = case_ks("n3000", nf)
        ref = p.ref(nf, ks)
        for k in ks:
            eig, nmv, res, Vh = p.run(k, nf)
            out["%d:%d" % (nf, k)] = [float(eig).hex(), int(nmv), float(res).hex(), hashlib.sha256(Vh[0].tobytes()).hexdigest(),
                                      *deviations(p, ref, k, eig, res, Vh[0]), *basis_defect(p, ref, k, nf, Vh)]
    return out


def _child(switch):
    env = dict(os.environ)
    env[switch] = "1"
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])   # (a child that died: nothing further runs here)
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_full_first_pass_switch_meets_the_same_bars():
    """HTN_LANCZOS_FULL_FIRST_PASS=1 (read once per process): same bars against the reference, not bit-equal to the product"""
    got = _child("HTN_LANCZOS_FULL_FIRST_PASS")
    bars = [rk.bar(m) for m in rk.F64_DEVIATION["n3000"]]
    assert len(got) == 30 + 27
    for key, (_, nmv, _, _, dt, dr, dx, g, q) in got.items():
        print("full first pass", key, "theta %.2e res %.2e x %.2e basis %.2e Q %.2e" % (dt, dr, dx, g, q))
        assert nmv == int(key.split(":")[1])
        assert dt <= bars[0] and dr <= bars[1] and dx <= bars[2] and g <= ORTHO_BAR and q <= ORTHO_BAR, key


def test_event_waits_switch_is_bit_identical_to_polling(hip_ops):
    """HTN_DEBUG_EVENT_WAITS=1: the host waits for an event instead of polling the record -- the same bits"""
    got = _child("HTN_DEBUG_EVENT_WAITS")
    here = sweep_n3000(hip_ops)
    assert set(got) == set(here) and len(here) == 30 + 27
    for key in here:
        assert got[key][:4] == here[key][:4], key


# ---- the three ABI vector primitives at their edges -------------------------------------------------------------------
NVECS = [1, 4, 5, 31, 32, 33, 63, 64]
_SENT = complex(-7.25, 3.5)


@pytest.fixture(scope="module")
def vec_data(hip_ops):
    """per n: 64 rows at ldv = n and at ldv = n + 3 (the padding holds a sentinel), w, coefficients; host and device"""
    rng = np.random.default_rng(77)
    data = {}
    for n in rk.EDGE_SIZES:
        rows = rk.rand_z(rng, 64 * n).reshape(64, n)
        w, coef = rk.rand_z(rng, n), rk.rand_z(rng, 64)
        per_ld = {}
        for ldv in (n, n + 3):
            flat = np.full(64 * ldv, _SENT, dtype=np.complex128)
            flat.reshape(64, ldv)[:, :n] = rows
            per_ld[ldv] = hip_ops.to_device(flat)
        data[n] = (rows, w, coef, per_ld, hip_ops.to_device(w), hip_ops.to_device(coef))
    return data


def _dots_chain(n):
    # htn_dots_z's summation tree, from the code: a slice holds per = ceil(n / 256) elements; each of the 256 threads of a
    # slice adds ceil(per / 256) products in series; then 6 butterfly levels in the wave, the 4 waves of the slice in series,
    # the reducing wave adds 4 partials per lane in series and takes 6 more butterfly levels: 20 further additions on the
    # longest path; the remaining 4 of the issue's 24 cover the two products and the addition inside one complex product
    per = -(-n // 256)
    return -(-per // 256) + 24


@pytest.mark.parametrize("nvec", NVECS)
def test_dots_at_the_edges(hip_ops, vec_data, nvec):
    """against a long double accumulation; bar (L + 24) eps sum |v| |w|, L the longest serial chain; the same bits twice"""
    for n in rk.EDGE_SIZES:
        rows, w, _, per_ld, dw, _ = vec_data[n]
        ref = (rows[:nvec].conj().astype(rk.CLD) * w.astype(rk.CLD)).sum(axis=1)
        mag = (np.abs(rows[:nvec]).astype(rk.LD) * np.abs(w).astype(rk.LD)).sum(axis=1)
        for ldv, dV in per_ld.items():
            out = hip_ops.to_device(np.full(nvec + 1, _SENT))
            hip_ops.dots(dV, ldv, nvec, dw, n, out)
            got = hip_ops.to_host(out)
            out2 = hip_ops.to_device(np.full(nvec + 1, _SENT))
            hip_ops.dots(dV, ldv, nvec, dw, n, out2)
            err = np.abs(got[:nvec] - ref).astype(np.float64)
            bound = (_dots_chain(n) * EPS * mag).astype(np.float64)
            assert (err <= bound).all(), (n, ldv, nvec, float((err / bound).max()))
            assert got[nvec] == _SENT and np.array_equal(hip_ops.to_host(out2), got), (n, ldv, nvec)


@pytest.mark.parametrize("nvec", NVECS)
def test_axpys_at_the_edges(hip_ops, vec_data, nvec):
    """w += sign * sum c_i V_i against long double; bar (nvec + 2) eps (|w_j| + sum |c_i| |V_ij|) per element"""
    for n in rk.EDGE_SIZES:
        rows, w, coef, per_ld, _, dcoef = vec_data[n]
        upd = (coef[:nvec, None].astype(rk.CLD) * rows[:nvec].astype(rk.CLD)).sum(axis=0)
        mag = np.abs(w).astype(rk.LD) + (np.abs(coef[:nvec, None]).astype(rk.LD) * np.abs(rows[:nvec]).astype(rk.LD)).sum(axis=0)
        for ldv, dV in per_ld.items():
            for sign in (1.0, -1.0):
                dw = hip_ops.to_device(np.concatenate([w, [_SENT]]))
                hip_ops.axpys(dw, dV, ldv, nvec, dcoef, sign, n)
                got = hip_ops.to_host(dw)
                err = np.abs(got[:n] - (w.astype(rk.CLD) + sign * upd)).astype(np.float64)
                bound = ((nvec + 2) * EPS * mag).astype(np.float64)
                assert (err <= bound).all(), (n, ldv, nvec, sign, float((err / bound).max()))
                assert got[n] == _SENT


def test_scale_inv_sqrt_at_the_edges(hip_ops, vec_data):
    """dst = src / sqrt(Re nrm2), dst aliasing src and not: 2 eps relative per element (sqrt, reciprocal, product)"""
    nrm2 = 3.7 + 0j
    dn = hip_ops.to_device(np.array([nrm2]))
    for n in rk.EDGE_SIZES:
        w = vec_data[n][1]
        ref = w.astype(rk.CLD) / np.sqrt(rk.LD(nrm2.real))
        for alias in (True, False):
            src = hip_ops.to_device(np.concatenate([w, [_SENT]]))
            dst = src if alias else hip_ops.to_device(np.full(n + 1, _SENT))
            hip_ops.scale_inv_sqrt(dst, src, dn, n)
            got = hip_ops.to_host(dst)
            for part in ("real", "imag"):
                err = np.abs(getattr(got[:n], part) - getattr(ref, part)).astype(np.float64)
                assert (err <= 2 * EPS * np.abs(getattr(w, part))).all(), (n, alias, part)
            assert got[n] == _SENT
            if not alias:
                assert np.array_equal(hip_ops.to_host(src)[:n], w)


def test_empty_calls_and_the_row_limit(hip_ops, vec_data):
    """nvec = 0 and n = 0 return 0 and write nothing (htn_dots_z with n = 0 and rows: the empty sums, exact zeros);
    nvec = 65 on htn_dots_z is the documented error"""
    n = 257
    rows, w, coef, per_ld, dw0, dcoef = vec_data[n]
    dV = per_ld[n]
    sent = np.full(8, _SENT)
    out = hip_ops.to_device(sent)
    hip_ops.dots(dV, n, 0, dw0, n, out)
    assert np.array_equal(hip_ops.to_host(out), sent)
    hip_ops.dots(dV, n, 5, dw0, 0, out)
    assert np.array_equal(hip_ops.to_host(out), np.concatenate([np.zeros(5), sent[5:]]))
    for nvec, nn in ((0, n), (5, 0), (0, 0)):
        dw = hip_ops.to_device(w)
        hip_ops.axpys(dw, dV, n, nvec, dcoef, -1.0, nn)
        assert np.array_equal(hip_ops.to_host(dw), w)
    dst = hip_ops.to_device(sent)
    hip_ops.scale_inv_sqrt(dst, dw0, dcoef, 0)
    assert np.array_equal(hip_ops.to_host(dst), sent)
    lib = hip_ops.lib
    scratch = hip_ops.empty_z(lib.htn_dots_scratch_elems(65))
    big = hip_ops.to_device(np.full(65, _SENT))
    rc = lib.htn_dots_z(hip_ops._p(dV), 1, 65, hip_ops._p(dw0), 1, hip_ops._p(big), hip_ops._p(scratch), hip_ops._stream())
    assert rc != 0 and "nvec > 64" in lib.htn_last_error().decode()
    with pytest.raises(abi.HtnError, match="nvec > 64"):
        abi.check(lib, rc, "htn_dots_z")
    hip_ops.sync()
    assert np.array_equal(hip_ops.to_host(big), np.full(65, _SENT))


if __name__ == "__main__":
    from hubbardtn_amd.device import HipOps
    print(json.dumps(sweep_n3000(HipOps(0))))
