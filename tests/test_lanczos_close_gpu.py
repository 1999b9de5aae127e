"""Closing a Lanczos solve at the step that is expected to converge (HTN_LANCZOS_CLOSE, hubbardtn_amd/csrc/htn_krylov.hip).

The switch is read once per process, so every mode -- auto (the predictor), never (every step open: the step behind the
converged one has run for nothing), always (every step closed) -- runs the same list of solves in ONE fresh child process
(`python tests/test_lanczos_close_gpu.py`); a fourth child repeats auto with HTN_DEBUG_POISON=1.  Which steps are closed
changes what is enqueued, never what is computed: eigenvalue, residual and every element of the returned vector must be
bit-identical in the three modes, and only the matvec count may differ:

  never    steps + 1 if the solve stopped before the last step of its cycle (the speculative step), else steps
  always   steps
  auto     between the two; with tol = 0 (nothing can be expected to converge) exactly what never enqueues

`steps` comes from the float64 statement of the driver (emul.NumpyOps.lanczos: same rules, same stop step), as in
test_krylov_steps_gpu.py.  Operators: ref_krylov.sylvester_stages at n = 3000 (100 x 30), 63 and 1025; every solve also
with three frozen rows.  The solves of a (n, nf):

  inside     tol 1e-10, krylovdim 23, from a start vector the float64 statement has brought to 1e-9: converges well inside
             the first cycle
  last       the same with krylovdim = (stop step of `inside`) + 1: convergence falls on the last step of the cycle
  restarts   krylovdim 6 from the random start vector: converges only after many restarts
  tol0       tol 0, krylovdim 9, one restart: 18 steps, never converges
  pair       `inside` and `restarts` enqueued back to back on the same stream and scratch, nothing waiting in between; the
             basis of the second and the scratch start as NaN.  Each must reproduce the bits of its solve run alone: the
             driver returns with its last kernels in flight and the next solve is ordered behind them by the stream alone.

The engine digest (a short two-site DMRG run: some dozens of solves back to back out of the backend's pool) must be the
same bits in all four children: with the pool handing out NaN-filled blocks this is what guards the host drains the driver
no longer has.
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

SIZES = [3000, 63, 1025]
NFS = [0, 3]
TOL = 1e-10
MODES = ["auto", "never", "always"]


def problem(n):
    """H, K, random start vector, three frozen rows: the same arrays in the parent and in every child"""
    m, nc = rk.factor(n)
    H, K = rk.make_operator(100 + n % 97, m, nc)
    rng = np.random.default_rng(5000 + n)
    return H, K, rk.rand_z(rng, n), rk.random_rows(rng, 3, n)


def f64_solve(H, K, x0, kd, tol, max_restart, Q):
    """the float64 statement -> n_matvec (= steps), (cycle, step) of the stop, residual of the last two steps / tol, x"""
    cpu = NumpyOps()
    n = x0.size
    V = cpu.zeros_z((kd + 2) * n)
    V[0:n] = x0
    rec = {}
    _, nmv, res = cpu.lanczos(rk.sylvester_stages(cpu, H, K), 0, 1, V, n, kd, tol, max_restart, frozen=Q, record=rec)
    return nmv, rec["stop"], res, V[0:n].copy()


def warm_start(H, K, x0, Q):
    nmv, stop, res, x = f64_solve(H, K, x0, 23, 1e-9, 50, Q)
    assert res < 1e-9
    return x


def solves(n, nf, warm, kd_last):
    """name -> (start vector, krylovdim, tol, max_restart)"""
    H, K, x0, Q3 = problem(n)
    return {"inside": (warm, 23, TOL, 5), "last": (warm, kd_last, TOL, 5), "restarts": (x0, 6, TOL, 400), "tol0": (x0, 9, 0.0, 1)}


# ---- the child: every solve of every (n, nf) on the GPU, and the engine digest ------------------------------------------
def _digest(eig, nmv, res, x):
    return [float(eig).hex(), int(nmv), float(res).hex(), hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()]


def child_run(plan):
    """plan: {"n:nf": {"warm": [re, im] lists, "kd_last": int}} -> {"n:nf:name": [eig.hex, n_matvec, res.hex, sha256(x)]}"""
    import torch
    from hubbardtn_amd.device import HipOps
    ops = HipOps(0)
    out = {}
    for key, item in plan.items():
        n, nf = (int(t) for t in key.split(":"))
        H, K, x0, Q3 = problem(n)
        stages = rk.sylvester_stages(ops, H, K)
        Qd = ops.to_device(Q3.reshape(-1)) if nf else None
        warm = np.array(item["warm"][0]) + 1j * np.array(item["warm"][1])
        cases = solves(n, nf, warm, item["kd_last"])

        def enqueue(name, nan_rows=False):
            start, kd, tol, mr = cases[name]
            V = ops.zeros_z((kd + 2) * n)
            if nan_rows:
                V[n:] = complex(float("nan"), float("nan"))
                ops._lan_scratch.fill_(complex(float("nan"), float("nan")))
            V[0:n] = ops.to_device(start)
            if nf == 0:
                eig, nmv, res = ops.lanczos(stages, 0, 1, V, n, kd, tol, mr)
            else:
                eig, nmv, res = ops.lanczos_orth(stages, 0, 1, V, n, kd, tol, mr, Qd, nf)
            return eig, nmv, res, V
        for name in cases:
            eig, nmv, res, V = enqueue(name)
            out["%s:%s" % (key, name)] = _digest(eig, nmv, res, ops.to_host(V[0:n]))
        a = enqueue("inside", nan_rows=True)
        b = enqueue("restarts", nan_rows=True)               # (no wait since `a` was enqueued)
        out["%s:pair_inside" % key] = _digest(*a[:3], ops.to_host(a[3][0:n]))
        out["%s:pair_restarts" % key] = _digest(*b[:3], ops.to_host(b[3][0:n]))
    out["engine"] = engine_digest(ops)
    torch.cuda.synchronize()
    return out


def engine_digest(ops):
    """a short two-site DMRG run through the C ABI: energies after every sweep and the centre Schmidt spectrum, as hex"""
    from hubbardtn_amd import engine, models, mps
    L = 12
    H = models.hamiltonian(models.OB_Sim([1.0], [4.0]), L)
    bonds, tens = mps.random_mps(L, (L, 0), 4, seed=11)
    eng = engine.DMRG2(ops, H, bonds, tens, chi_full=48, lanczos_tol=1e-10)
    Es = [float(eng.sweep()) for _ in range(3)]
    spec = eng.spectrum(L // 2)
    return {"E": [e.hex() for e in Es], "spec": {f"{c[0]},{c[1]}": [float(x).hex() for x in v] for c, v in sorted(spec.items())},
            "n_matvec": int(sum(s.n_matvec for s in eng.stats))}


if __name__ == "__main__":
    print("RESULT " + json.dumps(child_run(json.load(open(sys.argv[1])))))
    sys.exit(0)


pytestmark = pytest.mark.gpu


# ---- the parent: float64 statement once, one child per mode --------------------------------------------------------------
@pytest.fixture(scope="module")
def reference():
    """{"n:nf": {"warm", "kd_last", name: (steps, (cycle, step), kd)}} from the float64 statement (CPU, computed once)"""
    ref = {}
    for n in SIZES:
        H, K, x0, Q3 = problem(n)
        for nf in NFS:
            Q = Q3 if nf else None
            warm = warm_start(H, K, x0, Q)
            steps, stop, res, _ = f64_solve(H, K, warm, 23, TOL, 5, Q)
            assert stop[0] == 0 and 2 <= stop[1] <= 16, ("`inside` must converge well inside the first cycle", n, nf, stop)
            item = {"warm": warm, "kd_last": stop[1] + 1}
            for name, (start, kd, tol, mr) in solves(n, nf, warm, stop[1] + 1).items():
                steps, stop, res, _ = f64_solve(H, K, start, kd, tol, mr, Q)
                item[name] = (steps, stop, kd)
                print("float64 statement n", n, "nf", nf, name, "kd", kd, "steps", steps, "stop", stop, "res", res)
            assert item["last"][1] == (0, item["kd_last"] - 1)
            assert item["restarts"][1][0] >= 3
            assert item["tol0"][0] == 18
            ref["%d:%d" % (n, nf)] = item
    return ref


def _child(plan_path, **extra):
    env = dict(os.environ, **extra)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), plan_path], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])   # (a child that died: nothing further runs here)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.fixture(scope="module")
def runs(reference, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lanczos_close") / "plan.json")
    with open(path, "w") as f:
        json.dump({k: {"warm": [v["warm"].real.tolist(), v["warm"].imag.tolist()], "kd_last": v["kd_last"]} for k, v in reference.items()}, f)
    got = {mode: _child(path, HTN_LANCZOS_CLOSE=mode) for mode in MODES}
    got["poison"] = _child(path, HTN_LANCZOS_CLOSE="auto", HTN_DEBUG_POISON="1")
    return got


@pytest.mark.parametrize("nf", NFS)
@pytest.mark.parametrize("n", SIZES)
def test_modes_agree_bit_for_bit_and_count_what_they_enqueue(reference, runs, n, nf):
    key = "%d:%d" % (n, nf)
    for name in ("inside", "last", "restarts", "tol0"):
        steps, stop, kd = reference[key][name]
        a, v, w = (runs[m]["%s:%s" % (key, name)] for m in MODES)
        print(key, name, "steps", steps, "stop", stop, "kd", kd, "matvecs auto / never / always", a[1], v[1], w[1],
              "eig", float.fromhex(v[0]), "res", float.fromhex(v[2]))
        assert a[0] == v[0] == w[0] and a[2] == v[2] == w[2], (key, name, "eigenvalue / residual")
        assert a[3] == v[3] == w[3], (key, name, "returned vector")
        assert np.isfinite(float.fromhex(v[0])) and (name == "tol0" or float.fromhex(v[2]) < TOL)
        assert w[1] == steps, (key, name, "always: one matvec per step, nothing speculative")
        assert v[1] == steps + (1 if stop[1] < kd - 1 else 0), (key, name, "never: the speculative step and nothing else")
        assert w[1] <= a[1] <= v[1], (key, name)
        if name == "tol0":
            assert a[1] == v[1] == 18
        if name == "last":
            assert a[1] == v[1] == w[1]


@pytest.mark.parametrize("mode", MODES + ["poison"])
def test_back_to_back_solves_reproduce_the_solves_run_alone(runs, mode):
    """nothing waits between the two solves, their Krylov rows and the scratch start as NaN (in the `poison` child the
    scratch of the backend and every pool block as well): the bits of each solve run alone, un-poisoned"""
    for n in SIZES:
        for nf in NFS:
            key = "%d:%d" % (n, nf)
            for name in ("inside", "restarts"):
                assert runs[mode]["%s:pair_%s" % (key, name)] == runs["auto" if mode == "poison" else mode]["%s:%s" % (key, name)], (key, name)
                assert runs[mode]["%s:%s" % (key, name)][0::2] == runs["never"]["%s:%s" % (key, name)][0::2], (key, name)
                assert runs[mode]["%s:%s" % (key, name)][3] == runs["never"]["%s:%s" % (key, name)][3], (key, name)


def test_engine_run_is_the_same_bits_in_every_mode_and_with_a_poisoned_pool(runs):
    """dozens of bond updates back to back: every solve returns with its Ritz vector in flight and the SVD, the pool and the
    next solve follow on the stream"""
    ref = runs["never"]["engine"]
    assert all(np.isfinite(float.fromhex(x)) for x in ref["E"])
    for mode in ("auto", "always", "poison"):
        got = runs[mode]["engine"]
        print(mode, "matvecs", got["n_matvec"], "never", ref["n_matvec"])
        assert got["E"] == ref["E"] and got["spec"] == ref["spec"], mode
    assert runs["always"]["engine"]["n_matvec"] <= runs["auto"]["engine"]["n_matvec"] <= ref["n_matvec"]
    assert runs["poison"]["engine"]["n_matvec"] == runs["auto"]["engine"]["n_matvec"]
