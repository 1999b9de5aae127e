"""Shared by test_krylov_expm_cpu.py / test_krylov_expm_gpu.py: the cases of htn_krylov_expm_z -- a dense Hermitian H as one
grouped-GEMM stage, x = exp(-i dt H) x0 against eigh, the reference itself checked by a second route (a Taylor series in
extended precision over sub-steps of |dt| |H| <= 1/2)."""
import functools

import numpy as np

from hubbardtn_amd import abi
from ref_planner import TaskList

TOL = 1e-12          # tolerance handed to the solver in the accuracy cases
GATE = 1e-10         # |x - x_ref| <= GATE |x0|, |growth - ref| <= GATE ref: Saad's estimate is an estimate, not a bound


def rand_z(rng, n):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def tasks_for(n):
    """y[n x 1] = H[n x n] x[n x 1]: buffer 0 = x, 1 = y, 2 = H (column major)"""
    tl = TaskList()
    tl.block(0, 1, 0, n, 1, n)
    tl.gemm(0, 2, 0, n, abi.OP_N, 0, 0, n, abi.OP_N, n, 1.0)
    return tl.finalize()


@functools.lru_cache(maxsize=None)
def problem(name):
    """-> dict(H, x0, kd, dt, max_restart): the table of the issue.  |H| is the spectral norm, set exactly through eigh."""
    spec = {"a": (1000, 30, 1.0, 1.0, 8), "b": (257, 8, 40.0, 1.0, 4000), "c": (64, 10, 3.0, 1.0, 2),
            "d": (257, 30, 4.0, -0.7j, 8), "e": (130, 10, 2.0, 0.0, 2), "f": (130, 2, 1.0, 1e-5, 4000)}[name]
    n, kd, hnorm, dt, mr = spec
    rng = np.random.default_rng(1000 + ord(name))
    H = rand_z(rng, n * n).reshape(n, n)
    H = H + H.conj().T
    w, U = np.linalg.eigh(H)
    H *= hnorm / np.abs(w).max()
    w, U = np.linalg.eigh(H)
    x0 = rand_z(rng, n)
    if name == "c":
        x0 = U[:, 17] * (0.3 - 1.1j)                 # an eigenvector, not normalised
    return dict(name=name, n=n, H=H, w=w, U=U, x0=x0, kd=kd, dt=complex(dt), max_restart=mr)


@functools.lru_cache(maxsize=None)
def reference(name):
    """exp(-i dt H) x0 by eigh, confirmed to 1e-11 |x0| by the Taylor series in extended precision"""
    p = problem(name)
    x = p["U"] @ (np.exp(-1j * p["dt"] * p["w"]) * (p["U"].conj().T @ p["x0"]))
    hn = np.abs(p["w"]).max() * abs(p["dt"])
    nsub = max(1, int(np.ceil(2.0 * hn)))
    Hl = (-1j * p["dt"] / nsub * p["H"]).astype(np.clongdouble)
    y = p["x0"].astype(np.clongdouble)
    for _ in range(nsub):
        term, acc = y.copy(), y.copy()
        for k in range(1, 40):
            term = (Hl @ term) / k
            acc = acc + term
        y = acc
    dev = float(np.linalg.norm((y - x).astype(np.complex128))) / np.linalg.norm(p["x0"])
    assert dev <= 1e-11, (name, dev)
    return x, dev


def check(name, got, report):
    """got = (growth, alpha0, n_matvec, err, x normalised).  Asserts the gate; report(name, error, growth error) records figures"""
    p = problem(name)
    growth, a0, nmv, err, x = got
    ref, dev = reference(name)
    n0 = np.linalg.norm(p["x0"])
    e_x = np.linalg.norm(growth * n0 * x - ref) / n0
    g_ref = np.linalg.norm(ref) / n0
    e_g = abs(growth - g_ref) / g_ref
    a_ref = (np.vdot(p["x0"], p["H"] @ p["x0"]) / n0 ** 2).real
    print(f"case {name}: n {p['n']} kd {p['kd']} matvecs {nmv} estimate {err:.3e} |x - ref|/|x0| {e_x:.3e} growth err {e_g:.3e} "
          f"reference routes differ by {dev:.1e}")
    report(name, e_x, e_g)
    assert abs(np.linalg.norm(x) - 1.0) <= 1e-12
    assert abs(a0 - a_ref) <= 1e-12 * max(1.0, np.abs(p["w"]).max())
    assert e_x <= GATE and e_g <= GATE
    return nmv


def run_cases(solve, report=lambda *a: None, speculative=0):
    """solve(problem, kd, dt, tol, max_restart) -> (growth, alpha0, n_matvec, err, x).  speculative: matvecs a pipelined
    driver enqueues beyond the last one it uses (GPU: 1)"""
    for name in "abcdef":
        p = problem(name)
        nmv = check(name, solve(p, p["kd"], p["dt"], TOL, p["max_restart"]), report)
        if name == "a":
            assert nmv <= p["kd"] - 1 + speculative               # converges below krylovdim
        if name == "b":
            assert nmv > p["kd"]                                  # sub-stepping was needed
        if name == "c":
            assert nmv <= 1 + speculative                         # an eigenvector: one step, the pure phase
            x = solve(p, p["kd"], p["dt"], TOL, p["max_restart"])[4]
            ph = np.exp(-1j * p["dt"] * p["w"][17]) * p["x0"] / np.linalg.norm(p["x0"])
            assert np.linalg.norm(x - ph) <= 1e-12
        if name == "d":
            assert abs(np.linalg.norm(solve(p, p["kd"], p["dt"], TOL, p["max_restart"])[4]) - 1.0) <= 1e-12
        if name == "e":
            assert nmv <= 1                                       # dt = 0: the identity
        if name == "f":
            assert nmv > 2
    # (g) no restart allowed and a tolerance that cannot be met: a clean error that names what remains, then business as usual
    p = problem("b")
    try:
        solve(p, 4, p["dt"], 1e-300, 0)
    except abi.HtnError as ex:
        assert "remains" in str(ex), str(ex)
    else:
        raise AssertionError("max_restart = 0 with an unreachable tolerance must fail")
    check("a", solve(problem("a"), 30, 1.0, TOL, 8), report)
    for bad in (1, 32, 40):
        try:
            solve(problem("e"), bad, 0.1, TOL, 2)
        except abi.HtnError as ex:
            assert "krylovdim" in str(ex)
        else:
            raise AssertionError("krylovdim outside 2..31 must fail")
