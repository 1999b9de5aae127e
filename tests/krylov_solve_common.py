"""Shared by test_krylov_solve_cpu.py / test_krylov_solve_gpu.py: the cases of htn_krylov_solve_z -- a dense Hermitian H as one
grouped-GEMM stage (krylov_expm_common.tasks_for), (z - H) x = b against numpy.linalg.solve -- and a numpy statement of the
same algorithm (restarted minimal residual on the Lanczos basis, Givens rotations on the shifted tridiagonal matrix), whose
matvec count the library must reproduce."""
import functools

import numpy as np

from hubbardtn_amd import abi
from krylov_expm_common import rand_z, tasks_for        # noqa: F401  (tasks_for: used by the two test files)

TOL = 1e-12          # tolerance handed to the solver
GATE = 1e-10         # |b - (z - H) x| <= GATE |b|: 100 x tol, the recurrence residual is not the true one


@functools.lru_cache(maxsize=None)
def problem(name):
    """-> dict(H, b, kd, z, max_restart, ...): the table of the issue.  |H| is the spectral norm, set exactly through eigh."""
    spec = {"a": (1000, 30, 1.0, 0.3 + 0.5j, 50), "b": (257, 8, 4.0, 0.5 + 0.2j, 4000), "c": (64, 10, 3.0, 0.2 + 0.4j, 2),
            "d": (257, 30, 4.0, -1.0 - 0.3j, 50), "e": (130, 10, 2.0, 0.1 + 0.3j, 2), "f": (130, 2, 1.0, 0.2 + 0.5j, 4000)}[name]
    n, kd, hnorm, z, mr = spec
    rng = np.random.default_rng(2000 + ord(name))
    H = rand_z(rng, n * n).reshape(n, n)
    H = H + H.conj().T
    w, U = np.linalg.eigh(H)
    H *= hnorm / np.abs(w).max()
    w, U = np.linalg.eigh(H)
    b = rand_z(rng, n)
    lam = None
    if name == "c":
        b = U[:, 17] * (0.3 - 1.1j)                  # an eigenvector, not normalised
        lam = w[17]
    x_ref = np.linalg.solve(z * np.eye(n) - H, b)
    guess = x_ref.copy() if name == "e" else None    # (e) the start value is the solution
    return dict(name=name, n=n, H=H, w=w, b=b, kd=kd, z=complex(z), max_restart=mr, x_ref=x_ref, guess=guess, lam=lam)


def model(H, b, z, kd, tol, max_restart, x0=None):
    """the algorithm in numpy: -> (x, matvecs, restarts, steps of the last cycle, relative residual of the recurrence)"""
    n = len(b)
    bnorm = np.linalg.norm(b)
    x = np.zeros(n, dtype=complex) if x0 is None else np.array(x0, dtype=complex)
    nmv = 0
    r = np.array(b, dtype=complex)
    if x0 is not None:
        r = b - z * x + H @ x
        nmv += 1
    beta0 = np.linalg.norm(r)
    if beta0 <= tol * bnorm:
        return x, nmv, 0, 0, beta0 / bnorm
    amax = 0.0
    for restart in range(max_restart + 1):
        V = np.zeros((kd + 1, n), dtype=complex)
        V[0] = r / beta0
        T = np.zeros((kd + 1, kd), dtype=complex)
        conv = False
        for j in range(kd):
            w = H @ V[j]
            nmv += 1
            alpha = 0.0
            for _ in range(2):                                  # full two-pass Gram-Schmidt
                c = V[:j + 1].conj() @ w
                alpha += c[j].real
                w = w - c @ V[:j + 1]
            beta = np.linalg.norm(w)
            amax = max(amax, abs(alpha), beta)
            T[j, j] = alpha
            T[j + 1, j] = beta
            if j + 1 < kd:
                T[j, j + 1] = beta
            m = j + 1
            A = z * np.eye(m + 1, m) - T[:m + 1, :m]
            rhs = np.zeros(m + 1, dtype=complex)
            rhs[0] = beta0
            y = np.linalg.lstsq(A, rhs, rcond=None)[0]
            rho = rhs - A @ y
            res = np.linalg.norm(rho) / bnorm
            invariant = beta < 1e-14 * max(amax, 1e-300)
            conv = res <= tol or invariant
            if conv or m == kd:
                break
            V[j + 1] = w / beta
        x = x + y @ V[:m]
        if conv:
            return x, nmv, restart, m, res
        V[m] = w / beta
        r = rho @ V[:m + 1]
        beta0 = np.linalg.norm(rho)
    return x, nmv, max_restart, m, res


@functools.lru_cache(maxsize=None)
def model_of(name):
    p = problem(name)
    return model(p["H"], p["b"], p["z"], p["kd"], TOL, p["max_restart"], p["guess"])


def check(name, got, speculative=0):
    """got = (norm, residual, n_matvec, x, V[0]).  Asserts the gates of the issue; -> n_matvec"""
    p = problem(name)
    nrm, res, nmv, x, v0 = got
    H, b, z = p["H"], p["b"], p["z"]
    bn = np.linalg.norm(b)
    true_res = np.linalg.norm(b - (z * x - H @ x)) / bn
    err = np.linalg.norm(x - p["x_ref"]) / bn
    xm, nmv_m, restarts, last, res_m = model_of(name)
    spec = speculative if 0 < last < p["kd"] else 0            # a cycle that ends below krylovdim has one step in flight behind it
    print(f"case {name}: n {p['n']} kd {p['kd']} z {z} matvecs {nmv} (model {nmv_m} + {spec}, {restarts} restarts) recurrence residual "
          f"{res:.3e} true residual {true_res:.3e} |x - ref|/|b| {err:.3e} (bound {GATE / abs(z.imag):.1e})")
    assert true_res <= GATE
    assert err <= GATE / abs(z.imag)
    assert abs(nrm - np.linalg.norm(p["x_ref"])) <= GATE * bn / abs(z.imag)
    assert abs(np.linalg.norm(v0) - 1.0) <= 1e-12
    assert np.linalg.norm(v0 * nrm - x) <= 1e-12 * max(nrm, 1.0)
    assert nmv == nmv_m + spec, (nmv, nmv_m, spec)
    return nmv, restarts


def run_cases(solve, speculative=0):
    """solve(problem, kd, z, tol, max_restart, guess) -> (norm, residual, n_matvec, x, V[0]).  speculative: matvecs a pipelined
    driver enqueues beyond the last one it uses (GPU: 1)"""
    for name in "abcdef":
        p = problem(name)
        nmv, restarts = check(name, solve(p, p["kd"], p["z"], TOL, p["max_restart"], p["guess"]), speculative)
        if name == "a":
            assert restarts == 1                                  # one restart
        if name in "bf":
            assert restarts > 10                                  # many restarts
        if name == "c":
            assert nmv == 1 + speculative                         # an eigenvector: one step
            x = solve(p, p["kd"], p["z"], TOL, p["max_restart"], None)[3]
            assert np.linalg.norm(x - p["b"] / (p["z"] - p["lam"])) <= 1e-12
        if name == "e":
            assert nmv == 1                                       # the matvec of r0, nothing else
            x = solve(p, p["kd"], p["z"], TOL, p["max_restart"], p["guess"])[3]
            assert np.linalg.norm(x - p["guess"]) <= 1e-12
    # no restart allowed and a tolerance that cannot be met: a clean error that names what remains, then business as usual
    p = problem("b")
    try:
        solve(p, p["kd"], p["z"], 1e-300, 0, None)
    except abi.HtnError as ex:
        assert "remains" in str(ex), str(ex)
    else:
        raise AssertionError("max_restart = 0 with an unreachable tolerance must fail")
    pa = problem("a")
    check("a", solve(pa, pa["kd"], pa["z"], TOL, pa["max_restart"], None), speculative)
    for bad in (1, 32):
        try:
            solve(problem("e"), bad, 0.1 + 0.3j, TOL, 2, None)
        except abi.HtnError as ex:
            assert "krylovdim" in str(ex)
        else:
            raise AssertionError("krylovdim outside 2..31 must fail")
