"""The library's step-wise IDMRG2 driver (htn_idmrg_*, include/hubbardtn_hip.h) on the CPU baseline backend: the growth
loop through the C ABI alone against one of the reference's own infinite-chain constants (test/OB.jl:44-54), step by
step against the Python loop of hubbardtn_amd/idmrg.py with the same seeds, the needs_window protocol, error returns
and handle lifetimes, and the whole Python API on a native result."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from cpu_ops import CpuOps
from hubbardtn_amd import abi, models, mps

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_constants.json")))


# ---- the C ABI driven by hand: tables from models / mps, nothing from engine or idmrg ----------------------------------
def _window_mpo(sim):
    """the 2T translation-invariant MPO sites of a window (the bulk of a long open chain) and T"""
    P, Q = int(sim.P), int(sim.Q)
    T = (Q if P % 2 == 0 else 2 * Q) * int(sim.bands)
    big = models.hamiltonian(sim, 8 * max(T // int(sim.bands), 1))
    return [big[3 * T + i] for i in range(2 * T)], T, (2 * T * P) // Q


def _mpo_create(lib, ctx, sites, msym):
    names = sorted({e[2] for s in sites for e in s.entries})
    index = {n: k for k, n in enumerate(names)}
    optab = np.zeros(len(names), dtype=abi.SITE_OP_DT)
    for n, k in index.items():
        kk, dN, red = msym.site_ops[n]
        r = np.zeros((abi.MAX_SITE, abi.MAX_SITE))
        r[:red.shape[0], :red.shape[1]] = red
        optab[k]["k"], optab[k]["dN"], optab[k]["red"] = kk, dN, r.reshape(-1)
    levels, level_ptr = [], [0]
    for lv in [sites[0].left] + [s.right for s in sites]:
        levels.extend(lv)
        level_ptr.append(level_ptr[-1] + len(lv))
    ent = np.zeros(sum(len(s.entries) for s in sites), dtype=abi.MPO_ENTRY_DT)
    entry_ptr, q = [0], 0
    for s in sites:
        for (wl, wr, name, coef) in s.entries:
            ent[q] = (wl, wr, index[name], 0, complex(coef).real, complex(coef).imag)
            q += 1
        entry_ptr.append(q)
    sym = abi.Symmetry()
    sym.kind, sym.n_site = msym.kind, len(msym.site_mult)
    for s, (N, j) in enumerate(msym.site_mult):
        sym.site_N[s], sym.site_j[s] = N, j
    lv = np.array(levels, dtype=np.int32).reshape(-1, 2)
    lp, ep = np.array(level_ptr, dtype=np.int32), np.array(entry_ptr, dtype=np.int32)
    h = C.c_void_p()
    abi.check(lib, lib.htn_mpo_create(ctx, C.byref(sym), len(sites), optab.ctypes.data, len(names), lp.ctypes.data,
                                      lv.ctypes.data, ep.ctypes.data, ent.ctypes.data, C.byref(h)), "htn_mpo_create")
    return h


def _tables(bonds, tensors):
    secs, bond_ptr = [], [0]
    for b in bonds:
        secs.extend((N, j, n) for (N, j), n in sorted(b.items()) if n > 0)
        bond_ptr.append(len(secs))
    sec = np.array(secs, dtype=np.int32).reshape(-1, 3).view(abi.SECTOR_DT).reshape(-1)
    subs, sub_ptr, data_ptr, chunks = [], [0], [0], []
    for t in tensors:
        off = 0
        for (l, s, r), blk in t.items():
            subs.append((l[0], l[1], s, r[0], r[1], blk.shape[0], 0, off))
            chunks.append(np.asfortranarray(blk, dtype=np.complex128).reshape(-1, order="F"))
            off += blk.size
        sub_ptr.append(len(subs))
        data_ptr.append(data_ptr[-1] + off)
    sb = np.array([tuple(x[:6]) + (x[7],) for x in subs], dtype=abi.SUBBLOCK_DT)
    arrays = (np.array(bond_ptr, dtype=np.int32), np.ascontiguousarray(sec), np.array(sub_ptr, dtype=np.int32), sb,
              np.array(data_ptr, dtype=np.int64), np.concatenate(chunks))
    return arrays, [a.ctypes.data for a in arrays]


def _boundary(lib, h, side):
    n = lib.htn_idmrg_boundary(h, side, None)
    arr = np.zeros(n, dtype=abi.SECTOR_DT)
    assert lib.htn_idmrg_boundary(h, side, arr.ctypes.data) == n
    return {(int(r["N"]), int(r["j"])): int(r["count"]) for r in arr}


def _opts(T, dNw, chi_full=0, cutoff=0.0, tol=1e-4, maxiter=10, sweeps_per_step=6, warm_start=1, lanczos_tol=1e-10):
    o = abi.IdmrgOpts()
    o.sweep.chi_full, o.sweep.cutoff, o.sweep.krylovdim, o.sweep.maxrestart = chi_full, cutoff, 30, 3
    o.sweep.lanczos_tol, o.sweep.jacobi_tol, o.sweep.jacobi_max_sweeps = lanczos_tol, 1e-14, 40
    o.cell_sites, o.window_dN, o.tol, o.min_steps, o.maxiter = T, dNw, tol, 3, maxiter
    o.sweeps_per_step, o.warm_start = sweeps_per_step, warm_start
    return o


def _grow(lib, ctx, mpo, W, o, init_dimension, seed, sym):
    """the growth loop through htn_idmrg_*: -> (list of stats, list of 'window supplied' flags)"""
    h = C.c_void_p()
    abi.check(lib, lib.htn_idmrg_create(ctx, mpo, C.byref(o), C.byref(h)), "htn_idmrg_create")
    steps, supplied, needs = [], [], True
    try:
        while True:
            st = abi.IdmrgStats()
            if needs:
                bonds, tensors = mps.random_window(W, _boundary(lib, h, 0), _boundary(lib, h, 1), init_dimension,
                                                   seed=seed + len(steps), sym=sym)
                _, ptrs = _tables(bonds, tensors)
                abi.check(lib, lib.htn_idmrg_step(h, *ptrs, C.byref(st)), "htn_idmrg_step")
            else:
                abi.check(lib, lib.htn_idmrg_step(h, None, None, None, None, None, None, C.byref(st)), "htn_idmrg_step")
            steps.append(st)
            supplied.append(needs)
            assert st.step == len(steps) - 1
            if st.finished:
                return steps, supplied
            needs = bool(st.needs_window)
    finally:
        lib.htn_idmrg_destroy(h)


@pytest.fixture(scope="module")
def cpu():
    return CpuOps()


def test_c_abi_growth_reproduces_a_reference_test_constant(cpu):
    """test/OB.jl:44-54 (U = 5, half filling, truncbelow(1e-2)) with the settings of
    test_idmrg2_reproduces_a_reference_test_constant_with_the_reference_truncation, through the C ABI alone"""
    rec = GOLD["OB_filling"][1]
    sim = models.OB_Sim(rec["t"], rec["u"], 0.0, rec["P"], rec["Q"], rec["svalue"], 8)
    sites, T, dNw = _window_mpo(sim)
    lib = cpu.lib
    mpo = _mpo_create(lib, cpu.ctx, sites, models.SU2U1)
    try:
        o = _opts(T, dNw, cutoff=10.0 ** -rec["svalue"], tol=2e-4, maxiter=14, sweeps_per_step=3, lanczos_tol=1e-9)
        steps, supplied = _grow(lib, cpu.ctx, mpo, 2 * T, o, 8, 1234, models.SU2U1)
    finally:
        lib.htn_mpo_destroy(mpo)
    e = steps[-1].energy_per_site
    assert abs(e - rec["E_per_site"]) < rec["atol"]                 # the reference's own tolerance
    assert abs(e - rec["E_per_site"]) < 5e-4
    assert steps[-1].delta < 1e-3 and steps[-1].chi_full <= 20
    assert steps[0].delta == np.inf and np.isnan(steps[0].energy_per_site)


def test_native_and_python_loops_agree_step_by_step(cpu):
    """same seeds, same rules: the steps before any prediction agree to rounding; every later step to 1e-9"""
    from hubbardtn_amd import idmrg
    sim = models.OB_Sim([1.0], [4.0], 0.0, 1, 1, 2.0, 50)
    kw = dict(chi_full=60, tol=1e-4)
    for n in (1, 2):                       # (a finished step does not absorb: its window is the step's own)
        a = idmrg.idmrg2(cpu, sim, maxiter=n, driver="native", **kw)
        b = idmrg.idmrg2(cpu, sim, maxiter=n, driver="python", **kw)
        assert a.iterations == b.iterations == n and a.sweeps == b.sweeps
        assert set(a.spectrum) == set(b.spectrum)
        for c in a.spectrum:
            assert np.abs(a.spectrum[c] - b.spectrum[c]).max() <= 1e-12
        if n == 2:
            assert abs(a.energy_per_site - b.energy_per_site) <= 1e-12 and abs(a.delta - b.delta) <= 1e-12
    a = idmrg.idmrg2(cpu, sim, maxiter=24, driver="native", **kw)
    b = idmrg.idmrg2(cpu, sim, maxiter=24, driver="python", **kw)
    assert a.iterations == b.iterations and a.sweeps == b.sweeps
    for (ea, da), (eb, db) in list(zip(a.history, b.history))[1:]:
        assert abs(ea - eb) <= 1e-9 and abs(da - db) <= 1e-8
    assert idmrg._spectrum_distance(a.spectrum, b.spectrum, 0) <= 1e-8
    assert a.bond_dims == b.bond_dims and a.boundary["bL"] == b.boundary["bL"] and a.boundary["bR"] == b.boundary["bR"]
    assert abs(a.energy_per_site - (-0.5737)) < 1e-3                  # Lieb-Wu: -0.573729


@pytest.mark.parametrize("warm", [1, 0])
def test_needs_window_protocol(cpu, warm):
    """the host supplies the first two windows (prediction from the third on), or every window without warm start"""
    sim = models.OB_Sim([1.0], [4.0], 0.0, 1, 1, 2.0, 50)
    sites, T, dNw = _window_mpo(sim)
    lib = cpu.lib
    mpo = _mpo_create(lib, cpu.ctx, sites, models.SU2U1)
    try:
        steps, supplied = _grow(lib, cpu.ctx, mpo, 2 * T, _opts(T, dNw, chi_full=40, tol=1e-12, maxiter=6, warm_start=warm),
                                8, 7, models.SU2U1)
    finally:
        lib.htn_mpo_destroy(mpo)
    assert len(steps) == 6 and steps[-1].finished and not steps[-1].converged
    assert supplied == ([True, True, False, False, False, False] if warm else [True] * 6)
    assert [s.needs_window for s in steps[:-1]] == ([1, 0, 0, 0, 0] if warm else [1] * 5)


def test_errors_and_handle_lifetimes(cpu):
    sim = models.OB_Sim([1.0], [4.0], 0.0, 1, 1, 2.0, 50)
    sites, T, dNw = _window_mpo(sim)
    W = 2 * T
    lib = cpu.lib
    ctx = C.c_void_p()
    abi.check(lib, lib.htn_ctx_create(abi.BACKEND_CPU, 0, None, C.byref(ctx)), "htn_ctx_create")
    mpo = _mpo_create(lib, ctx, sites, models.SU2U1)
    h = C.c_void_p()
    o = _opts(T, dNw, chi_full=30, maxiter=3)
    abi.check(lib, lib.htn_idmrg_create(ctx, mpo, C.byref(o), C.byref(h)), "htn_idmrg_create")
    st = abi.IdmrgStats()
    win = C.c_void_p()
    assert lib.htn_idmrg_window(h, C.byref(win)) != 0 and b"no step" in lib.htn_last_error()
    assert _boundary(lib, h, 0) == {(0, 0): 1} and _boundary(lib, h, 1) == {(W, 0): 1}
    assert lib.htn_idmrg_boundary(h, 2, None) == -1
    # a window was requested: NULL is refused
    assert lib.htn_idmrg_step(h, None, None, None, None, None, None, C.byref(st)) != 0
    assert b"needs a window from the host" in lib.htn_last_error()
    # a window whose left end table is not the boundary's: the bond and the sector are named
    bonds, tensors = mps.random_window(W, {(0, 0): 2}, {(W, 0): 1}, 8, seed=3)
    _, ptrs = _tables(bonds, tensors)
    assert lib.htn_idmrg_step(h, *ptrs, C.byref(st)) != 0
    msg = lib.htn_last_error().decode()
    assert "bond 0" in msg and "(0, 0)" in msg and "left boundary" in msg, msg
    bonds, tensors = mps.random_window(W, {(0, 0): 1}, {(W, 0): 1, (W, 2): 1}, 8, seed=3)
    _, ptrs = _tables(bonds, tensors)
    assert lib.htn_idmrg_step(h, *ptrs, C.byref(st)) != 0
    msg = lib.htn_last_error().decode()
    assert f"bond {W}" in msg and f"({W}, 2)" in msg and "right boundary" in msg, msg
    # the refused calls left the driver usable
    bonds, tensors = mps.random_window(W, {(0, 0): 1}, {(W, 0): 1}, 8, seed=3)
    arrays, ptrs = _tables(bonds, tensors)
    abi.check(lib, lib.htn_idmrg_step(h, *ptrs, C.byref(st)), "htn_idmrg_step")
    assert st.step == 0 and st.needs_window == 1 and not st.finished
    abi.check(lib, lib.htn_idmrg_window(h, C.byref(win)), "htn_idmrg_window")
    # handles released in an unusual order: context first, then the MPO, the driver, the window (each keeps what it needs)
    lib.htn_ctx_destroy(ctx)
    lib.htn_mpo_destroy(mpo)
    _, ptrs = _tables(*mps.random_window(W, _boundary(lib, h, 0), _boundary(lib, h, 1), 8, seed=4))
    abi.check(lib, lib.htn_idmrg_step(h, *ptrs, C.byref(st)), "htn_idmrg_step")
    lib.htn_idmrg_destroy(h)
    assert lib.htn_mps_nsites(win) == W
    n = lib.htn_mps_spectrum(win, T, None, None)
    assert n > 0
    lib.htn_mps_destroy(win)
    # and the other way round: window first, then the driver, the MPO, the context
    abi.check(lib, lib.htn_ctx_create(abi.BACKEND_CPU, 0, None, C.byref(ctx)), "htn_ctx_create")
    mpo = _mpo_create(lib, ctx, sites, models.SU2U1)
    abi.check(lib, lib.htn_idmrg_create(ctx, mpo, C.byref(o), C.byref(h)), "htn_idmrg_create")
    abi.check(lib, lib.htn_idmrg_step(h, *_tables(bonds, tensors)[1], C.byref(st)), "htn_idmrg_step")
    abi.check(lib, lib.htn_idmrg_window(h, C.byref(win)), "htn_idmrg_window")
    lib.htn_mps_destroy(win)
    lib.htn_idmrg_destroy(h)
    lib.htn_mpo_destroy(mpo)
    lib.htn_ctx_destroy(ctx)
    # a driver whose window MPO does not hold 2T sites is refused
    abi.check(lib, lib.htn_ctx_create(abi.BACKEND_CPU, 0, None, C.byref(ctx)), "htn_ctx_create")
    mpo = _mpo_create(lib, ctx, sites, models.SU2U1)
    o.cell_sites = T + 1
    assert lib.htn_idmrg_create(ctx, mpo, C.byref(o), C.byref(h)) != 0 and b"cell_sites" in lib.htn_last_error()
    lib.htn_mpo_destroy(mpo)
    lib.htn_ctx_destroy(ctx)


def test_whole_api_on_a_native_result(cpu, tmp_path):
    """find_groundstate(InfiniteMPS, H, IDMRG2(driver="native")) -> a state the rest of the API works on"""
    from hubbardtn_amd import api, engine, storage
    rec = GOLD["OB_filling"][1]
    sim = api.OB_Sim(rec["t"], rec["u"], 0.0, rec["P"], rec["Q"], rec["svalue"], 8)
    H = api.hamiltonian(sim)
    psi = api.initialize_mps(H, sim.P, sim.bond_dim, ops=cpu)
    alg = api.IDMRG2(trscheme=api.truncbelow(10.0 ** -sim.svalue), tol=2e-4, maxiter=14, eigsolve_tol=1e-9,
                     sweeps_per_step=3, driver="native")
    psi, envs, delta = api.find_groundstate(psi, H, alg)
    e = api.expectation_value(psi, H)
    assert e.shape == (2,) and abs(e[0] - rec["E_per_site"]) < 5e-4
    assert delta < 1e-3 and len(api.dim_state(psi)) == len(H) and max(api.dim_state(psi)) <= 20
    n = api.density_state(psi)
    assert n.shape == (len(H),) and abs(n.mean() - 1.0) < 1e-6
    eng = psi.result.engine
    assert isinstance(eng, engine.DMRG2) and eng.L == 4 and envs.engine is eng
    p = storage.save_state(psi, str(tmp_path), "psi")
    bonds, sites = storage.load_state(p)
    re_ = engine.DMRG2(cpu, eng.cmpo, bonds, [s["blocks"] for s in sites], cutoff=eng.cutoff,
                       left_env=psi.result.boundary["Lenv"], right_env=psi.result.boundary["Renv"])
    for i in range(eng.L):
        a, b = eng.download_site(i), re_.download_site(i)
        assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert re_.bond_dims() == eng.bond_dims()
    # the python default is unchanged
    assert api.IDMRG2().driver == "python"
    with pytest.raises(ValueError):
        from hubbardtn_amd import idmrg
        idmrg.idmrg2(cpu, sim, driver="julia")
