"""The library's IDMRG2 driver (htn_idmrg_*, driver="native") on the GPU: every infinite-chain constant the reference's
tests pin, at the bounds of tests/test_idmrg_gpu.py, and step-for-step agreement with the Python loop."""
import json
import os
import time

import numpy as np
import pytest

from hubbardtn_amd import api, idmrg, models

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_constants.json")))


def _energy(d):
    return float(np.sum(np.real(api.expectation_value(d["groundstate"], d["ham"])))) / len(d["ham"])


@pytest.mark.parametrize("rec", GOLD["OB_parameters"] + GOLD["OB_filling"], ids=lambda r: f"U{r['u'][0]:g}_P{r['P']}Q{r['Q']}")
def test_native_reference_infinite_chain_constants(rec):
    model = api.OB_Sim(rec["t"], rec["u"], 0.0, rec["P"], rec["Q"], rec["svalue"])
    d = api.produce_groundstate(model, tol=1e-5, maxiter=60, driver="native")
    E = _energy(d)
    assert abs(E - rec["E_per_site"]) < rec["atol"] and abs(E - rec["E_per_site"]) < 1e-3
    assert len(api.dim_state(d["groundstate"])) == len(d["ham"]) == idmrg.unit_cell(rec["P"], rec["Q"])


def test_native_two_band_spinful_and_chemical_potential_cases():
    rec = GOLD["MB_groundstate"]
    model = api.MB_Sim(np.array(rec["t"]), np.array(rec["u"]), np.array(rec["J"]), rec["P"], rec["Q"], rec["svalue"], rec["bond_dim"])
    assert abs(_energy(api.produce_groundstate(model, tol=1e-4, maxiter=40, driver="native")) - rec["E_per_site"]) < rec["atol"]
    d1 = api.produce_groundstate(api.OB_Sim([1.0], [8.0], 0.0, 1, 1, 2.0, spin=True), tol=1e-4, maxiter=40, driver="native")
    E1 = _energy(d1)
    assert abs(E1 - (-0.32637)) < 2e-3
    t = np.array([[0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    u = np.array([[3.0, 0.0, 0.0, 0.0], [0.0, 3.0, 0.0, 0.0]])
    d2 = api.produce_groundstate(api.MB_Sim(t, u, np.zeros((2, 2)), 1, 1, 2.0, 20, code="Spin", spin=True), tol=1e-4,
                                 maxiter=40, driver="native")
    assert len(d2["ham"]) == 4 and abs(_energy(d2) - (-0.63093)) < 3e-2
    for d in (d1, d2):
        n = api.density_state(d["groundstate"])
        up, dn = api.density_spin(d["groundstate"])
        assert abs(n.sum() - (up + dn).sum()) < 1e-8 and abs(n.sum() / len(d["ham"]) - 1.0) < 5e-3
    d = api.produce_groundstate(api.OBC_Sim2([1.0], [1.0], 0.5, 2.0), tol=1e-4, maxiter=40, driver="native")
    n = api.density_state(d["groundstate"])
    E0 = float(np.sum(api.expectation_value(d["groundstate"], d["ham"]))) / len(d["ham"]) + 0.5 * float(n.mean())
    assert np.abs(n - 1.0).max() < 1e-5 and abs(E0 - (-1.03541433)) < 1e-3, E0
    t = np.array([[0.5, 0.0, 1.0, 0.0], [0.0, 0.5, 0.0, 1.0]])
    u = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]])
    db = api.produce_groundstate(api.MBC_Sim(t, u, np.zeros((2, 2)), 2.0, 20, code="MBC"), tol=1e-4, maxiter=40, driver="native")
    nb = api.density_state(db["groundstate"])
    Eb = (float(np.sum(api.expectation_value(db["groundstate"], db["ham"]))) + 0.5 * float(nb.sum())) / len(db["ham"])
    assert abs(Eb - (-1.01631556)) < 1e-1 and Eb > -1.0404


def test_native_and_python_loops_agree_on_the_hip_backend(hip_ops):
    """one Bethe-ansatz case at truncdim(120): same step count, same energy density; wall times of both drivers printed"""
    rec = max(GOLD["OB_parameters"], key=lambda r: r["u"][0])
    sim = models.OB_Sim(rec["t"], rec["u"])
    t0 = time.perf_counter()
    a = idmrg.idmrg2(hip_ops, sim, chi_full=120, tol=1e-4, maxiter=25, driver="native")
    t1 = time.perf_counter()
    b = idmrg.idmrg2(hip_ops, sim, chi_full=120, tol=1e-4, maxiter=25, driver="python")
    t2 = time.perf_counter()
    print(f"\nIDMRG2 chi=120 U={rec['u'][0]:g}: native {t1 - t0:.2f} s, python {t2 - t1:.2f} s, {a.iterations} steps, "
          f"{a.sweeps} / {b.sweeps} sweeps")
    assert a.iterations == b.iterations
    assert abs(a.energy_per_site - b.energy_per_site) <= 1e-9
    assert abs(a.energy_per_site - rec["bethe"]) < 4e-4
