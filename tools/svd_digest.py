"""Bit-level fingerprint of htn_jacobi_svd_z, for refactors of the SVD kernels that must not change what they compute.

    python tools/svd_digest.py [--lib path/to/libhubbardtn_hip.so]

Runs fixed seeded blocks, one call each, through every path of the Jacobi SVD and prints one line per case: the first 32 hex
digits of a sha256 over S, G, Vj and info, then info (Jacobi sweeps per block) and the outer sweeps of the multi-workgroup
paths.  Two builds of the library compute the same thing exactly when all lines agree.  The switches are read once per
process, so every setting runs in a child of its own, under its own time limit; the chain stops at the first child that
fails.  Without --lib the library of this tree is fingerprinted (hubbardtn_amd/build.py builds it), with --lib that file.

    setting            path            case
    default            one workgroup   64 x 64 accumulate; 130 x 90
    default            ring            230 x 230 QRCP (its digest differs from the pair visits' one below: other rotation order)
    HTN_SVD_PAIRS=1    pair visits     230 x 230 QRCP; 202 x 150 QRCP (column counts no multiples of 8: dead slots in cross and
                                       intra visits)
    default            tall            520 x 530 plain; 600 x 40 accumulate (both tall_apply calls, dead slots)
"""
from __future__ import annotations

import argparse
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, m, n, QRCP, accumulate, decades of the graded spectrum.  QRCP: G0 is m x n, the result n x min(m, n)
SETTINGS = {
    "default": [("one workgroup 64 x 64 accumulate", 64, 64, False, True, 12),
                ("one workgroup 130 x 90", 130, 90, False, False, 10),
                ("ring 230 x 230 QRCP", 230, 230, True, False, 12),
                ("tall 520 x 530", 520, 530, False, False, 12),
                ("tall 600 x 40 accumulate", 600, 40, False, True, 10)],
    "HTN_SVD_PAIRS": [("pair visits 230 x 230 QRCP", 230, 230, True, False, 12),
                      ("pair visits 202 x 150 QRCP", 202, 150, True, False, 12)],
}
CHILD_SECONDS = 120


def _rand_z(rng, n):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def run_setting(setting, lib):
    from hubbardtn_amd import abi
    if lib:
        abi._lib = abi.load_library(os.path.abspath(lib))      # the library HipOps takes
    from hubbardtn_amd.device import HipOps
    ops = HipOps(0)
    for k, (name, m, n, qrcp, acc, dec) in enumerate(SETTINGS[setting]):
        rng = np.random.default_rng(1000 + k)
        r = min(m, n)
        U, _ = np.linalg.qr(_rand_z(rng, m * r).reshape(m, r))
        W, _ = np.linalg.qr(_rand_z(rng, n * r).reshape(n, r))
        M = (U * 10.0 ** (-dec * np.arange(r) / (r - 1))) @ W.conj().T
        desc = np.zeros(1, dtype=abi.SVD_DT)
        if qrcp:
            desc[0] = (0, 0, 0, n, r, abi.SVD_QRCP, m)
            vo, so = ((n + 63) // 64 * 64) * r, r
        else:
            desc[0] = (0, 0, 0, m, n, abi.SVD_ACCUMULATE if acc else 0, 0)
            vo, so = (n * n if acc else 1), n
        dG = ops.to_device(M.T.reshape(-1))
        dV, dS, info = ops.zeros_z(vo), ops.empty_f64(so), ops.empty_i32(1)
        used = ops.jacobi_svd(dG, dV, dS, ops.to_device(desc), 1, max(m, n), 80, 1e-14, info, desc_host=desc)
        h = hashlib.sha256()
        for t in (dS, dG, dV, info):
            h.update(np.ascontiguousarray(ops.to_host(t)).tobytes())
        inf = ops.to_host(info).tolist()
        if min(inf) <= 0:
            raise SystemExit(f"{name}: not converged, info {inf}")
        print(f"{setting:<14s}| {name:<34s}| {h.hexdigest()[:32]} info {inf} outer sweeps {used}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=None, help="library file to fingerprint (default: this tree's)")
    ap.add_argument("--child", choices=tuple(SETTINGS), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return run_setting(a.child, a.lib)
    for setting in SETTINGS:
        env = {k: v for k, v in os.environ.items() if k != "HTN_SVD_PAIRS"}
        if setting != "default":
            env[setting] = "1"
        cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--child", setting]
        rc = subprocess.run(cmd + (["--lib", a.lib] if a.lib else []), env=env).returncode
        if rc != 0:
            raise SystemExit(f"svd_digest: the child for {setting} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
