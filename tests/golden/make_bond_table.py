"""Generates hubbardtn_amd/bond_table.py: the SU(2)-reduced operator strings of the bond-operator correlators
(engine.DMRG2.bond_correlator) that are not plain products of two closed term channels --
  ("bond", d), ("dimer", d) for d = 0, 1: B_i B_{i+d} and (S_i . S_{i+1}) (S_{i+d} . S_{i+d+1}) with a shared site (d = 1) or the
      same bond twice (d = 0): the operators of a shared site recoupled into ranks 0 / 1;
  ("spair", d) for d = 0, 1, 2: Delta+_i Delta_{i+d}, Delta_i = (c_{i up} c_{i+1 dn} - c_{i dn} c_{i+1 up}) / sqrt 2 (d = 2 stands for
      all disjoint pairs: four operators with the level (2, 0) between the bonds).
As tests/golden/make_string_table.py does for the interaction strings: candidate strings with unit coefficient are expanded to
dense matrices through the oracle's explicit Clebsch-Gordan tensors (oracle/mpo.mpo_to_dense) and the coefficients that
reproduce the dense second-quantised product (Jordan-Wigner matrices) are solved for; a residual above 1e-12 aborts.  Run once:
python tests/golden/make_bond_table.py.  The script also checks that the disjoint products of the Hermitian kinds are what
hubbardtn_amd/bondcorr.py builds from the term channels."""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_string_table as mst           # noqa: E402  (puts the repository root on sys.path)
from hubbardtn_amd import bondcorr, models          # noqa: E402

lm = mst.lm
# candidates per charge of a site: a basis of the site operators of that charge and rank
CAND = {0: (("id", 0), ("n", 0), ("docc", 0), ("S", 2)), +1: (("cdag", 1), ("cdagF", 1)), -1: (("c", 1), ("Fc", 1)),
        +2: (("pair_dag", 0),), -2: (("pair", 0),)}


def dense_bond_ops(L):
    """-> B(i), D(i) = S_i . S_{i+1}, Delta(i) as dense matrices of an L-site chain"""
    def site_op(mats):
        out = np.eye(1)
        for s in range(L):
            out = np.kron(out, mats.get(s, lm["id"]))
        return out

    def c_op(i, spin):
        mats = {s: lm["F"] for s in range(i)}
        mats[i] = lm["a_up"] if spin == 0 else lm["a_dn"]
        return site_op(mats)
    c = {(i, s): c_op(i, s) for i in range(L) for s in (0, 1)}
    B = lambda i: sum(c[(i, s)].T @ c[(i + 1, s)] + c[(i + 1, s)].T @ c[(i, s)] for s in (0, 1))
    sp = lambda i: c[(i, 0)].T @ c[(i, 1)]
    sz = lambda i: 0.5 * (c[(i, 0)].T @ c[(i, 0)] - c[(i, 1)].T @ c[(i, 1)])
    D = lambda i: sz(i) @ sz(i + 1) + 0.5 * (sp(i) @ sp(i + 1).T + sp(i).T @ sp(i + 1))
    Delta = lambda i: (c[(i, 0)] @ c[(i + 1, 1)] - c[(i, 1)] @ c[(i + 1, 0)]) / np.sqrt(2.0)
    return B, D, Delta


def fit(L, target, site_charges):
    """site_charges: the charges dN each site may carry.  Every combination of candidate operators whose charges add up to
    zero, with every admissible level spin, is a column; the columns are linearly independent (the candidates of a site are
    a basis), so the least-squares solution is the representation -> [(coef, [opnames], [labels])] without the zeros"""
    keep, cols = [], []
    for charges in itertools.product(*site_charges):
        if sum(charges) != 0:
            continue
        for combo in itertools.product(*[CAND[q] for q in charges]):
            names, ks = [n_ for n_, _ in combo], [k for _, k in combo]

            def rec(p, kprev, labels, dNacc):
                if p == L - 1:
                    if kprev == ks[p]:
                        yield list(labels)
                    return
                for k in range(abs(kprev - ks[p]), kprev + ks[p] + 1, 2):
                    if k <= 2:
                        yield from rec(p + 1, k, labels + [(dNacc + charges[p], k)], dNacc + charges[p])
            for labels in rec(0, 0, [], 0):
                m = mst.string_dense(L, list(enumerate(names)), labels)
                if np.abs(m).max() > 0:
                    keep.append((names, labels))
                    cols.append(m.ravel())
    A = np.stack(cols, axis=1)
    coef, *_ = np.linalg.lstsq(A, target.ravel(), rcond=None)
    res = np.abs(A @ coef - target.ravel()).max()
    assert res < 1e-12, ("no exact representation", res)
    return [(snap(coef[n_]), keep[n_][0], [tuple(x) for x in keep[n_][1]]) for n_ in range(len(keep)) if abs(coef[n_]) > 1e-12]


def snap(v):
    """exact form of a fitted coefficient (small rationals times sqrt of 1, 2, 3, 6)"""
    for b in (1.0, 2.0, 3.0, 6.0):
        for den in (1.0, 2.0, 4.0, 8.0, 16.0):
            for num in range(1, 25):
                for sgn in (1.0, -1.0):
                    c = sgn * num / den * np.sqrt(b)
                    if abs(v - c) < 1e-12:
                        return float(c)
    raise AssertionError(("coefficient without a closed form", v))


def main():
    table = {}
    odd, even = (+1, -1), (0, +2, -2)
    for d, L in ((0, 2), (1, 3), (2, 4)):
        B, D, Delta = dense_bond_ops(L)
        if d < 2:
            table[("bond", d)] = fit(L, B(0) @ B(d), [even, even] if d == 0 else [odd, even, odd])
            table[("dimer", d)] = fit(L, D(0) @ D(d), [(0,)] * L)
        else:                                   # the disjoint products of the Hermitian kinds: built from the term channels
            for kind, O in (("bond", B), ("dimer", D)):
                far = bondcorr._far_su2(models.SU2U1, kind)
                m = sum(cf * mst.string_dense(L, list(enumerate(names)), labels) for cf, names, labels in far)
                assert np.abs(m - O(0) @ O(2)).max() < 1e-12, kind
        table[("spair", d)] = fit(L, Delta(0).T @ Delta(d), [even, even] if d == 0 else [odd, even, odd] if d == 1 else [(+1,), (+1,), (-1,), (-1,)])
    out = os.path.join(mst.ROOT, "hubbardtn_amd", "bond_table.py")
    with open(out, "w") as f:
        f.write('"""GENERATED by tests/golden/make_bond_table.py -- do not edit.\n\n'
                'SU(2)-reduced operator strings of products of two nearest-neighbour bond operators (hubbardtn_amd/bondcorr.py):\n'
                '  ("bond", d): B_i B_{i+d}, B_i = sum_s (c+_{i s} c_{i+1 s} + h.c.);  ("dimer", d): (S_i . S_{i+1}) (S_{i+d} . S_{i+d+1})  (d = 0, 1);\n'
                '  ("spair", d): Delta+_i Delta_{i+d}, Delta_i = (c_{i up} c_{i+1 dn} - c_{i dn} c_{i+1 up}) / sqrt 2  (d = 0, 1; 2: any disjoint pair).\n'
                'Value: [(coefficient, [reduced site operator per site], [(dN, 2k) label of the level after each site but the last])].\n'
                'Coefficients are exact fits against the dense second-quantised operator (residual < 1e-12)."""\n\nTABLE = {\n')
        for key in sorted(table):
            f.write(f"    {key!r}: [\n")
            for row in table[key]:
                f.write(f"        {row!r},\n")
            f.write("    ],\n")
        f.write("}\n")
    print("wrote", out, {k: len(v) for k, v in table.items()})


if __name__ == "__main__":
    main()
