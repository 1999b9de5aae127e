"""Host tables of the bond-operator correlators (engine.DMRG2.bond_correlator): the operator strings whose expectation values
add up to <O+_i O_j> for two nearest-neighbour bond operators.

A string is (coefficient, [site operator per site], [(dN, k) label of the MPO level after each operator but the last]): what
models._build_mpo takes as `strings` in the SU(2) modes.  Three lists per kind:
  [0]  j = i      the product on the two sites i, i+1            (measured by htn_mps_correlator at distance 1)
  [1]  j = i + 1  the product on the three sites i, i+1, i+2     (htn_mps_correlator2 with a one-site close)
  [2]  j >= i + 2 disjoint bonds: operators on i, i+1, j, j+1    (htn_mps_correlator2)
The bond operators themselves are the symmetry's term channels (models.TERM_CHANNELS*): B_i is the "hop" term with
coefficient +1, S_i . S_{i+1} the "ss" term; the pair field has no term channel and is written out here.
  SU(2) modes: disjoint Hermitian bonds are products of two closed channels (the level between them is the scalar); products
      that share a site need the shared site's operators recoupled into ranks 0 / 1, and the pair field its Clebsch-Gordan
      factor: generated coefficients (bond_table.py, fitted against dense operators by tests/golden/make_bond_table.py).
  U(1) x U(1) mode: every factor is a plain matrix (all Clebsch-Gordan factors 1), products are taken site by site here."""
from math import sqrt

import numpy as np

from .models import _A_DN, _A_UP, _charge_u1, _jw_string

SU2_KINDS = ("bond", "dimer", "spair")
U1_KINDS = SU2_KINDS + ("bond_up", "bond_dn", "dimer_zz", "dimer_xy")


def _channels(sym, kind):
    """the term channels that make up the Hermitian bond operator of `kind`: [(factor, op_open, op_close, (dN, k))]"""
    if kind.startswith("bond"):
        pick = (lambda name: True) if kind == "bond" else (lambda name: name.startswith("hop" + kind[4:]))
        return [(f, o, c, q) for (name, q, o, _p, c, f) in sym.channels["hop"] if pick(name)]
    pick = {"dimer": lambda name: True, "dimer_zz": lambda name: name == "szsz", "dimer_xy": lambda name: name != "szsz"}[kind]
    return [(f, o, c, q) for (name, q, o, _p, c, f) in sym.channels["ss"] if pick(name)]


def _check_kind(sym, kind):
    if kind not in (SU2_KINDS if sym.su2 else U1_KINDS) or (kind == "spair" and sym.kind == 2):
        raise ValueError(f"bond correlator kind '{kind}' is not available in the {sym.name} mode")


# ---- U(1) x U(1): products of Jordan-Wigner matrices --------------------------------------------------------------------
def _bond_u1(sym, kind):
    """(O+, O) on the sites (0, 1) as [(factor, matrix on site 0, matrix on site 1)]"""
    if kind == "spair":
        pairs = ((1.0 / sqrt(2.0), _A_UP, _A_DN), (-1.0 / sqrt(2.0), _A_DN, _A_UP))       # (c_up c'_dn - c_dn c'_up) / sqrt 2
        O = []
        for f, a, b in pairs:
            m = _jw_string([(0, a, True), (1, b, True)])
            O.append((f, m[0], m[1]))
    else:
        O = [(f, sym.site_ops[o][2], sym.site_ops[c][2]) for (f, o, c, _q) in _channels(sym, kind)]
    return [(f, x.T.copy(), y.T.copy()) for f, x, y in O], O


def _string_u1(coef, mats):
    """a product of local matrices on adjacent sites -> a string with the accumulated charges as level labels; None if zero"""
    ops, labels, acc = [], [], (0, 0)
    for m in mats:
        q = _charge_u1(m)
        if q is None:
            return None
        acc = (acc[0] + q[0], acc[1] + q[1])
        ops.append((q[1], q[0], m))
        labels.append(acc)
    assert acc == (0, 0)
    return (coef, ops, labels[:-1])


def _strings_u1(sym, kind):
    left, right = _bond_u1(sym, kind)
    tabs = ([], [], [])
    for fl, xl, yl in left:
        for fr, xr, yr in right:
            for d, mats in enumerate(((xl @ xr, yl @ yr), (xl, yl @ xr, yr), (xl, yl, xr, yr))):
                s = _string_u1(fl * fr, mats)
                if s is not None:
                    tabs[d].append(s)
    return tabs


# ---- SU(2) modes --------------------------------------------------------------------------------------------------------
def _far_su2(sym, kind):
    """disjoint bonds of a Hermitian kind: every closed channel of the first bond times every one of the second"""
    ch = _channels(sym, kind)
    return [(fa * fb, [oa, ca, ob, cb], [qa, (0, 0), qb]) for (fa, oa, ca, qa) in ch for (fb, ob, cb, qb) in ch]


def _strings_su2(sym, kind):
    from .bond_table import TABLE
    return TABLE[(kind, 0)], TABLE[(kind, 1)], TABLE[(kind, 2)] if kind == "spair" else _far_su2(sym, kind)


def _merged(sym, strings, pos):
    """strings that differ in the operator at `pos` alone (same charge and rank there, same levels) are one string with the
    sum of those operators at `pos`: one device pass instead of several"""
    op = lambda o: tuple(sym.site_ops[o]) if isinstance(o, str) else o
    groups = {}
    for coef, ops, labels in strings:
        ops = [op(o) for o in ops]
        key = (tuple((k, dN, np.asarray(m, dtype=float).tobytes()) for n, (k, dN, m) in enumerate(ops) if n != pos),
               tuple(map(tuple, labels)), ops[pos][0], ops[pos][1])
        g = groups.setdefault(key, [ops, labels, np.zeros_like(np.asarray(ops[pos][2], dtype=float))])
        g[2] = g[2] + coef * np.asarray(ops[pos][2], dtype=float)
    return [(1.0, ops[:pos] + [(ops[pos][0], ops[pos][1], m)] + ops[pos + 1:], labels) for ops, labels, m in groups.values()]


def strings(sym, kind):
    """-> (strings of j = i, of j = i + 1, of j >= i + 2) of <O+_i O_j>; ValueError for a kind the mode does not define"""
    _check_kind(sym, kind)
    same, shared, far = _strings_su2(sym, kind) if sym.su2 else _strings_u1(sym, kind)
    return _merged(sym, same, 1), _merged(sym, shared, 1), far


def one_bond(sym, kind):
    """the two-site strings of the Hermitian bond operator O_i itself"""
    _check_kind(sym, kind)
    if kind == "spair":
        raise ValueError("the pair field changes the particle number: it has no expectation value")
    if sym.su2:
        return [(f, [o, c], [q]) for (f, o, c, q) in _channels(sym, kind)]
    return [s for s in (_string_u1(f, (x, y)) for f, x, y in _bond_u1(sym, kind)[1]) if s is not None]
