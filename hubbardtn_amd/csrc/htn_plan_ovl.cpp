// Planners of the overlap environments and of the projector vector of orthogonalised DMRG (htn_core.h: OvlLayout).  Host
// C++ (no HIP).
// NOT a translation unit of its own: #included by htn_plan.cpp (one unit, see its head); never name it on a build line.
#include "htn_tasks.h"

namespace htn {

// O_new^c [bra x ket] = sum_{a, s} B[a, s, c]^H (O^a K[a, s, c]).  stage 1: Z = O^a K -> BUF_Z; stage 2: B^H Z -> BUF_Y
void plan_ovl_left(const OvlLayout& Ol, const SiteLayout& bra, const SiteLayout& ket, const OvlLayout& Onew, OvlPlan& out) {
    TaskList t1, t2;
    int64_t zoff = 0;
    for (size_t q = 0; q < Onew.secs.size(); ++q) {
        const Sec c = Onew.secs[q];
        t2.block(mk(c.N, c.j), BUF_Y, Onew.off[q], Onew.m[q], Onew.n[q], Onew.m[q]);
    }
    for (size_t bi = 0; bi < ket.blocks.size(); ++bi) {
        const Key& bk = ket.bkeys[bi];
        const Sec a{bk[0], bk[1]}, c{bk[3], bk[4]};
        const int s = bk[2];
        const int ia = Ol.find(a), ic = Onew.find(c), bb = bra.block(a, s, c);
        if (ia < 0 || ic < 0 || bb < 0) continue;
        const BlockRec &Kb = ket.blocks[bi], &Bb = bra.blocks[bb];
        const int b1 = t1.block(mk(a.N, a.j, s, c.N, c.j), BUF_Z, zoff, Ol.m[ia], Kb.n, Ol.m[ia]);
        t1.gemm(b1, BUF_L, Ol.off[ia], Ol.m[ia], HTN_OP_N, BUF_S2, Kb.off, Kb.ld, HTN_OP_N, Ol.n[ia], 1.0);
        t2.gemm(t2.find(mk(c.N, c.j)), BUF_S1, Bb.off, Bb.ld, HTN_OP_C, BUF_Z, zoff, Ol.m[ia], HTN_OP_N, Ol.m[ia], 1.0);
        zoff += (int64_t)Ol.m[ia] * Kb.n;
    }
    t1.finalize(out.t1);
    t2.finalize(out.t2);
    out.zsize = zoff;
}

// O_new^a [ket x bra] = sum_{s, b} (K[a, s, b] O^b) B[a, s, b]^H
void plan_ovl_right(const OvlLayout& Or, const SiteLayout& bra, const SiteLayout& ket, const OvlLayout& Onew, OvlPlan& out) {
    TaskList t1, t2;
    int64_t zoff = 0;
    for (size_t q = 0; q < Onew.secs.size(); ++q) {
        const Sec a = Onew.secs[q];
        t2.block(mk(a.N, a.j), BUF_Y, Onew.off[q], Onew.m[q], Onew.n[q], Onew.m[q]);
    }
    for (size_t bi = 0; bi < ket.blocks.size(); ++bi) {
        const Key& bk = ket.bkeys[bi];
        const Sec a{bk[0], bk[1]}, b{bk[3], bk[4]};
        const int s = bk[2];
        const int ib = Or.find(b), ia = Onew.find(a), bb = bra.block(a, s, b);
        if (ib < 0 || ia < 0 || bb < 0) continue;
        const BlockRec &Kb = ket.blocks[bi], &Bb = bra.blocks[bb];
        const int b1 = t1.block(mk(a.N, a.j, s, b.N, b.j), BUF_Z, zoff, Kb.m, Or.n[ib], Kb.m);
        t1.gemm(b1, BUF_S2, Kb.off, Kb.ld, HTN_OP_N, BUF_R, Or.off[ib], Or.m[ib], HTN_OP_N, Or.m[ib], 1.0);
        t2.gemm(t2.find(mk(a.N, a.j)), BUF_Z, zoff, Kb.m, HTN_OP_N, BUF_S1, Bb.off, Bb.ld, HTN_OP_C, Or.n[ib], 1.0);
        zoff += (int64_t)Kb.m * Or.n[ib];
    }
    t1.finalize(out.t1);
    t2.finalize(out.t2);
    out.zsize = zoff;
}

// p[a, s1, c, s2, b] = (O_L^a K1[a, s1, c]) (K2[c, s2, b] O_R^b): stage 1 forms both brackets in BUF_Z, stage 2 multiplies them
// into every block of the bra's theta layout (a block without a partner in the ket is written as zeros)
void plan_ovl_project(const OvlLayout& Ol, const OvlLayout& Or, const SiteLayout& k1, const SiteLayout& k2, const ThetaLayout& tl,
                      OvlPlan& out) {
    TaskList t1, t2;
    int64_t zoff = 0;
    std::unordered_map<Key, int64_t, KeyHash> zl, zr;
    for (size_t bi = 0; bi < k1.blocks.size(); ++bi) {
        const Key& bk = k1.bkeys[bi];
        const Sec a{bk[0], bk[1]};
        const int ia = Ol.find(a);
        if (ia < 0) continue;
        const BlockRec& Kb = k1.blocks[bi];
        const int b1 = t1.block(mk(0, bk[0], bk[1], bk[2], bk[3], bk[4]), BUF_Z, zoff, Ol.m[ia], Kb.n, Ol.m[ia]);
        t1.gemm(b1, BUF_L, Ol.off[ia], Ol.m[ia], HTN_OP_N, BUF_S1, Kb.off, Kb.ld, HTN_OP_N, Ol.n[ia], 1.0);
        zl[bk] = zoff;
        zoff += (int64_t)Ol.m[ia] * Kb.n;
    }
    for (size_t bi = 0; bi < k2.blocks.size(); ++bi) {
        const Key& bk = k2.bkeys[bi];
        const Sec b{bk[3], bk[4]};
        const int ib = Or.find(b);
        if (ib < 0) continue;
        const BlockRec& Kb = k2.blocks[bi];
        const int b1 = t1.block(mk(1, bk[0], bk[1], bk[2], bk[3], bk[4]), BUF_Z, zoff, Kb.m, Or.n[ib], Kb.m);
        t1.gemm(b1, BUF_S2, Kb.off, Kb.ld, HTN_OP_N, BUF_R, Or.off[ib], Or.m[ib], HTN_OP_N, Or.m[ib], 1.0);
        zr[bk] = zoff;
        zoff += (int64_t)Kb.m * Or.n[ib];
    }
    for (auto& M : tl.mats) {
        const Sec c = M.c;
        const int kc = k1.br->dim(c);
        for (size_t i = 0; i < M.rows_g.size(); ++i)
            for (size_t j = 0; j < M.cols_g.size(); ++j) {
                const Sec a = M.rows_g[i].sec, b = M.cols_g[j].sec;
                const int s1 = M.rows_g[i].s, s2 = M.cols_g[j].s;
                const int na = tl.bl->dim(a), nb = tl.br->dim(b);
                const int b2 = t2.block(tkey(a, s1, c, s2, b), BUF_Y, M.off + M.roffs[i] + (int64_t)M.coffs[j] * M.rows, na, nb, M.rows);
                auto l = zl.find(mk(a.N, a.j, s1, c.N, c.j));
                auto r = zr.find(mk(c.N, c.j, s2, b.N, b.j));
                if (kc <= 0 || l == zl.end() || r == zr.end()) continue;
                t2.gemm(b2, BUF_Z, l->second, na, HTN_OP_N, BUF_Z, r->second, kc, HTN_OP_N, kc, 1.0);
            }
    }
    t1.finalize(out.t1);
    t2.finalize(out.t2);
    out.zsize = zoff;
}

}  // namespace htn
