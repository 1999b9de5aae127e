// Planners of everything around the H_eff apply in a sweep: the gauge move of a one-site update, theta = T1 . T2 and the
// two H environment steps.  Host C++ (no HIP).
// NOT a translation unit of its own: #included by htn_plan.cpp (one unit, see its head); never name it on a build line.
#include "htn_tasks.h"

namespace htn {

// ---- gauge move of a one-site update -----------------------------------------------------------------------------------
// QR (centre in left layout, move right) or LQ (right layout, move left) descriptors of the centre's sector matrices, and
// the task list that takes the triangular factors (BUF_S1, one n_c x n_c matrix per sector, ld n_c) into the neighbour
// (BUF_S2 -> BUF_Y, same layout): B_c <- R_c B_c per left sector c of a right-layout neighbour, A_c <- A_c L_c per right
// sector of a left-layout one.  A sector the centre does not reach has no segment: its block is written as zeros.
void plan_gauge1(const SiteLayout& cen, const SiteLayout& nb, std::vector<htn_qr_block>& desc, int64_t& rsize, Tasks& out) {
    const bool right = cen.kind == 'L';
    desc.clear();
    rsize = 0;
    std::unordered_map<uint64_t, std::pair<int64_t, int>> rof;
    for (const auto& M : cen.mats) {
        htn_qr_block d;
        memset(&d, 0, sizeof(d));
        d.offset = M.off;
        d.ld = M.rows;
        d.trans = right ? 0 : 1;
        d.m = right ? M.rows : M.cols;
        d.n = right ? M.cols : M.rows;
        d.r_offset = rsize;
        d.ldr = d.n;
        rof[skey(M.c)] = {rsize, d.n};
        rsize += (int64_t)d.n * d.n;
        desc.push_back(d);
    }
    TaskList t;
    for (const auto& M : nb.mats) {
        const int bi = t.block(mk(M.c.N, M.c.j), BUF_Y, M.off, M.rows, M.cols, M.rows);
        auto it = rof.find(skey(M.c));
        if (it == rof.end()) continue;
        const int nc = it->second.second;
        if (right) t.gemm(bi, BUF_S1, it->second.first, nc, HTN_OP_N, BUF_S2, M.off, M.rows, HTN_OP_N, nc, 1.0);
        else t.gemm(bi, BUF_S2, M.off, M.rows, HTN_OP_N, BUF_S1, it->second.first, nc, HTN_OP_N, nc, 1.0);
    }
    t.finalize(out);
}

// ---- theta = T1 . T2 ------------------------------------------------------------------------------------------------
// mode "RR": both right layout (centre on i); "LL": both left layout (centre on i+1); "LR": left x right layout.
// buffers: BUF_S1 = site i, BUF_S2 = site i+1, output BUF_Y.
void plan_theta(const char* mode, const SiteLayout& lay1, const SiteLayout& lay2, const ThetaLayout& tl, Tasks& out) {
    TaskList t;
    const bool LR = !strcmp(mode, "LR"), RR = !strcmp(mode, "RR");
    for (auto& M : tl.mats) {
        const Sec c = M.c;
        if (LR) {
            const int bi = t.block(mk(0, c.N, c.j), BUF_Y, M.off, M.rows, M.cols, M.rows);
            const int m1 = lay1.mat(c), m2 = lay2.mat(c);
            if (m1 >= 0 && m2 >= 0) {
                const auto& A = lay1.mats[m1];
                const auto& Bm = lay2.mats[m2];
                t.gemm(bi, BUF_S1, A.off, A.rows, HTN_OP_N, BUF_S2, Bm.off, Bm.rows, HTN_OP_N, A.cols, 1.0);
            }
        } else if (RR) {
            const int m2 = lay2.mat(c);
            for (size_t i = 0; i < M.rows_g.size(); ++i) {
                const Sec a = M.rows_g[i].sec;
                const int s1 = M.rows_g[i].s;
                const int bi = t.block(mk(1, a.N, a.j, s1, c.N, c.j), BUF_Y, M.off + M.roffs[i], tl.bl->dim(a), M.cols, M.rows);
                const int blk = lay1.block(a, s1, c);
                if (blk >= 0 && m2 >= 0) {
                    const BlockRec& r = lay1.blocks[blk];
                    const auto& Bm = lay2.mats[m2];
                    t.gemm(bi, BUF_S1, r.off, r.ld, HTN_OP_N, BUF_S2, Bm.off, Bm.rows, HTN_OP_N, r.n, 1.0);
                }
            }
        } else {
            const int m1 = lay1.mat(c);
            for (size_t j = 0; j < M.cols_g.size(); ++j) {
                const Sec b = M.cols_g[j].sec;
                const int s2 = M.cols_g[j].s;
                const int bi = t.block(mk(2, c.N, c.j, s2, b.N, b.j), BUF_Y, M.off + (int64_t)M.coffs[j] * M.rows, M.rows,
                                       tl.br->dim(b), M.rows);
                const int blk = lay2.block(c, s2, b);
                if (blk >= 0 && m1 >= 0) {
                    const BlockRec& r = lay2.blocks[blk];
                    const auto& A = lay1.mats[m1];
                    t.gemm(bi, BUF_S1, A.off, A.rows, HTN_OP_N, BUF_S2, r.off, r.ld, HTN_OP_N, r.m, 1.0);
                }
            }
        }
    }
    t.finalize(out);
}

// ---- environments (a10) -------------------------------------------------------------------------------------------
// GL[i+1] from GL[i], left-layout site tensor (BUF_S1), MPO site W.  stage 1 -> BUF_Z (Y panels), stage 2 -> BUF_Y.
void plan_left_env(const Mpo& mpo, const EnvLayout& Ll, const SiteLayout& lay, const MpoSite& W, const EnvLayout& Lnew,
                   EnvPlan& out) {
    const Sym& sym = mpo.sym;
    TaskList t1, t2;
    int64_t zoff = 0;
    KeyMap ypanel;
    for (size_t q = 0; q < Lnew.blocks.size(); ++q) {
        const Key& k = Lnew.bkeys[q];
        const Sec cp{k[0], k[1]}, c{k[3], k[4]};
        const int wp = k[2];
        const auto& nb = Lnew.blocks[q];
        const int b2 = t2.block(k, BUF_Y, nb.off, nb.m, nb.n, nb.m);
        const int mcp = lay.mat(cp), mc = lay.mat(c);
        if (mcp < 0 || mc < 0) continue;                       // structurally zero block
        const auto& Mcp = lay.mats[mcp];
        ypanel[k] = 1;
        t2.gemm(b2, BUF_S1, Mcp.off, Mcp.rows, HTN_OP_C, BUF_Z, zoff, Mcp.rows, HTN_OP_N, Mcp.rows, 1.0);
        int ro = 0;
        for (auto& g : Mcp.groups) {
            t1.block(mk(cp.N, cp.j, wp, c.N, c.j, g.sec.N, g.sec.j, g.s), BUF_Z, zoff + ro, lay.bl->dim(g.sec), nb.n, Mcp.rows);
            ro += lay.bl->dim(g.sec);
        }
        zoff += (int64_t)Mcp.rows * nb.n;
    }
    std::vector<Sec> cps;
    for (auto& e : W.entries) {
        const int wl = e.wl, wr = e.wr;
        if (wr == 0 && W.right.size() > 1) continue;           // 'start' level stays the implicit identity
        const SiteOp& o = mpo.ops[e.op];
        const int kl = W.left[wl].k, kr = W.right[wr].k;
        for (size_t bi = 0; bi < lay.blocks.size(); ++bi) {
            const Key& bk = lay.bkeys[bi];
            const Sec a{bk[0], bk[1]}, c{bk[3], bk[4]};
            const int s = bk[2];
            const BlockRec& Ab = lay.blocks[bi];
            for (int sp = 0; sp < sym.n_site; ++sp) {
                const double r = o.red[sp][s];
                if (r == 0.0) continue;
                std::vector<Sec> one{a};
                const std::vector<Sec>* aps = wl == 0 ? &one : Ll.kets(wl, a);
                if (!aps) continue;
                for (Sec ap : *aps) {
                    sym.fuse(ap, sp, cps);
                    for (Sec cp : cps) {
                        if (!ypanel.count(mk(cp.N, cp.j, wr, c.N, c.j)) || lay.block(ap, sp, cp) < 0) continue;
                        const double cf = coef_left(sym.jeff(ap.j), sym.jeff(kl), sym.jeff(a.j), sym.jeff(sym.site[sp].j),
                                                    sym.jeff(sym.site[s].j), sym.jeff(o.k), sym.jeff(cp.j), sym.jeff(kr),
                                                    sym.jeff(c.j));
                        const cplx alpha = cf * r * e.coef;
                        if (alpha == cplx(0.0, 0.0)) continue;
                        const int b1 = t1.find(mk(cp.N, cp.j, wr, c.N, c.j, ap.N, ap.j, sp));
                        if (wl == 0)
                            t1.copy(b1, BUF_S1, Ab.off, Ab.ld, alpha);
                        else {
                            const auto& Lb = Ll.blocks[Ll.block(ap, wl, a)];
                            t1.gemm(b1, BUF_L, Lb.off, Lb.m, HTN_OP_N, BUF_S1, Ab.off, Ab.ld, HTN_OP_N, Lb.n, alpha);
                        }
                    }
                }
            }
        }
    }
    t1.finalize(out.t1);
    t2.finalize(out.t2);
    out.zsize = zoff;
}

// GR[i] (stored transposed: block (c, w, c') = [n_c, n_c']) from GR[i+1], right-layout site tensor (BUF_S1), MPO site W
void plan_right_env(const Mpo& mpo, const EnvLayout& Rl, const SiteLayout& lay, const MpoSite& W, const EnvLayout& Rnew,
                    EnvPlan& out) {
    const Sym& sym = mpo.sym;
    TaskList t1, t2;
    const int nfin_r = (int)W.right.size() - 1, nfin_l = (int)W.left.size() - 1;
    int64_t zoff = 0;
    KeyMap ypanel;
    for (size_t q = 0; q < Rnew.blocks.size(); ++q) {
        const Key& k = Rnew.bkeys[q];
        const Sec c{k[0], k[1]}, cp{k[3], k[4]};
        const int w = k[2];
        const auto& nb = Rnew.blocks[q];
        const int b2 = t2.block(k, BUF_Y, nb.off, nb.m, nb.n, nb.m);
        const int mcp = lay.mat(cp), mc = lay.mat(c);
        if (mcp < 0 || mc < 0) continue;
        const auto& Mcp = lay.mats[mcp];
        ypanel[k] = 1;
        // Rt[c, w, c'] (n_c x n_c') = Y (n_c x cols') . B_{c'}^H (cols' x n_c')
        t2.gemm(b2, BUF_Z, zoff, nb.m, HTN_OP_N, BUF_S1, Mcp.off, Mcp.rows, HTN_OP_C, Mcp.cols, 1.0);
        int co = 0;
        for (auto& g : Mcp.groups) {
            t1.block(mk(c.N, c.j, w, cp.N, cp.j, g.s, g.sec.N, g.sec.j), BUF_Z, zoff + (int64_t)co * nb.m, nb.m, lay.br->dim(g.sec), nb.m);
            co += lay.br->dim(g.sec);
        }
        zoff += (int64_t)nb.m * Mcp.cols;
    }
    std::vector<Sec> cps;
    for (auto& e : W.entries) {
        const int wl = e.wl, wr = e.wr;
        if (wl == nfin_l && W.left.size() > 1) continue;       // 'final' level stays the implicit identity
        const SiteOp& o = mpo.ops[e.op];
        const int kl = W.left[wl].k, kr = W.right[wr].k;
        for (size_t bi = 0; bi < lay.blocks.size(); ++bi) {
            const Key& bk = lay.bkeys[bi];
            const Sec c{bk[0], bk[1]}, b{bk[3], bk[4]};
            const int s = bk[2];
            const BlockRec& Bb = lay.blocks[bi];
            for (int sp = 0; sp < sym.n_site; ++sp) {
                const double r = o.red[sp][s];
                if (r == 0.0) continue;
                std::vector<Sec> one{b};
                const std::vector<Sec>* bps = wr == nfin_r ? &one : Rl.kets(wr, b);
                if (!bps) continue;
                for (Sec bp : *bps) {
                    sym.split(bp, sp, cps);
                    for (Sec cp : cps) {
                        if (!ypanel.count(mk(c.N, c.j, wl, cp.N, cp.j)) || lay.block(cp, sp, bp) < 0) continue;
                        const double cf = coef_right(sym.jeff(cp.j), sym.jeff(kl), sym.jeff(c.j), sym.jeff(sym.site[sp].j),
                                                     sym.jeff(sym.site[s].j), sym.jeff(o.k), sym.jeff(bp.j), sym.jeff(kr),
                                                     sym.jeff(b.j));
                        const cplx alpha = cf * r * e.coef;
                        if (alpha == cplx(0.0, 0.0)) continue;
                        const int b1 = t1.find(mk(c.N, c.j, wl, cp.N, cp.j, sp, bp.N, bp.j));
                        if (wr == nfin_r)
                            t1.copy(b1, BUF_S1, Bb.off, Bb.ld, alpha);
                        else {
                            const auto& Rb = Rl.blocks[Rl.block(b, wr, bp)];
                            t1.gemm(b1, BUF_S1, Bb.off, Bb.ld, HTN_OP_N, BUF_R, Rb.off, Rb.m, HTN_OP_N, Rb.m, alpha);
                        }
                    }
                }
            }
        }
    }
    t1.finalize(out.t1);
    t2.finalize(out.t2);
    out.zsize = zoff;
}

}  // namespace htn
