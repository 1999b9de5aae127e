// Planners of y = H_eff x: two sites (theta), one site, no site (the bond matrix).  Each walks its own terms -- the physics,
// with its own recoupling coefficient -- and hands every term to one emitter, which turns it into segments of the Y list and,
// where a term has both environments, of the Z staging list.  Host C++ (no HIP).
// NOT a translation unit of its own: #included by htn_plan.cpp (one unit, see its head); never name it on a build line.
#include "htn_tasks.h"

namespace htn {
namespace {

// The terms of an effective Hamiltonian, y[oi] += alpha * L x R for the block x (x_off, x_ld, x_n columns) of BUF_X.  A null
// Lb / Rb means "no environment on that side".  With both, the term is staged: Z = sum alpha L x over the terms that share the
// key zk (one output block, one right-hand block), then y[oi] += Z R once.
struct HeffTerms {
    TaskList ty, tz;
    int64_t zoff = 0, nterms = 0;
    void term(int oi, int64_t x_off, int x_ld, int x_n, const EnvLayout::Blk* Lb, const EnvLayout::Blk* Rb, const Key& zk, cplx alpha) {
        if (alpha == cplx(0.0, 0.0)) return;
        ++nterms;
        if (!Lb && !Rb) {
            ty.copy(oi, BUF_X, x_off, x_ld, alpha);
        } else if (!Rb) {
            ty.gemm(oi, BUF_L, Lb->off, Lb->m, HTN_OP_N, BUF_X, x_off, x_ld, HTN_OP_N, Lb->n, alpha);
        } else if (!Lb) {
            ty.gemm(oi, BUF_X, x_off, x_ld, HTN_OP_N, BUF_R, Rb->off, Rb->m, HTN_OP_N, Rb->m, alpha);
        } else {
            int zi = tz.find(zk);
            if (zi < 0) {
                zi = tz.block(zk, BUF_Z, zoff, Lb->m, x_n, Lb->m);
                ty.gemm(oi, BUF_Z, zoff, Lb->m, HTN_OP_N, BUF_R, Rb->off, Rb->m, HTN_OP_N, Rb->m, 1.0);
                zoff += (int64_t)Lb->m * x_n;
            }
            tz.gemm(zi, BUF_L, Lb->off, Lb->m, HTN_OP_N, BUF_X, x_off, x_ld, HTN_OP_N, Lb->n, alpha);
        }
    }
    void finish(ApplyPlan& out) {
        out.has_z = !tz.blocks.empty();
        if (out.has_z) tz.finalize(out.tz);
        ty.finalize(out.ty);
        out.zsize = zoff;
        out.nterms = nterms;
    }
};

}  // namespace

// ---- y = H_eff x ----------------------------------------------------------------------------------
void plan_apply(const Mpo& mpo, const ThetaLayout& tl, const EnvLayout& Ll, const EnvLayout& Rl, const MpoSite& W1,
                const MpoSite& W2, ApplyPlan& out) {
    const Sym& sym = mpo.sym;
    const int nfin = (int)W2.right.size() - 1;
    std::unordered_map<int, std::vector<const MpoEntry*>> w2;
    for (auto& e : W2.entries) w2[e.wl].push_back(&e);
    HeffTerms h;
    for (size_t i = 0; i < tl.blocks.size(); ++i) {
        const BlockRec& r = tl.blocks[i];
        h.ty.block(tl.bkeys[i], BUF_Y, r.off, r.m, r.n, r.ld);
    }
    std::vector<Sec> cps;
    for (size_t xi = 0; xi < tl.blocks.size(); ++xi) {
        const Key& beta = tl.bkeys[xi];
        const BlockRec& X = tl.blocks[xi];
        const Sec a{beta[0], beta[1]}, c{beta[3], beta[4]}, b{beta[6], beta[7]};
        const int s1 = beta[2], s2 = beta[5];
        const int js1 = sym.jeff(sym.site[s1].j), js2 = sym.jeff(sym.site[s2].j);
        for (auto& e1 : W1.entries) {
            const int w = e1.wl, wm = e1.wr;
            const SiteOp& o1 = mpo.ops[e1.op];
            const int kw = W1.left[w].k, kmid = W1.right[wm].k;
            std::vector<Sec> one_a{a};
            const std::vector<Sec>* aps = w == 0 ? &one_a : Ll.kets(w, a);
            if (!aps || aps->empty()) continue;
            for (int s1p = 0; s1p < sym.n_site; ++s1p) {
                const double r1 = o1.red[s1p][s1];
                if (r1 == 0.0) continue;
                auto iw = w2.find(wm);
                if (iw == w2.end()) continue;
                for (const MpoEntry* e2 : iw->second) {
                    const int wp = e2->wr;
                    const SiteOp& o2 = mpo.ops[e2->op];
                    const int kwp = W2.right[wp].k;
                    std::vector<Sec> one_b{b};
                    const std::vector<Sec>* bps = wp == nfin ? &one_b : Rl.kets(wp, b);
                    if (!bps || bps->empty()) continue;
                    for (int s2p = 0; s2p < sym.n_site; ++s2p) {
                        const double r2 = o2.red[s2p][s2];
                        if (r2 == 0.0) continue;
                        for (Sec ap : *aps) {
                            sym.fuse(ap, s1p, cps);
                            for (Sec cp : cps)
                                for (Sec bp : *bps) {
                                    const Key betap = tkey(ap, s1p, cp, s2p, bp);
                                    const int oi = h.ty.find(betap);
                                    if (oi < 0) continue;
                                    const double cf = coef_apply(sym.jeff(a.j), sym.jeff(ap.j), sym.jeff(kw), js1,
                                                                 sym.jeff(sym.site[s1p].j), sym.jeff(o1.k), sym.jeff(kmid),
                                                                 sym.jeff(c.j), sym.jeff(cp.j), js2, sym.jeff(sym.site[s2p].j),
                                                                 sym.jeff(o2.k), sym.jeff(kwp), sym.jeff(b.j), sym.jeff(bp.j));
                                    const cplx alpha = cf * r1 * r2 * e1.coef * e2->coef;
                                    h.term(oi, X.off, X.ld, X.n, w != 0 ? &Ll.blocks[Ll.block(ap, w, a)] : nullptr,
                                           wp != nfin ? &Rl.blocks[Rl.block(b, wp, bp)] : nullptr, mk(oi, wp, b.N, b.j), alpha);
                                }
                        }
                    }
                }
            }
        }
    }
    h.finish(out);
}

// ---- y = H_eff x for ONE site (one-site DMRG) ------------------------------------------------------------------------
// y[a',s',c'] += coef * L[a',w,a] x[a,s,c] R[c,w',c'] with coef = coef_left(site) * (2S_c' + 1) / (2S_c + 1): the left half is
// stage 1 of plan_left_env, the closing factor the one coef_apply carries for the right bond of theta.  Terms with both
// environments go through BUF_Z (Z = L x, summed over a, w and s for one (output block, w', c)), like plan_apply.
void plan_apply1(const Mpo& mpo, const SiteLayout& lay, const EnvLayout& Ll, const EnvLayout& Rl, const MpoSite& W, ApplyPlan& out) {
    const Sym& sym = mpo.sym;
    const int nfin = (int)W.right.size() - 1;
    HeffTerms h;
    for (size_t i = 0; i < lay.blocks.size(); ++i) {
        const BlockRec& r = lay.blocks[i];
        h.ty.block(lay.bkeys[i], BUF_Y, r.off, r.m, r.n, r.ld);
    }
    for (size_t xi = 0; xi < lay.blocks.size(); ++xi) {
        const Key& beta = lay.bkeys[xi];
        const BlockRec& X = lay.blocks[xi];
        const Sec a{beta[0], beta[1]}, c{beta[3], beta[4]};
        const int s = beta[2];
        for (auto& e : W.entries) {
            const int w = e.wl, wp = e.wr;
            const SiteOp& o = mpo.ops[e.op];
            const int kl = W.left[w].k, kr = W.right[wp].k;
            std::vector<Sec> one_a{a}, one_c{c};
            const std::vector<Sec>* aps = w == 0 ? &one_a : Ll.kets(w, a);
            const std::vector<Sec>* cps = wp == nfin ? &one_c : Rl.kets(wp, c);
            if (!aps || !cps) continue;
            for (int sp = 0; sp < sym.n_site; ++sp) {
                const double r = o.red[sp][s];
                if (r == 0.0) continue;
                for (Sec ap : *aps)
                    for (Sec cp : *cps) {
                        const int oi = h.ty.find(mk(ap.N, ap.j, sp, cp.N, cp.j));
                        if (oi < 0) continue;
                        const double cf = coef_left(sym.jeff(ap.j), sym.jeff(kl), sym.jeff(a.j), sym.jeff(sym.site[sp].j),
                                                    sym.jeff(sym.site[s].j), sym.jeff(o.k), sym.jeff(cp.j), sym.jeff(kr),
                                                    sym.jeff(c.j)) *
                                          (sym.jeff(cp.j) + 1) / (sym.jeff(c.j) + 1);
                        const cplx alpha = cf * r * e.coef;
                        h.term(oi, X.off, X.ld, X.n, w != 0 ? &Ll.blocks[Ll.block(ap, w, a)] : nullptr,
                               wp != nfin ? &Rl.blocks[Rl.block(c, wp, cp)] : nullptr, mk(oi, wp, c.N, c.j), alpha);
                    }
            }
        }
    }
    h.finish(out);
}

// ---- y = H_eff x for NO site (the bond matrix between two sites: the backward step of one-site TDVP) --------------------
// y[c'] += coef * L[c',w,c] x[c] R[c,w,c'] over the MPO levels w of the bond: plan_apply1 with the site's MPO tensor removed,
// i.e. a site of one multiplet (j = 0) under the identity (k = 0, reduced element 1), so that a = c, a' = c' and both levels
// are w: coef = coef_left(j = 0 site) * (2S_c' + 1) / (2S_c + 1).  x and y are in BOND layout: one n_c x n_c matrix per sector
// of the bond, in the bond's sector order, leading dimension n_c -- what plan_gauge1 lays out for the triangular factors.
// Level 0 has no left environment, the last level no right one; every other level goes through BUF_Z (Z = L x), like plan_apply1.
void plan_apply0(const Mpo& mpo, const Bond& bond, const EnvLayout& Ll, const EnvLayout& Rl, ApplyPlan& out) {
    const Sym& sym = mpo.sym;
    const std::vector<Lvl>& levels = Ll.levels;
    const int nfin = (int)levels.size() - 1;
    HeffTerms h;
    std::vector<int64_t> offs(bond.secs.size());
    int64_t size = 0;
    for (size_t ci = 0; ci < bond.secs.size(); ++ci) {
        const Sec c = bond.secs[ci];
        const int n = bond.dims[ci];
        offs[ci] = size;
        h.ty.block(mk(c.N, c.j), BUF_Y, size, n, n, n);
        size += (int64_t)n * n;
    }
    for (size_t ci = 0; ci < bond.secs.size(); ++ci) {
        const Sec c = bond.secs[ci];
        const int nc = bond.dims[ci];
        for (int w = 0; w <= nfin; ++w) {
            const bool hasL = w != 0, hasR = w != nfin;
            std::vector<Sec> one_c{c};
            const std::vector<Sec>* cps = hasL ? Ll.kets(w, c) : (hasR ? Rl.kets(w, c) : &one_c);
            if (!cps) continue;
            const int kw = sym.jeff(levels[w].k);
            for (Sec cp : *cps) {
                const int oi = h.ty.find(mk(cp.N, cp.j));
                if (oi < 0) continue;
                const int lb = hasL ? Ll.block(cp, w, c) : 0, rb = hasR ? Rl.block(c, w, cp) : 0;
                if (lb < 0 || rb < 0) continue;
                const int jc = sym.jeff(c.j), jcp = sym.jeff(cp.j);
                const double cf = coef_left(jcp, kw, jc, 0, 0, 0, jcp, kw, jc) * (jcp + 1) / (jc + 1);
                h.term(oi, offs[ci], nc, nc, hasL ? &Ll.blocks[lb] : nullptr, hasR ? &Rl.blocks[rb] : nullptr, mk(oi, w, c.N, c.j), cf);
            }
        }
    }
    h.finish(out);
}

}  // namespace htn
