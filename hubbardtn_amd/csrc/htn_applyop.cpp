// A local operator applied to a finite MPS (htn_mps_apply_op) and the transition amplitudes <O_x bra|ket> of all sites
// (htn_mps_transition); DESIGN.md section 4c.  Host C++ (no HIP): the planner below writes bond tables, layouts and place-item
// lists; the device work is Backend::block_place, the overlap transfers of htn_overlap.cpp's planners and block_trdots.
// NOT a translation unit of its own: #included by htn_engine.cpp (one unit, see its head); never name it on a build line.
//
// The operator O (rank k, charge dN) acts on site x and its charge leaves through the RIGHT end: every bond b > x is
// re-labelled by fusion with (dN, k).  An old sector r contributes its multiplets to each new sector r' in r (x) (dN, k); the
// multiplets of r' are the concatenation of its contributions in the sorted order of r.  In bare (left-coupled) reduced
// tensors, with all couplings in the order (first (x) second -> result) that coef_left assumes,
//   opened  X[l, s, r'(r)]     = (-1)^(N_l dN) <s||O||s'> A[l, s', r] . (-1)^(l+s'+k+r') sqrt((2r+1)(2s+1)) {l s' r; k r' s}
//   passed  T'[l'(l), s, r'(r)] = T[l, s, r] . (-1)^(k+s+l'+r) sqrt((2l'+1)(2r+1)) {k l l'; s r' r}
// (recoupling ((l s')r, k)r' -> (l, (s' k)s)r' and ((l s)r, k)r' -> ((l k)l', s)r'; the Jordan-Wigner string of the library's
// fermion operators runs to the LEFT of the site, so an odd operator meets no sign on the sites it passes), and the stored
// blocks carry the tilde factors of DESIGN section 2 on top: sqrt((2r'+1)/(2r+1)) for X, sqrt((2r'+1)(2l+1)/((2l'+1)(2r+1)))
// for T'.  Those telescope along every path of sectors, so the same items serve a source in any gauge.  Abelian kind: all
// spins enter as 0, every factor is 1 and only the string sign is left.
#include <set>

#include "htn_engine.h"

namespace {

struct FPart {
    Sec r;
    int32_t off, dim;
};
struct Fused {                     // a bond of the applied state and where the multiplets of every old sector went
    BondP src, bond;
    std::unordered_map<uint64_t, std::vector<FPart>> parts;      // r' -> its contributions, sorted by r
    std::string sig;               // names (source table, kept pairs) in plan caches
    const std::vector<FPart>* of(Sec rp) const {
        auto it = parts.find(skey(rp));
        return it == parts.end() ? nullptr : &it->second;
    }
};
typedef std::shared_ptr<const Fused> FusedP;
typedef std::set<std::pair<Sec, Sec>> PairSet;      // (r', r)

struct PlaceC {                    // one site tensor of the applied state: its layout and the items that build it
    SiteLayoutP lay;
    std::vector<htn_place_item> items;
    DBufP items_dev;
};
struct OpInfo {
    SiteOp op;
    std::string tag;               // the operator's name in the plan cache: its table
};

void targets(const Sym& sym, Sec r, const SiteOp& op, std::vector<Sec>& out) {
    out.clear();
    const int N = sym.wrapN(r.N + op.dN);
    if (!sym.su2()) {
        out.push_back({N, r.j + op.k});
        return;
    }
    for (int jj = abs(r.j - op.k); jj <= r.j + op.k; jj += 2) out.push_back({N, jj});
}
// can b sites hold the sector at all
bool physical(const Sym& sym, Sec c, int b) {
    if (sym.kind == HTN_SYM_SU2) return c.j >= 0 && c.j <= b;
    return c.N >= 0 && c.N <= 2 * b && abs(c.j) <= std::min(c.N, 2 * b - c.N);
}

FusedP identity_fused(BondP src) {
    auto f = std::make_shared<Fused>();
    f->src = f->bond = src;
    for (size_t q = 0; q < src->secs.size(); ++q) f->parts[skey(src->secs[q])] = {{src->secs[q], 0, src->dims[q]}};
    f->sig = "I" + src->key;
    return f;
}
// keep == nullptr: every sector b sites can hold
FusedP fuse_bond(const Sym& sym, BondP src, const SiteOp& op, int b, const PairSet* keep) {
    auto f = std::make_shared<Fused>();
    f->src = src;
    std::map<Sec, std::vector<FPart>> acc;
    std::vector<Sec> tg;
    for (size_t q = 0; q < src->secs.size(); ++q) {         // (sorted: the contributions of r' arrive in the order of r)
        targets(sym, src->secs[q], op, tg);
        for (Sec rp : tg) {
            if (keep ? !keep->count({rp, src->secs[q]}) : !physical(sym, rp, b)) continue;
            auto& v = acc[rp];
            v.push_back({src->secs[q], v.empty() ? 0 : v.back().off + v.back().dim, src->dims[q]});
        }
    }
    std::vector<std::pair<Sec, int>> tot;
    f->sig = "F" + src->key + "|";
    for (auto& kv : acc) {
        tot.push_back({kv.first, kv.second.back().off + kv.second.back().dim});
        for (auto& p : kv.second) {
            const int32_t rec[4] = {kv.first.N, kv.first.j, p.r.N, p.r.j};
            f->sig.append((const char*)rec, sizeof(rec));
        }
        f->parts[skey(kv.first)] = std::move(kv.second);
    }
    f->bond = std::make_shared<Bond>(tot);
    return f;
}

// bare recoupling coefficient x tilde factor; spins doubled, abelian kinds pass zeros
double opened_coef(int jl, int jsp, int jr, int k, int jrp, int js) {
    const double ph = ((jl + jsp + k + jrp) / 2) & 1 ? -1.0 : 1.0;
    return ph * sqrt((double)((jr + 1) * (js + 1))) * wigner6j(jl, jsp, jr, k, jrp, js) * sqrt((double)(jrp + 1) / (double)(jr + 1));
}
double passed_coef(int jl, int jlp, int js, int k, int jr, int jrp) {
    const double ph = ((k + js + jlp + jr) / 2) & 1 ? -1.0 : 1.0;
    return ph * sqrt((double)((jlp + 1) * (jr + 1))) * wigner6j(k, jl, jlp, js, jrp, jr) *
           sqrt((double)((jrp + 1) * (jl + 1)) / (double)((jlp + 1) * (jr + 1)));
}

// the source of sub-block (l' <- l, s, r' <- r) of the new tensor: block index in S and coefficient; -1: none (zeros).
// -2: more than one site state feeds it (block_place does not add)
int place_source(const Sym& sym, const SiteOp& op, bool opened, const SiteLayout& S, Sec l, Sec lp, int s, Sec r, Sec rp, double* coef) {
    if (rp.N != sym.wrapN(lp.N + sym.site[s].N) || !sym.triangle(lp.j, sym.site[s].j, rp.j)) return -1;
    const int k = sym.jeff(op.k), js = sym.jeff(sym.site[s].j);
    if (!opened) {
        const int q = S.block(l, s, r);
        if (q < 0) return -1;
        *coef = passed_coef(sym.jeff(l.j), sym.jeff(lp.j), js, k, sym.jeff(r.j), sym.jeff(rp.j));
        return *coef == 0.0 ? -1 : q;
    }
    int found = -1;
    for (int sp = 0; sp < sym.n_site; ++sp) {
        const double red = op.red[s][sp];
        if (red == 0.0) continue;
        const int q = S.block(l, sp, r);
        if (q < 0) continue;
        const double c = red * ((l.N & 1) && (op.dN & 1) ? -1.0 : 1.0) *
                         opened_coef(sym.jeff(l.j), sym.jeff(sym.site[sp].j), sym.jeff(r.j), k, sym.jeff(rp.j), js);
        if (c == 0.0) continue;
        if (found >= 0) return -2;
        found = q;
        *coef = c;
    }
    return found;
}

// the (r', r) pairs of the right bond that receive something from the left (apply_op keeps only those: no dead sectors)
int reach(const Sym& sym, const SiteOp& op, bool opened, const SiteLayout& S, const Fused& FL, PairSet& out) {
    std::vector<Sec> tg;
    for (size_t q = 0; q < S.blocks.size(); ++q) {
        const Key& bk = S.bkeys[q];
        const Sec l{bk[0], bk[1]}, r{bk[3], bk[4]};
        targets(sym, r, op, tg);
        std::vector<Sec> lps;
        if (opened)
            lps.push_back(l);
        else {
            std::vector<Sec> cand;
            targets(sym, l, op, cand);
            for (Sec c : cand) {
                const auto* ps = FL.of(c);
                if (!ps) continue;
                for (const FPart& p : *ps)
                    if (p.r == l) lps.push_back(c);
            }
        }
        for (Sec lp : lps)
            for (Sec rp : tg)
                for (int s = 0; s < sym.n_site; ++s) {
                    if (!opened && s != bk[2]) continue;
                    if (opened && op.red[s][bk[2]] == 0.0) continue;
                    double c = 0.0;
                    const int src = place_source(sym, op, opened, S, l, lp, s, r, rp, &c);
                    if (src == -2) return set_error("apply_op: the operator maps two site states onto one: not supported");
                    if (src >= 0) out.insert({rp, r});
                }
    }
    return 0;
}

int plan_place(const Sym& sym, const SiteOp& op, bool opened, const SiteLayout& S, const Fused& FL, const Fused& FR, PlaceC& out) {
    out.lay = build_site_layout(sym, S.kind, FL.bond, FR.bond);
    const SiteLayout& N = *out.lay;
    for (size_t q = 0; q < N.blocks.size(); ++q) {
        const Key& bk = N.bkeys[q];
        const Sec lp{bk[0], bk[1]}, rp{bk[3], bk[4]};
        const int s = bk[2];
        const BlockRec& D = N.blocks[q];
        const auto *pls = FL.of(lp), *prs = FR.of(rp);
        if (!pls || !prs) return set_error("apply_op: internal error (a block of the new layout has no parts)");
        for (const FPart& pl : *pls)
            for (const FPart& pr : *prs) {
                htn_place_item it;
                memset(&it, 0, sizeof(it));
                it.dst_off = D.off + pl.off + (int64_t)pr.off * D.ld;
                it.rows = pl.dim, it.cols = pr.dim, it.ldd = D.ld;
                it.src_off = -1, it.lds = 1, it.coef = 0.0;
                double c = 0.0;
                const int src = place_source(sym, op, opened, S, pl.r, lp, s, pr.r, rp, &c);
                if (src == -2) return set_error("apply_op: the operator maps two site states onto one: not supported");
                if (src >= 0) {
                    const BlockRec& B = S.blocks[src];
                    it.src_off = B.off, it.lds = B.ld, it.coef = c;
                }
                out.items.push_back(it);
            }
    }
    return 0;
}

int load_op(const Sym& sym, const htn_site_op* o, OpInfo& out) {
    out.op.k = o->k, out.op.dN = o->dN;
    for (int a = 0; a < HTN_MAX_SITE; ++a)
        for (int b = 0; b < HTN_MAX_SITE; ++b) out.op.red[a][b] = a < sym.n_site && b < sym.n_site ? o->red[a * HTN_MAX_SITE + b] : 0.0;
    if (sym.su2() && o->k < 0) return set_error("the operator rank is negative");
    out.tag.assign((const char*)o, sizeof(*o));
    return 0;
}

// what both entries ask of the state the operator acts on
int applyop_checks(const htn_mps* m, const SiteOp& op, const char* who) {
    const htn_ctx* ctx = m->ctx;
    if (ctx->world > 1 || ctx->shard || ctx->exch || m->be->has_comm())
        return set_error("%s: not available on a context with a communicator or an exchange hook", who);
    if (!m->orth.empty()) return set_error("%s: not available for a state with attached orthogonal states", who);
    const int L = m->L;
    if (m->Llay[0]->size != 0 || m->Rlay[L]->size != 0 || m->bonds[0]->multiplets() != 1 || m->bonds[L]->multiplets() != 1)
        return set_error("%s: needs a finite chain with open ends (end bonds of one sector, dimension 1)", who);
    const Sym& sym = m->mpo->sym;
    if (sym.su2() && op.k != 0 && m->bonds[L]->secs[0].j != 0)
        return set_error("%s: the state has total spin %d/2 and the operator rank %d/2: the sector of the result would not be unique "
                         "(the state must have total spin 0 or the operator rank 0)", who, m->bonds[L]->secs[0].j, op.k);
    return 0;
}

// the compiled site tensor (opened on the operator's site, passed right of it) of `m`'s site i between the given fused bonds
std::shared_ptr<PlaceC> place_plan(htn_mps* m, const OpInfo& oi, bool opened, int i, const FusedP& FL, const FusedP& FR) {
    const SiteLayout& S = *m->site_lay[i];
    return m->cached<PlaceC>(std::string(opened ? "aopX" : "aopT") + S.kind + oi.tag + FL->sig + "|" + FR->sig, [&]() -> std::shared_ptr<PlaceC> {
        auto p = std::make_shared<PlaceC>();
        if (plan_place(m->mpo->sym, oi.op, opened, S, *FL, *FR, *p)) return nullptr;
        if (!(p->items_dev = upload_vec(m->be, p->items))) return nullptr;
        return p;
    });
}
int place_run(htn_mps* m, const PlaceC& p, int i, cplx* dst) {
    return m->be->block_place(dst, m->site_buf[i].ptr(), (const htn_place_item*)p.items_dev->p, p.items.data(), (int)p.items.size());
}

}  // namespace

// ---- htn_mps_apply_op --------------------------------------------------------------------------------------------------------
int htn_mps::apply_op(int x, const htn_site_op* op_in, htn_mps** out, double* norm2_host) {
    const char* who = "htn_mps_apply_op";
    const Sym& sym = mpo->sym;
    if (x < 0 || x >= L) return set_error("%s: site %d out of range (the chain has %d sites)", who, x, L);
    OpInfo oi;
    if (load_op(sym, op_in, oi) || applyop_checks(this, oi.op, who)) return 1;
    if (centre != x) return set_error("%s: the centre is on site %d, not on site %d", who, centre, x);
    for (int i = 0; i < L; ++i)
        if (i != x && site_lay[i]->kind != (i < x ? 'L' : 'R'))
            return set_error("%s: site %d is not in %s layout (the centre is on site %d)", who, i, i < x ? "left" : "right", x);

    // bond tables and site plans, left to right; a pair (r', r) is kept only if something arrives in it
    std::vector<FusedP> fb(L + 1);
    std::vector<std::shared_ptr<PlaceC>> plans(L);
    fb[x] = identity_fused(bonds[x]);
    bool pruned = true;
    for (int i = x; i < L; ++i) {
        auto f = cached<Fused>(std::string("aopB") + (pruned ? "p" : "a") + site_lay[i]->kind + oi.tag + fb[i]->sig + "|" + bonds[i + 1]->key,
                               [&]() -> std::shared_ptr<Fused> {
                                   PairSet keep;
                                   if (pruned && reach(sym, oi.op, i == x, *site_lay[i], *fb[i], keep)) return nullptr;
                                   return std::const_pointer_cast<Fused>(fuse_bond(sym, bonds[i + 1], oi.op, i + 1, pruned ? &keep : nullptr));
                               });
        if (!f) return 1;
        if (f->bond->secs.empty() && pruned) {       // the operator annihilates the state: zero tensors on every sector the sites can hold
            pruned = false;
            --i;
            continue;
        }
        if (f->bond->secs.empty()) return set_error("%s: no sector of bond %d can take the operator's charge", who, i + 1);
        fb[i + 1] = f;
        if (!(plans[i] = place_plan(this, oi, i == x, i, fb[i], fb[i + 1]))) return 1;
    }
    if (fb[L]->bond->multiplets() != 1) return set_error("%s: the end bond of the result is not one sector of dimension 1", who);

    MpsGuard g{mps_new(ctx, mpo_handle)};
    htn_mps* e = g.p;
    e->bonds.resize(L + 1);
    for (int b = 0; b <= L; ++b) e->bonds[b] = b <= x ? bonds[b] : fb[b]->bond;
    for (int i = 0; i < L; ++i) {
        e->site_lay[i] = i < x ? site_lay[i] : plans[i]->lay;
        e->site_buf[i] = e->zalloc(e->site_lay[i]->size, false);
        if (!e->site_buf[i].base) return set_error("%s: device allocation failed", who);
        if (i < x ? relay(*site_lay[i], site_buf[i].ptr(), *site_lay[i], e->site_buf[i].ptr()) : place_run(this, *plans[i], i, e->site_buf[i].ptr()))
            return 1;
    }
    // boundaries as mps_finish builds them for open ends, then the environments the centre position needs
    e->Llay[0] = build_env_layout(sym, 'L', e->bonds[0], mpo->sites[0].left);
    e->Rlay[L] = build_env_layout(sym, 'R', e->bonds[L], mpo->sites[L - 1].right);
    e->Lbuf[0] = e->zalloc(e->Llay[0]->size, true);
    e->Rbuf[L] = e->zalloc(e->Rlay[L]->size, true);
    if (!e->Lbuf[0].base || !e->Rbuf[L].base) return set_error("%s: device allocation failed", who);
    for (int i = 0; i < x; ++i)
        if (e->left_env(i)) return 1;
    for (int i = L - 1; i > x; --i)
        if (e->right_env(i)) return 1;
    e->centre = x;
    e->energy = NAN;
    double v[2];
    if (e->overlap(e, v)) return 1;      // (one download: the pass is complete when the call returns)
    e->raw_n2 = std::max(v[0], 0.0);
    if (norm2_host) *norm2_host = v[0];
    g.p = nullptr;
    *out = e;
    return 0;
}

// ---- htn_mps_transition ------------------------------------------------------------------------------------------------------
namespace {

// one overlap transfer with an explicit bra tensor (layout lb, device data bs) against site i of `ket`; plans live in m's cache
int ovl_step_with(htn_mps* m, char side, const SiteLayout& lb, const cplx* bs, const htn_mps* ket, int i, const OvlLayoutP& inl, const DView& in,
                  OvlLayoutP* outl, DView* out) {
    const bool left = side == 'L';
    const SiteLayout& lk = *ket->site_lay[i];
    auto c = m->cached<OvlC>(std::string(left ? "aopOL" : "aopOR") + lb.kind + lk.kind + lb.bl->key + "|" + lb.br->key + "|" + ket->bonds[i]->key + "|" +
                                 ket->bonds[i + 1]->key,
                             [&]() -> std::shared_ptr<OvlC> {
                                 auto e = std::make_shared<OvlC>();
                                 e->lay = left ? build_ovl_layout(lb.br, ket->bonds[i + 1]) : build_ovl_layout(ket->bonds[i], lb.bl);
                                 OvlPlan p;
                                 (left ? plan_ovl_left : plan_ovl_right)(*inl, lb, lk, *e->lay, p);
                                 return m->compile2(e, p);
                             });
    if (!c) return 1;
    DView z = m->zalloc(c->zsize, false), o = m->zalloc(c->lay->size, true);
    if (!z.base || !o.base) return set_error("device allocation failed (overlap environment)");
    if (m->gemm(c->d1, {{left ? BUF_L : BUF_R, in.ptr()}, {BUF_S2, ket->site_buf[i].ptr()}, {BUF_Z, z.ptr()}})) return 1;
    if (m->gemm(c->d2, {{BUF_S1, bs}, {BUF_Z, z.ptr()}, {BUF_Y, o.ptr()}})) return 1;
    *outl = c->lay;
    *out = o;
    return 0;
}

}  // namespace

int htn_mps::transition(const htn_site_op* op_in, const htn_mps* ket, cplx* out_host) {
    const char* who = "htn_mps_transition";
    const Sym& sym = mpo->sym;
    if (ctx != ket->ctx) return set_error("%s: the states live in different contexts", who);
    if (L != ket->L) return set_error("%s: %d and %d sites", who, L, ket->L);
    OpInfo oi;
    if (load_op(sym, op_in, oi) || applyop_checks(this, oi.op, who)) return 1;
    {
        const Sym& b = ket->mpo->sym;
        bool same = sym.kind == b.kind && sym.n_site == b.n_site;
        for (int q = 0; same && q < sym.n_site; ++q) same = sym.site[q] == b.site[q];
        if (!same) return set_error("%s: the states have different symmetries", who);
    }
    // the passed tensors do not depend on x: every bond b >= 1 fused once, every sector the sites can hold
    std::vector<FusedP> fb(L + 1);
    for (int b = 1; b <= L; ++b) {
        fb[b] = cached<Fused>(std::string("aopBa") + ikey("b", b) + oi.tag + bonds[b]->key, [&]() -> std::shared_ptr<Fused> {
            return std::const_pointer_cast<Fused>(fuse_bond(sym, bonds[b], oi.op, b, nullptr));
        });
        if (!fb[b]) return 1;
    }
    OvlLayoutP endl = build_ovl_layout(ket->bonds[L], fb[L]->bond), startl = build_ovl_layout(bonds[0], ket->bonds[0]);
    if (fb[L]->bond->multiplets() != 1 || ket->bonds[L]->multiplets() != 1 || endl->size != 1 || startl->size != 1)
        return set_error("%s: the total sector of the ket is not the sector of the bra fused with the operator's charge (dN %d, k %d)", who,
                         oi.op.dN, oi.op.k);
    const cplx one(1.0, 0.0);
    // ---- right pass: O_R'[b] (ket x passed bra) for b = L .. 1 ----
    std::vector<OvlLayoutP> Rl(L + 1);
    std::vector<DView> Rb(L + 1);
    Rl[L] = endl;
    Rb[L] = zalloc(1, false);
    DView table = zalloc(L, true);
    if (!Rb[L].base || !table.base || be->upload(Rb[L].ptr(), &one, sizeof(one))) return set_error("%s: device allocation failed", who);
    for (int i = L - 1; i >= 1; --i) {
        auto p = place_plan(this, oi, false, i, fb[i], fb[i + 1]);
        if (!p) return 1;
        DView t = zalloc(p->lay->size, false);
        if (!t.base) return set_error("%s: device allocation failed", who);
        if (place_run(this, *p, i, t.ptr())) return 1;
        if (ovl_step_with(this, 'R', *p->lay, t.ptr(), ket, i, Rl[i + 1], Rb[i + 1], &Rl[i], &Rb[i])) return 1;
    }
    // ---- left pass with the bra's own tensors; on every site the opened tensor, closed against the right half ----
    OvlLayoutP Ll = startl;
    DView Lb = zalloc(1, false);
    if (!Lb.base || be->upload(Lb.ptr(), &one, sizeof(one))) return set_error("%s: device allocation failed", who);
    for (int x = 0; x < L; ++x) {
        auto p = place_plan(this, oi, true, x, identity_fused(bonds[x]), fb[x + 1]);
        if (!p) return 1;
        DView t = zalloc(p->lay->size, false);
        if (!t.base) return set_error("%s: device allocation failed", who);
        if (place_run(this, *p, x, t.ptr())) return 1;
        OvlLayoutP Xl;
        DView Xb;
        if (ovl_step_with(this, 'L', *p->lay, t.ptr(), ket, x, Ll, Lb, &Xl, &Xb)) return 1;
        const OvlLayoutP& Ro = Rl[x + 1];
        auto m = cached<MeetC>(std::string("aopM") + oi.tag + fb[x + 1]->sig + "|" + ket->bonds[x + 1]->key, [&]() -> std::shared_ptr<MeetC> {
            auto mc = std::make_shared<MeetC>();
            for (size_t q = 0; q < Xl->secs.size(); ++q) {
                const int rq = Ro->find(Xl->secs[q]);
                if (rq < 0) continue;
                htn_trdot_item it;
                memset(&it, 0, sizeof(it));
                it.a_off = Xl->off[q], it.b_off = Ro->off[rq];
                it.rows = Xl->m[q], it.cols = Xl->n[q], it.lda = Xl->m[q], it.ldb = Ro->m[rq];
                it.out = 0, it.w_re = 1.0;
                mc->items.push_back(it);
            }
            if (!(mc->items_dev = upload_vec(be, mc->items))) return nullptr;
            return mc;
        });
        if (!m) return 1;
        if (be->block_trdots(Xb.ptr(), Rb[x + 1].ptr(), (const htn_trdot_item*)m->items_dev->p, m->items.data(), (int)m->items.size(),
                             table.ptr() + x, 1))
            return 1;
        if (x + 1 < L) {
            OvlLayoutP nl;
            DView nb;
            if (ovl_step('L', ket, x, Ll, Lb, &nl, &nb)) return 1;
            Ll = nl, Lb = nb;
        }
    }
    if (be->download(out_host, table.ptr(), sizeof(cplx) * (size_t)L)) return 1;
    if (amp != 1.0 || ket->amp != 1.0)
        for (int x = 0; x < L; ++x) out_host[x] *= amp * ket->amp;
    return 0;
}
