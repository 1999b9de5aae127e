// Correlation functions of an htn_mps (htn_engine.h), the state read only: two-point functions (htn_mps_correlator) and
// functions of two nearest-neighbour bond operators (htn_mps_correlator2).  One probe pass (htn_mps::corr_pass) behind both
// entries; an entry is its charge checks and a CorrProbe, the specification of what its pass differs in.
// Host C++ (no HIP).
// NOT a translation unit of its own: #included by htn_engine.cpp (one unit, see its head); never name it on a build line.
#include <functional>

#include "htn_engine.h"

// =====================================================================================================================
// Two-point correlation functions C(i, j) = <close_j . pass ... pass . open_i> of one channel for all i <= j
// (htn_mps_correlator).  Both halves are environments of small probe MPO sites, planned by plan_left_env /
// plan_right_env like the Hamiltonian's.  Those planners keep one level implicit (the left 'start', the right 'final': the
// identity of a canonical state); the norm environments of a state in ANY gauge are not the identity, so the probes put an
// unused level into that place and carry the norm level explicitly:
//   left probe, every site      left [-, norm]   right [-, norm, open, done]      (norm -> norm, id) (norm -> open, open)
//                                                                                 (norm -> done, onsite)
//   right probe, site j         right [norm, open_{j+1} .. open_{L-1}, -]   left [norm, open_j, open_{j+1} .. open_{L-1}, -]
//                                                                                 (norm <- norm, id) (open_j <- norm, close)
//                                                                                 (open_j' <- open_j', pass)
// The left pass keeps the output of every site (norm level first: the buffer is the next site's input as it stands); the right
// pass keeps the current bond only and meets the left half of bond b = i + 1 in one block_trdots launch:
//   C(i, j) = sum_{bra, ket} (2S_bra + 1) / (2S_ket + 1) tr(Lopen_i[bra, ket] Ropen_j[ket, bra])
// -- the factor H_eff's apply closes a right environment with (coef_apply), independent of the level's spin and of the gauge:
// the stored tensors of a path carry sqrt(2J + 1) in all (ovl_step's note) --, C(i, i) = <Lclosed_i, Rnorm>, <psi|psi> = <rho, Rnorm>.
// Results of bond b go to row i of a device table shifted by one element: the norm lands in the unused slot (i, i - 1).
//
// Two nearest-neighbour bond operators, C(i, j) = <close1_{j+1} close0_j . pass ... pass . open1_{i+1} open0_i> of one channel
// for all j >= i + 2 (htn_mps_correlator2): the same scheme with two more probe levels per end:
//   left probe, every site      left [-, norm, half]   right [-, norm, half, open]
//                                                      (norm -> norm, id) (norm -> half, open0) (half -> open, open1)
//   right probe, site b         right [norm, halfR, open_{b+1} .. open_{L-2}, -]   left [norm, halfR', open_b, open_{b+1} .. open_{L-2}, -]
//                                                      (norm <- norm, id) (halfR' <- norm, close1) (open_b <- halfR, close0)
//                                                      (open_j' <- open_j', pass)
// (n_close = 1: no halfR level, open_b <- norm by close0, j up to L - 1).  The left buffer of a bond lists its levels in
// order, so the output of site i, read with the first three levels, is the input of site i + 1 as it stands.  The open level
// that site i + 1 writes and the right half meet on bond b = i + 2.
// =====================================================================================================================
struct CorrProbe {
    const char* who;               // the entry, in error texts
    std::string name, tag;         // plan-cache keys: name + 'L' / 'R' / 'M', then the probe's own name: its operator tables
    Mpo ops;                       // probe operators (probe_ops): the identity, then the entry's
    MpoSite WL;                    // the left probe site
    bool wide_start;               // bond 0 of the left pass holds every level of WL.left (zero but the norm), not the norm alone
    // n_left and dist decide which bonds meet and which rows hold results: the left pass crosses the sites 0 .. n_left - 1, so the
    // bonds dist <= b <= n_left have a left half; bond b closes row i = b - dist, whose results are its columns j >= i + dist.
    // Hence rows = n_left - dist + 1 rows met a right half (and carry their norm); the rows below stay zero
    int n_left, dist;
    int open_l, onsite_l;          // levels of WL.right that meet the right half: open (-> C(i, j)), closed on the site (-> C(i, i); -1: none)
    int first, pass_op;            // right half: index of the first open level of a bond, probe operator that carries one across a site
    std::function<std::string(int)> bond_tag;      // plan-cache key part of bond b (right probe site and meet)
    // the right probe site of site b: puts its new level into the levels of bond b + 1 and adds the entries that close onto it
    std::function<void(int, std::vector<Lvl>&, std::vector<MpoEntry>&)> grow;
};
struct MeetPair {                  // the blocks of left level wl meet those of right level wr; the sum goes to element `out` of the row
    int wl, wr, out;
};

// what both entries ask of the context, the pass operator and the chain
int htn_mps::corr_checks(const char* who, const htn_site_op& pass, const char* ends_note) {
    if (ctx->world > 1 || ctx->shard || ctx->exch || be->has_comm())
        return set_error("%s: not available on a context with a communicator or an exchange hook", who);
    if (pass.dN != 0 || pass.k != 0) return set_error("%s: the pass operator carries a charge (dN %d, k %d)", who, pass.dN, pass.k);
    if (Llay[0]->size != 0 || Rlay[L]->size != 0 || bonds[0]->multiplets() != 1 || bonds[L]->multiplets() != 1)
        return set_error("%s: needs a finite chain with open ends (end bonds of one sector, dimension 1)%s", who, ends_note);
    return 0;
}

// operator table of a probe MPO: 0 the identity, then `ops` in order
static Mpo probe_ops(const Sym& sym, std::initializer_list<const htn_site_op*> ops) {
    Mpo pm;
    pm.sym = sym;
    auto add_op = [&](const htn_site_op& o) {
        SiteOp r;
        r.k = o.k, r.dN = o.dN;
        for (int a = 0; a < HTN_MAX_SITE; ++a)
            for (int b = 0; b < HTN_MAX_SITE; ++b) r.red[a][b] = o.red[a * HTN_MAX_SITE + b];
        pm.ops.push_back(r);
    };
    htn_site_op ident;
    memset(&ident, 0, sizeof(ident));
    for (int s = 0; s < sym.n_site; ++s) ident.red[s * HTN_MAX_SITE + s] = 1.0;
    add_op(ident);
    for (const htn_site_op* o : ops) add_op(*o);
    return pm;
}

// site i's tensor in the layout `want` (of its own bonds): the stored buffer if it is of that kind, else a pool block it is re-laid into
DView htn_mps::site_as(const SiteLayout& want, int i) {
    if (site_lay[i]->kind == want.kind) return site_buf[i];
    DView v = zalloc(want.size, false);
    if (!v.base) set_error("device allocation failed (site %d in %c layout)", i, want.kind);
    else if (relay(*site_lay[i], site_buf[i].ptr(), want, v.ptr())) v = DView();
    return v;
}

// One step of a probe environment across site i, either side (env_step's twin for an MPO site that is not the Hamiltonian's):
// `in` lives on bond i (left) / i + 1 (right) in the layout `inl` of the levels W.left / W.right (null: built when the step is
// planned); the plan is filed under `key`
int htn_mps::probe_step(char side, const Mpo& pm, const MpoSite& W, const EnvLayoutP& inl, const cplx* in, int i, const std::string& key,
                        EnvLayoutP* outl, DView* out) {
    const bool left = side == 'L';
    const SiteLayoutP lay = site_layout(side, bonds[i], bonds[i + 1]);
    const DView site = site_as(*lay, i);
    if (!site.base) return 1;
    auto c = cached<EnvC>(key, [&]() -> std::shared_ptr<EnvC> {
        auto e = std::make_shared<EnvC>();
        e->lay = build_env_layout(pm.sym, side, bonds[left ? i + 1 : i], left ? W.right : W.left);
        EnvPlan p;
        const EnvLayoutP il = inl ? inl : build_env_layout(pm.sym, side, bonds[left ? i : i + 1], left ? W.left : W.right);
        (left ? plan_left_env : plan_right_env)(pm, *il, *lay, W, *e->lay, p);
        return compile2(e, p);
    });
    if (!c || env_launch(left, *c, in, site.ptr(), out)) return 1;
    *outl = c->lay;
    return 0;
}

// the trace-dot items of one bond: for every pair, the blocks of the left level against their partners of the right level, with
// the block weight (2S_bra + 1) / (2S_ket + 1)
static std::shared_ptr<MeetC> meet_items(Backend* be, const Sym& sym, const EnvLayout& Ll, const EnvLayout& Rl, const std::vector<MeetPair>& pairs) {
    auto mc = std::make_shared<MeetC>();
    for (const MeetPair& pr : pairs)
        for (size_t q = 0; q < Ll.blocks.size(); ++q) {
            const Key& k = Ll.bkeys[q];
            if (k[2] != pr.wl) continue;
            const Sec bra{k[0], k[1]}, ket{k[3], k[4]};
            const int rq = Rl.block(ket, pr.wr, bra);
            if (rq < 0) continue;
            const auto &lb = Ll.blocks[q], &rb = Rl.blocks[rq];
            htn_trdot_item it;
            memset(&it, 0, sizeof(it));
            it.a_off = lb.off, it.b_off = rb.off;
            it.rows = lb.m, it.cols = lb.n, it.lda = lb.m, it.ldb = rb.m;
            it.out = pr.out;
            it.w_re = (double)sym.qdim(bra) / (double)sym.qdim(ket);
            mc->items.push_back(it);
        }
    if (!(mc->items_dev = upload_vec(be, mc->items))) return nullptr;
    return mc;
}

// The pass: left environments of every bond (kept until the right pass has met them: O(L chi^2) in all), then the right half
// from bond L down, one meet per bond into row i of the device table, one download, every row divided by its own <psi|psi>
int htn_mps::corr_pass(const CorrProbe& p, cplx* out_host, double* norm_host) {
    const Sym& sym = mpo->sym;
    const cplx one(1.0, 0.0);
    auto unit = [&](int64_t n, bool zero) {                        // a buffer that starts with the norm of an end bond, 1
        DView v = zalloc(n, zero);
        if (!v.base || be->upload(v.ptr(), &one, sizeof(one))) set_error("%s: device allocation failed", p.who), v = DView();
        return v;
    };
    auto bkey = [&](int i) { return bonds[i]->key + "|" + bonds[i + 1]->key; };

    std::vector<EnvLayoutP> Hlay(L + 1);
    std::vector<DView> Hbuf(L + 1);
    Hbuf[0] = unit(p.wide_start ? build_env_layout(sym, 'L', bonds[0], p.WL.left)->size : 1, p.wide_start);
    if (!Hbuf[0].base) return 1;
    for (int i = 0; i < p.n_left; ++i)                             // (the kept output of site i - 1 lists one level more than WL.left: no layout to pass)
        if (probe_step('L', p.ops, p.WL, nullptr, Hbuf[i].ptr(), i, p.name + "L" + p.tag + bkey(i), &Hlay[i + 1], &Hbuf[i + 1])) return 1;

    DView table = zalloc((int64_t)L * L + 1, true);
    if (!table.base) return set_error("%s: device allocation failed", p.who);
    std::vector<Lvl> rlev = {{0, 0}, {0, 0}};                      // levels of the right half on bond b: [norm, .. open_b .., -]
    EnvLayoutP Rl = build_env_layout(sym, 'R', bonds[L], rlev);
    DView Rb = unit(1, false);
    if (!Rb.base) return 1;
    for (int b = L; b >= p.dist; --b) {
        const int i = b - p.dist;
        if (b < L) {                                               // the right half crosses site b: bond b + 1 -> bond b
            MpoSite WR;
            WR.right = rlev;
            WR.entries = {{0, 0, 0, cplx(1.0)}};
            p.grow(b, rlev, WR.entries);
            WR.left = rlev;
            for (int w = p.first; w + 1 < (int)WR.right.size(); ++w) WR.entries.push_back({w + 1, w, p.pass_op, cplx(1.0)});
            if (probe_step('R', p.ops, WR, Rl, Rb.ptr(), b, p.name + "R" + p.tag + p.bond_tag(b) + bkey(b), &Rl, &Rb)) return 1;
        }
        if (b > p.n_left) continue;                                // (no left half yet: the bonds the close operators sit on)
        // results of this bond: 0 = <psi|psi>, 1 = C(i, i), 1 + (j - i) = C(i, j) for the closing sites j = b .. b + n_open - 1
        const int n_open = (int)rlev.size() - 1 - p.first;
        auto m = cached<MeetC>(p.name + "M" + p.tag + p.bond_tag(b) + bonds[b]->key, [&]() -> std::shared_ptr<MeetC> {
            std::vector<MeetPair> pairs = {{1, 0, 0}};
            if (p.onsite_l >= 0) pairs.push_back({p.onsite_l, 0, 1});
            for (int j = b; j < b + n_open; ++j) pairs.push_back({p.open_l, p.first + (j - b), 1 + (j - i)});
            return meet_items(be, sym, *Hlay[b], *Rl, pairs);
        });
        if (!m) return 1;
        if (be->block_trdots(Hbuf[b].ptr(), Rb.ptr(), (const htn_trdot_item*)m->items_dev->p, m->items.data(), (int)m->items.size(),
                             table.ptr() + ((int64_t)i * L + i), L - i + 1))
            return 1;
        Hbuf[b] = DView();
    }
    std::vector<cplx> t((size_t)L * L + 1);
    if (be->download(t.data(), table.ptr(), sizeof(cplx) * t.size())) return 1;
    const int rows = p.n_left - p.dist + 1;                        // rows i that met a right half
    for (int i = 0; i < L; ++i) {
        const cplx nrm = i < rows ? t[(size_t)i * L + i] : one;
        if (!(std::abs(nrm) > 0.0)) return set_error("%s: <psi|psi> = %g on bond %d", p.who, nrm.real(), i + p.dist);
        if (i == 0 && norm_host) *norm_host = nrm.real();
        for (int j = 0; j < L; ++j)
            out_host[(size_t)i * L + j] = i < rows && (j >= i + p.dist || (j == i && p.onsite_l >= 0)) ? t[1 + (size_t)i * L + j] / nrm : cplx(0.0, 0.0);
    }
    return 0;
}

int htn_mps::correlator(const htn_corr_channel& ch, cplx* out_host, double* norm_host) {
    const Sym& sym = mpo->sym;
    const char* who = "htn_mps_correlator";
    if (corr_checks(who, ch.pass, "")) return 1;
    if (ch.open.dN + ch.close.dN != 0 || (sym.su2() ? ch.open.k != ch.close.k : ch.open.k + ch.close.k != 0))
        return set_error("%s: the charges of open (dN %d, k %d) and close (dN %d, k %d) do not add up to zero", who, ch.open.dN, ch.open.k,
                         ch.close.dN, ch.close.k);
    if (ch.has_onsite && (ch.onsite.dN != 0 || ch.onsite.k != 0))
        return set_error("%s: the onsite operator carries a charge (dN %d, k %d)", who, ch.onsite.dN, ch.onsite.k);
    const bool onsite = ch.has_onsite != 0;
    const Lvl scalar{0, 0}, open{ch.open.dN, ch.open.k};
    CorrProbe p;
    p.who = who, p.name = "corr";
    p.tag.assign((const char*)&ch, sizeof(ch));
    p.ops = probe_ops(sym, {&ch.open, &ch.pass, &ch.close, &ch.onsite});      // 1 open, 2 pass, 3 close, 4 onsite
    p.WL.left = {scalar, scalar};
    p.WL.right = {scalar, scalar, open};
    p.WL.entries = {{1, 1, 0, cplx(1.0)}, {1, 2, 1, cplx(1.0)}};
    if (onsite) {
        p.WL.right.push_back(scalar);
        p.WL.entries.push_back({1, 3, 4, cplx(1.0)});
    }
    p.wide_start = false, p.n_left = L, p.dist = 1;
    p.open_l = 2, p.onsite_l = onsite ? 3 : -1, p.first = 1, p.pass_op = 2;
    p.bond_tag = [this](int b) { return ikey("K", L - b + 1); };  // K levels: norm + one per closing site j >= b
    p.grow = [&](int, std::vector<Lvl>& rlev, std::vector<MpoEntry>& e) {
        rlev.insert(rlev.begin() + 1, open);
        e.push_back({1, 0, 3, cplx(1.0)});
    };
    return corr_pass(p, out_host, norm_host);
}

int htn_mps::correlator2(const htn_corr_channel2& ch, cplx* out_host, double* norm_host) {
    const Sym& sym = mpo->sym;
    const char* who = "htn_mps_correlator2";
    if (corr_checks(who, ch.pass, ", not a window with boundary environments")) return 1;
    if (ch.n_close != 1 && ch.n_close != 2) return set_error("%s: n_close must be 1 or 2 (%d given)", who, ch.n_close);
    const bool two = ch.n_close == 2;
    if (L < (two ? 4 : 3)) return set_error("%s: the chain has %d sites, two disjoint bonds need at least %d", who, L, two ? 4 : 3);
    auto couples = [&](int ka, int kb, int kc) {                   // may ranks ka and kb add up to kc
        return sym.su2() ? (kc >= std::abs(ka - kb) && kc <= ka + kb && (ka + kb + kc) % 2 == 0) : ka + kb == kc;
    };
    const htn_site_op &o0 = ch.open[0], &o1 = ch.open[1], &c0 = ch.close[0], &c1 = ch.close[1];
    if (o0.dN + o1.dN != ch.open_dN || !couples(o0.k, o1.k, ch.open_k))
        return set_error("%s: the open operators (dN %d, k %d) and (dN %d, k %d) cannot couple to the level (dN %d, k %d)", who, o0.dN, o0.k,
                         o1.dN, o1.k, ch.open_dN, ch.open_k);
    const int cdN = c0.dN + (two ? c1.dN : 0);
    // the level between close0 and close1 carries what close1 takes to the scalar: (-dN, k) (abelian kind: -k)
    const Lvl halfR{two ? -c1.dN : 0, two ? (sym.su2() ? c1.k : -c1.k) : 0};
    if (ch.open_dN + cdN != 0 || !couples(ch.open_k, c0.k, halfR.k))
        return set_error("%s: the charges of the open pair (dN %d, k %d) and of the close operators (dN %d, k %d)%s do not add up to zero", who,
                         ch.open_dN, ch.open_k, c0.dN, c0.k, two ? " (dN, k of close[0]; close[1] follows)" : "");
    const Lvl scalar{0, 0}, half{o0.dN, o0.k}, open{ch.open_dN, ch.open_k};
    CorrProbe p;
    p.who = who, p.name = "corr2";
    htn_corr_channel2 named = ch;                                  // the probe's name in the plan cache: its operator tables,
    named.pad = 0;                                                 // without the fields the pass does not read
    if (!two) memset(&named.close[1], 0, sizeof(named.close[1]));
    p.tag.assign((const char*)&named, sizeof(named));
    p.ops = probe_ops(sym, {&o0, &o1, &ch.pass, &c0, &c1});       // 1 open0, 2 open1, 3 pass, 4 close0, 5 close1
    p.WL.left = {scalar, scalar, half};
    p.WL.right = {scalar, scalar, half, open};
    p.WL.entries = {{1, 1, 0, cplx(1.0)}, {1, 2, 1, cplx(1.0)}, {2, 3, 2, cplx(1.0)}};
    p.wide_start = true, p.n_left = L - ch.n_close, p.dist = 2;   // the last bond that is met is L - 1 (n_close = 1) or L - 2
    p.open_l = 3, p.onsite_l = -1, p.first = two ? 2 : 1, p.pass_op = 3;
    p.bond_tag = [](int b) { return ikey("b", b); };
    p.grow = [&, two](int b, std::vector<Lvl>& rlev, std::vector<MpoEntry>& e) {
        if (!two) {
            rlev.insert(rlev.begin() + 1, open);
            e.push_back({1, 0, 4, cplx(1.0)});
        } else if (b == L - 1) {
            rlev.insert(rlev.begin() + 1, halfR);
            e.push_back({1, 0, 5, cplx(1.0)});
        } else {
            rlev.insert(rlev.begin() + 2, open);
            if (b > 2) e.push_back({1, 0, 5, cplx(1.0)});          // (the halfR level of bond 2 would be read by nothing)
            e.push_back({2, 1, 4, cplx(1.0)});
        }
    };
    return corr_pass(p, out_host, norm_host);
}
