// Overlaps and measurements of an htn_mps (htn_engine.h): overlap environments <psi|phi>, the states attached to an
// orthogonalised sweep (htn_mps_set_orthogonal, htn_mps_overlap), two-point correlation functions (htn_mps_correlator),
// correlation functions of nearest-neighbour bond operators (htn_mps_correlator2).
// Host C++ (no HIP).
// NOT a translation unit of its own: #included by htn_engine.cpp (one unit, see its head); never name it on a build line.
#include "htn_engine.h"

// ---- overlap environments (orthogonalised DMRG, htn_mps_overlap) ------------------------------------------------------
int htn_mps::ovl_boundary(const htn_mps* ket, int b, OvlLayoutP* outl, DView* out) {
    OvlLayoutP lay = b == 0 ? build_ovl_layout(bonds[0], ket->bonds[0]) : build_ovl_layout(ket->bonds[L], bonds[L]);
    if (lay->size != 1) return set_error("overlap: the end bonds of the two states are not one common sector of dimension 1");
    DView v = zalloc(1, false);
    const cplx one(1.0, 0.0);
    if (!v.base || be->upload(v.ptr(), &one, sizeof(one))) return set_error("overlap: device allocation failed");
    *outl = lay;
    *out = v;
    return 0;
}

// side 'L': O_L[bra x ket] moves from bond i to bond i+1; side 'R': O_R[ket x bra] from bond i+1 to bond i (the output is
// zero-filled: a transfer leaves sectors without a contribution unwritten)
int htn_mps::ovl_step(char side, const htn_mps* ket, int i, const OvlLayoutP& inl, const DView& in, OvlLayoutP* outl, DView* out) {
    const bool left = side == 'L';
    const SiteLayout &lb = *site_lay[i], &lk = *ket->site_lay[i];
    auto c = cached<OvlC>(std::string(left ? "ovlL" : "ovlR") + lb.kind + lk.kind + bonds[i]->key + "|" + bonds[i + 1]->key + "|" +
                              ket->bonds[i]->key + "|" + ket->bonds[i + 1]->key,
                          [&]() -> std::shared_ptr<OvlC> {
                              auto e = std::make_shared<OvlC>();
                              e->lay = left ? build_ovl_layout(bonds[i + 1], ket->bonds[i + 1]) : build_ovl_layout(ket->bonds[i], bonds[i]);
                              OvlPlan p;
                              (left ? plan_ovl_left : plan_ovl_right)(*inl, lb, lk, *e->lay, p);
                              return compile2(e, p);
                          });
    if (!c) return 1;
    DView z = zalloc(c->zsize, false), o = zalloc(c->lay->size, true);
    if (!z.base || !o.base) return set_error("device allocation failed (overlap environment)");
    if (gemm(c->d1, {{left ? BUF_L : BUF_R, in.ptr()}, {BUF_S2, ket->site_buf[i].ptr()}, {BUF_Z, z.ptr()}})) return 1;
    if (gemm(c->d2, {{BUF_S1, site_buf[i].ptr()}, {BUF_Z, z.ptr()}, {BUF_Y, o.ptr()}})) return 1;
    *outl = c->lay;
    *out = o;
    return 0;
}

// row of the projector: <phi| carried into the bases of this state's bond (i, i+1), in its theta layout
int htn_mps::ovl_project(const OrthState& os, int i, const ThetaLayout& tl, cplx* dst) {
    const htn_mps* ket = os.phi;
    const SiteLayout &k1 = *ket->site_lay[i], &k2 = *ket->site_lay[i + 1];
    auto c = cached<OvlC>(std::string("ovlP") + k1.kind + k2.kind + bonds[i]->key + "|" + bonds[i + 2]->key + "|" + ket->bonds[i]->key + "|" +
                              ket->bonds[i + 1]->key + "|" + ket->bonds[i + 2]->key,
                          [&]() -> std::shared_ptr<OvlC> {
                              OvlPlan p;
                              plan_ovl_project(*os.Llay[i], *os.Rlay[i + 2], k1, k2, tl, p);
                              return compile2(std::make_shared<OvlC>(), p);
                          });
    if (!c) return 1;
    DView z = zalloc(c->zsize, false);
    if (!z.base) return set_error("device allocation failed (projector row)");
    if (gemm(c->d1, {{BUF_L, os.Lbuf[i].ptr()}, {BUF_R, os.Rbuf[i + 2].ptr()}, {BUF_S1, ket->site_buf[i].ptr()},
                     {BUF_S2, ket->site_buf[i + 1].ptr()}, {BUF_Z, z.ptr()}}))
        return 1;
    return gemm(c->d2, {{BUF_Z, z.ptr()}, {BUF_Y, dst}});
}

void htn_mps::orth_detach() {
    for (auto& os : orth) htn_mps_destroy(os.phi);
    orth.clear();
    orth_dropped = 0;
}

// Overlap environments of every bond from the tensors as they are now (a scalar transfer needs no particular gauge); the
// sweep then keeps them current exactly as it keeps the H environments.  The attached states must not change while attached.
int htn_mps::orth_attach(htn_mps* const* others, int n) {
    std::vector<OrthState> fresh((size_t)n);
    for (int k = 0; k < n; ++k) {
        OrthState& os = fresh[k];
        os.phi = others[k];
        os.Llay.resize(L + 1);
        os.Rlay.resize(L + 1);
        os.Lbuf.resize(L + 1);
        os.Rbuf.resize(L + 1);
        if (ovl_boundary(os.phi, 0, &os.Llay[0], &os.Lbuf[0]) || ovl_boundary(os.phi, L, &os.Rlay[L], &os.Rbuf[L])) return 1;
        for (int i = 0; i < L; ++i)
            if (ovl_step('L', os.phi, i, os.Llay[i], os.Lbuf[i], &os.Llay[i + 1], &os.Lbuf[i + 1])) return 1;
        for (int i = L - 1; i >= 0; --i)
            if (ovl_step('R', os.phi, i, os.Rlay[i + 1], os.Rbuf[i + 1], &os.Rlay[i], &os.Rbuf[i])) return 1;
    }
    if (be->sync()) return 1;
    for (int k = 0; k < n; ++k) ++others[k]->refs;
    orth_detach();
    orth.swap(fresh);
    return 0;
}

// ---- htn_mps_set_orthogonal / htn_mps_overlap ---------------------------------------------------------------------------
int htn_mps::set_orthogonal(const htn_mps* const* others, int n) {
    if (be->activate()) return 1;
    if (n == 0) {
        orth_detach();
        return 0;
    }
    if (ctx->world > 1) return set_error("htn_mps_set_orthogonal: not available on a context with a communicator");
    std::vector<htn_mps*> list;
    for (int k = 0; k < n; ++k) {
        htn_mps* o = const_cast<htn_mps*>(others[k]);
        if (!o || o == this) return set_error("htn_mps_set_orthogonal: state %d is NULL or the state itself", k);
        if (o->ctx != ctx) return set_error("htn_mps_set_orthogonal: state %d lives in a different context", k);
        if (o->L != L) return set_error("htn_mps_set_orthogonal: state %d has %d sites, this state %d", k, o->L, L);
        const Sym &a = mpo->sym, &b = o->mpo->sym;
        bool same = a.kind == b.kind && a.n_site == b.n_site;
        for (int q = 0; same && q < a.n_site; ++q) same = a.site[q] == b.site[q];
        if (!same) return set_error("htn_mps_set_orthogonal: state %d has a different symmetry", k);
        if (o->bonds[0]->key != bonds[0]->key || o->bonds[o->L]->key != bonds[L]->key)
            return set_error("htn_mps_set_orthogonal: state %d is in a different total sector", k);
        if (bonds[0]->dim_full(a) != 1 || bonds[L]->secs.size() != 1 || bonds[L]->dims[0] != 1)
            return set_error("htn_mps_set_orthogonal: the end bonds must be single sectors of dimension 1 (a finite chain)");
        list.push_back(o);
    }
    return orth_attach(list.data(), n);
}

int htn_mps::overlap(const htn_mps* b, double* out_host) {
    if (ctx != b->ctx) return set_error("htn_mps_overlap: the states live in different contexts");
    if (L != b->L) return set_error("htn_mps_overlap: %d and %d sites", L, b->L);
    if (be->activate()) return 1;
    out_host[0] = out_host[1] = 0.0;
    if (bonds[0]->key != b->bonds[0]->key || bonds[L]->key != b->bonds[b->L]->key) return 0;      // different total sectors
    OvlLayoutP lay;
    DView buf;
    if (ovl_boundary(b, 0, &lay, &buf)) return 1;
    for (int i = 0; i < L; ++i) {
        OvlLayoutP nl;
        DView nb;
        if (ovl_step('L', b, i, lay, buf, &nl, &nb)) return 1;
        lay = nl;
        buf = nb;
    }
    if (lay->size != 1) return set_error("htn_mps_overlap: the right end bonds are not one sector of dimension 1");
    cplx v;
    if (be->download(&v, buf.ptr(), sizeof(v))) return 1;
    if (amp != 1.0 || b->amp != 1.0) v *= amp * b->amp;      // (states made by htn_mps_apply_op: htn_engine.h)
    out_host[0] = v.real();
    out_host[1] = v.imag();
    return 0;
}

// =====================================================================================================================
// Two-point correlation functions C(i, j) = <close_j . pass ... pass . open_i> of one channel for all i <= j, the state read only
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
// =====================================================================================================================
int htn_mps::correlator(const htn_corr_channel& ch, cplx* out_host, double* norm_host) {
    const Sym& sym = mpo->sym;
    const char* who = "htn_mps_correlator";
    if (ctx->world > 1 || ctx->shard || ctx->exch || be->has_comm())
        return set_error("%s: not available on a context with a communicator or an exchange hook", who);
    if (ch.open.dN + ch.close.dN != 0 || (sym.su2() ? ch.open.k != ch.close.k : ch.open.k + ch.close.k != 0))
        return set_error("%s: the charges of open (dN %d, k %d) and close (dN %d, k %d) do not add up to zero", who, ch.open.dN, ch.open.k,
                         ch.close.dN, ch.close.k);
    if (ch.pass.dN != 0 || ch.pass.k != 0) return set_error("%s: the pass operator carries a charge (dN %d, k %d)", who, ch.pass.dN, ch.pass.k);
    if (ch.has_onsite && (ch.onsite.dN != 0 || ch.onsite.k != 0))
        return set_error("%s: the onsite operator carries a charge (dN %d, k %d)", who, ch.onsite.dN, ch.onsite.k);
    if (Llay[0]->size != 0 || Rlay[L]->size != 0 || bonds[0]->multiplets() != 1 || bonds[L]->multiplets() != 1)
        return set_error("%s: needs a finite chain with open ends (end bonds of one sector, dimension 1)", who);

    // probe operators: 0 id, 1 open, 2 pass, 3 close, 4 onsite
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
    add_op(ident), add_op(ch.open), add_op(ch.pass), add_op(ch.close), add_op(ch.onsite);
    const bool onsite = ch.has_onsite != 0;
    const Lvl scalar{0, 0}, open{ch.open.dN, ch.open.k};
    const std::string tag((const char*)&ch, sizeof(ch));          // the probe's name in the plan cache: its operator tables
    auto bkey = [&](int i) { return bonds[i]->key + "|" + bonds[i + 1]->key; };

    // ---- left pass ----
    MpoSite WL;
    WL.left = {scalar, scalar};
    WL.right = {scalar, scalar, open};
    WL.entries = {{1, 1, 0, cplx(1.0)}, {1, 2, 1, cplx(1.0)}};
    if (onsite) {
        WL.right.push_back(scalar);
        WL.entries.push_back({1, 3, 4, cplx(1.0)});
    }
    std::vector<EnvLayoutP> Hlay(L + 1);
    std::vector<DView> Hbuf(L + 1);
    Hbuf[0] = zalloc(1, false);
    const cplx one(1.0, 0.0);
    if (!Hbuf[0].base || be->upload(Hbuf[0].ptr(), &one, sizeof(one))) return set_error("%s: device allocation failed", who);
    for (int i = 0; i < L; ++i) {
        const SiteLayoutP lay = site_layout('L', bonds[i], bonds[i + 1]);
        DView relaid;
        const cplx* site = site_buf[i].ptr();
        if (site_lay[i]->kind != 'L') {
            relaid = zalloc(lay->size, false);
            if (!relaid.base) return set_error("%s: device allocation failed", who);
            if (relay(*site_lay[i], site, *lay, relaid.ptr())) return 1;
            site = relaid.ptr();
        }
        auto c = cached<EnvC>("corrL" + tag + bkey(i), [&]() -> std::shared_ptr<EnvC> {
            auto e = std::make_shared<EnvC>();
            e->lay = build_env_layout(sym, 'L', bonds[i + 1], WL.right);
            EnvPlan p;
            plan_left_env(pm, *build_env_layout(sym, 'L', bonds[i], WL.left), *lay, WL, *e->lay, p);
            return compile2(e, p);
        });
        if (!c) return 1;
        DView z = zalloc(c->zsize, false), o = zalloc(c->lay->size, false);
        if (!z.base || !o.base) return set_error("%s: device allocation failed", who);
        if (gemm(c->d1, {{BUF_L, Hbuf[i].ptr()}, {BUF_S1, site}, {BUF_Z, z.ptr()}})) return 1;
        if (gemm(c->d2, {{BUF_S1, site}, {BUF_Z, z.ptr()}, {BUF_Y, o.ptr()}})) return 1;
        Hlay[i + 1] = c->lay;
        Hbuf[i + 1] = o;                            // kept until the right pass has met it: O(L chi^2) in all
    }

    // ---- right pass, meeting the left half on every bond ----
    DView table = zalloc((int64_t)L * L + 1, true);
    if (!table.base) return set_error("%s: device allocation failed", who);
    std::vector<Lvl> rlev = {scalar, scalar};                      // levels of the right half on bond b: [norm, open_b .., -]
    EnvLayoutP Rl = build_env_layout(sym, 'R', bonds[L], rlev);
    DView Rb = zalloc(1, false);
    if (!Rb.base || be->upload(Rb.ptr(), &one, sizeof(one))) return set_error("%s: device allocation failed", who);
    for (int b = L; b >= 1; --b) {
        const int i = b - 1, K = L - b + 1;                        // K levels: norm + one per closing site j >= b
        if (b < L) {                                               // the right half crosses site b: bond b + 1 -> bond b
            const SiteLayoutP lay = site_layout('R', bonds[b], bonds[b + 1]);
            DView relaid;
            const cplx* site = site_buf[b].ptr();
            if (site_lay[b]->kind != 'R') {
                relaid = zalloc(lay->size, false);
                if (!relaid.base) return set_error("%s: device allocation failed", who);
                if (relay(*site_lay[b], site, *lay, relaid.ptr())) return 1;
                site = relaid.ptr();
            }
            MpoSite WR;
            WR.right = rlev;
            rlev.insert(rlev.begin() + 1, open);
            WR.left = rlev;
            WR.entries = {{0, 0, 0, cplx(1.0)}, {1, 0, 3, cplx(1.0)}};
            for (int w = 1; w + 1 < (int)WR.right.size(); ++w) WR.entries.push_back({w + 1, w, 2, cplx(1.0)});
            auto c = cached<EnvC>("corrR" + tag + ikey("K", K) + bkey(b), [&]() -> std::shared_ptr<EnvC> {
                auto e = std::make_shared<EnvC>();
                e->lay = build_env_layout(sym, 'R', bonds[b], WR.left);
                EnvPlan p;
                plan_right_env(pm, *Rl, *lay, WR, *e->lay, p);
                return compile2(e, p);
            });
            if (!c) return 1;
            DView z = zalloc(c->zsize, false), o = zalloc(c->lay->size, false);
            if (!z.base || !o.base) return set_error("%s: device allocation failed", who);
            if (gemm(c->d1, {{BUF_R, Rb.ptr()}, {BUF_S1, site}, {BUF_Z, z.ptr()}})) return 1;
            if (gemm(c->d2, {{BUF_S1, site}, {BUF_Z, z.ptr()}, {BUF_Y, o.ptr()}})) return 1;
            Rl = c->lay;
            Rb = o;
        }
        // results of this bond: 0 = <psi|psi>, 1 = C(i, i), 1 + (j - i) = C(i, j)
        const EnvLayout& Ll = *Hlay[b];
        auto m = cached<MeetC>("corrM" + tag + ikey("K", K) + bonds[b]->key, [&]() -> std::shared_ptr<MeetC> {
            auto mc = std::make_shared<MeetC>();
            auto pair = [&](int wl, int wr, int out) {
                for (size_t q = 0; q < Ll.blocks.size(); ++q) {
                    const Key& k = Ll.bkeys[q];
                    if (k[2] != wl) continue;
                    const Sec bra{k[0], k[1]}, ket{k[3], k[4]};
                    const int rq = Rl->block(ket, wr, bra);
                    if (rq < 0) continue;
                    const auto &lb = Ll.blocks[q], &rb = Rl->blocks[rq];
                    htn_trdot_item it;
                    memset(&it, 0, sizeof(it));
                    it.a_off = lb.off, it.b_off = rb.off;
                    it.rows = lb.m, it.cols = lb.n, it.lda = lb.m, it.ldb = rb.m;
                    it.out = out;
                    it.w_re = (double)sym.qdim(bra) / (double)sym.qdim(ket);
                    mc->items.push_back(it);
                }
            };
            pair(1, 0, 0);
            if (onsite) pair(3, 0, 1);
            for (int j = b; j < L; ++j) pair(2, 1 + (j - b), 1 + (j - i));
            if (!(mc->items_dev = upload_vec(be, mc->items))) return nullptr;
            return mc;
        });
        if (!m) return 1;
        if (be->block_trdots(Hbuf[b].ptr(), Rb.ptr(), (const htn_trdot_item*)m->items_dev->p, m->items.data(), (int)m->items.size(),
                             table.ptr() + ((int64_t)i * L + i), K + 1))
            return 1;
        Hbuf[b] = DView();
    }
    std::vector<cplx> t((size_t)L * L + 1);
    if (be->download(t.data(), table.ptr(), sizeof(cplx) * t.size())) return 1;
    for (int i = 0; i < L; ++i) {
        const cplx nrm = t[(size_t)i * L + i];
        if (!(std::abs(nrm) > 0.0)) return set_error("%s: <psi|psi> = %g on bond %d", who, nrm.real(), i + 1);
        if (i == 0 && norm_host) *norm_host = nrm.real();
        for (int j = 0; j < L; ++j) out_host[(size_t)i * L + j] = j > i || (j == i && onsite) ? t[1 + (size_t)i * L + j] / nrm : cplx(0.0, 0.0);
    }
    return 0;
}

// =====================================================================================================================
// Correlation functions of two nearest-neighbour bond operators, C(i, j) = <close1_{j+1} close0_j . pass ... pass . open1_{i+1} open0_i>
// of one channel for all j >= i + 2, the state read only (htn_mps_correlator2).  The scheme of
// htn_mps::correlator with two more probe levels per end:
//   left probe, every site      left [-, norm, half]   right [-, norm, half, open]
//                                                      (norm -> norm, id) (norm -> half, open0) (half -> open, open1)
//   right probe, site b         right [norm, halfR, open_{b+1} .. open_{L-2}, -]   left [norm, halfR', open_b, open_{b+1} .. open_{L-2}, -]
//                                                      (norm <- norm, id) (halfR' <- norm, close1) (open_b <- halfR, close0)
//                                                      (open_j' <- open_j', pass)
// (n_close = 1: no halfR level, open_b <- norm by close0, j up to L - 1).  The left buffer of a bond lists its levels in
// order, so the output of site i, read with the first three levels, is the input of site i + 1 as it stands.  The open level
// that site i + 1 writes and the right half meet on bond b = i + 2 in one block_trdots launch with the block weight of the
// two-point function; its results go to row i of the device table, shifted by one element (the norm in the unused slot).
// =====================================================================================================================
int htn_mps::correlator2(const htn_corr_channel2& ch, cplx* out_host, double* norm_host) {
    const Sym& sym = mpo->sym;
    const char* who = "htn_mps_correlator2";
    if (ctx->world > 1 || ctx->shard || ctx->exch || be->has_comm())
        return set_error("%s: not available on a context with a communicator or an exchange hook", who);
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
    if (ch.pass.dN != 0 || ch.pass.k != 0) return set_error("%s: the pass operator carries a charge (dN %d, k %d)", who, ch.pass.dN, ch.pass.k);
    if (Llay[0]->size != 0 || Rlay[L]->size != 0 || bonds[0]->multiplets() != 1 || bonds[L]->multiplets() != 1)
        return set_error("%s: needs a finite chain with open ends (end bonds of one sector, dimension 1), not a window with boundary environments", who);

    // probe operators: 0 id, 1 open0, 2 open1, 3 pass, 4 close0, 5 close1
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
    add_op(ident), add_op(o0), add_op(o1), add_op(ch.pass), add_op(c0), add_op(c1);
    const Lvl scalar{0, 0}, half{o0.dN, o0.k}, open{ch.open_dN, ch.open_k};
    htn_corr_channel2 named = ch;                                  // the probe's name in the plan cache: its operator tables,
    named.pad = 0;                                                 // without the fields the pass does not read
    if (!two) memset(&named.close[1], 0, sizeof(named.close[1]));
    const std::string tag((const char*)&named, sizeof(named));
    auto bkey = [&](int i) { return bonds[i]->key + "|" + bonds[i + 1]->key; };
    const cplx one(1.0, 0.0);

    // ---- left pass ----
    MpoSite WL;
    WL.left = {scalar, scalar, half};
    WL.right = {scalar, scalar, half, open};
    WL.entries = {{1, 1, 0, cplx(1.0)}, {1, 2, 1, cplx(1.0)}, {2, 3, 2, cplx(1.0)}};
    std::vector<EnvLayoutP> Hlay(L + 1);
    std::vector<DView> Hbuf(L + 1);
    Hbuf[0] = zalloc(build_env_layout(sym, 'L', bonds[0], WL.left)->size, true);      // norm = 1 first, an empty half level (if it has a block)
    if (!Hbuf[0].base || be->upload(Hbuf[0].ptr(), &one, sizeof(one))) return set_error("%s: device allocation failed", who);
    for (int i = 0; i + ch.n_close < L; ++i) {                     // the last bond that is met is L - 1 (n_close = 1) or L - 2
        const SiteLayoutP lay = site_layout('L', bonds[i], bonds[i + 1]);
        DView relaid;
        const cplx* site = site_buf[i].ptr();
        if (site_lay[i]->kind != 'L') {
            relaid = zalloc(lay->size, false);
            if (!relaid.base) return set_error("%s: device allocation failed", who);
            if (relay(*site_lay[i], site, *lay, relaid.ptr())) return 1;
            site = relaid.ptr();
        }
        auto c = cached<EnvC>("corr2L" + tag + bkey(i), [&]() -> std::shared_ptr<EnvC> {
            auto e = std::make_shared<EnvC>();
            e->lay = build_env_layout(sym, 'L', bonds[i + 1], WL.right);
            EnvPlan p;
            plan_left_env(pm, *build_env_layout(sym, 'L', bonds[i], WL.left), *lay, WL, *e->lay, p);
            return compile2(e, p);
        });
        if (!c) return 1;
        DView z = zalloc(c->zsize, false), o = zalloc(c->lay->size, false);
        if (!z.base || !o.base) return set_error("%s: device allocation failed", who);
        if (gemm(c->d1, {{BUF_L, Hbuf[i].ptr()}, {BUF_S1, site}, {BUF_Z, z.ptr()}})) return 1;
        if (gemm(c->d2, {{BUF_S1, site}, {BUF_Z, z.ptr()}, {BUF_Y, o.ptr()}})) return 1;
        Hlay[i + 1] = c->lay;
        Hbuf[i + 1] = o;                            // kept until the right pass has met it: O(L chi^2) in all
    }

    // ---- right pass, meeting the left half on every bond b = i + 2 ----
    DView table = zalloc((int64_t)L * L + 1, true);
    if (!table.base) return set_error("%s: device allocation failed", who);
    std::vector<Lvl> rlev = {scalar, scalar};                      // levels of the right half on bond b: [norm, (halfR,) open_b .., -]
    EnvLayoutP Rl = build_env_layout(sym, 'R', bonds[L], rlev);
    DView Rb = zalloc(1, false);
    if (!Rb.base || be->upload(Rb.ptr(), &one, sizeof(one))) return set_error("%s: device allocation failed", who);
    const int first = two ? 2 : 1;                                 // index of open_b among the levels of bond b
    for (int b = L - 1; b >= 2; --b) {
        const int i = b - 2;
        {                                                          // the right half crosses site b: bond b + 1 -> bond b
            const SiteLayoutP lay = site_layout('R', bonds[b], bonds[b + 1]);
            DView relaid;
            const cplx* site = site_buf[b].ptr();
            if (site_lay[b]->kind != 'R') {
                relaid = zalloc(lay->size, false);
                if (!relaid.base) return set_error("%s: device allocation failed", who);
                if (relay(*site_lay[b], site, *lay, relaid.ptr())) return 1;
                site = relaid.ptr();
            }
            MpoSite WR;
            WR.right = rlev;
            WR.entries = {{0, 0, 0, cplx(1.0)}};
            if (!two) {
                rlev.insert(rlev.begin() + 1, open);
                WR.entries.push_back({1, 0, 4, cplx(1.0)});
            } else if (b == L - 1) {
                rlev.insert(rlev.begin() + 1, halfR);
                WR.entries.push_back({1, 0, 5, cplx(1.0)});
            } else {
                rlev.insert(rlev.begin() + 2, open);
                if (b > 2) WR.entries.push_back({1, 0, 5, cplx(1.0)});      // (the halfR level of bond 2 would be read by nothing)
                WR.entries.push_back({2, 1, 4, cplx(1.0)});
            }
            WR.left = rlev;
            for (int w = first; w + 1 < (int)WR.right.size(); ++w) WR.entries.push_back({w + 1, w, 3, cplx(1.0)});
            auto c = cached<EnvC>("corr2R" + tag + ikey("b", b) + bkey(b), [&]() -> std::shared_ptr<EnvC> {
                auto e = std::make_shared<EnvC>();
                e->lay = build_env_layout(sym, 'R', bonds[b], WR.left);
                EnvPlan p;
                plan_right_env(pm, *Rl, *lay, WR, *e->lay, p);
                return compile2(e, p);
            });
            if (!c) return 1;
            DView z = zalloc(c->zsize, false), o = zalloc(c->lay->size, false);
            if (!z.base || !o.base) return set_error("%s: device allocation failed", who);
            if (gemm(c->d1, {{BUF_R, Rb.ptr()}, {BUF_S1, site}, {BUF_Z, z.ptr()}})) return 1;
            if (gemm(c->d2, {{BUF_S1, site}, {BUF_Z, z.ptr()}, {BUF_Y, o.ptr()}})) return 1;
            Rl = c->lay;
            Rb = o;
        }
        const int n_open = (int)rlev.size() - 1 - first;           // closing sites j = b .. b + n_open - 1
        if (n_open <= 0) continue;                                 // (n_close = 2, b = L - 1: only the halfR level so far)
        // results of this bond: 0 = <psi|psi>, 1 + (j - i) = C(i, j)
        const EnvLayout& Ll = *Hlay[b];
        auto m = cached<MeetC>("corr2M" + tag + ikey("b", b) + bonds[b]->key, [&]() -> std::shared_ptr<MeetC> {
            auto mc = std::make_shared<MeetC>();
            auto pair = [&](int wl, int wr, int out) {
                for (size_t q = 0; q < Ll.blocks.size(); ++q) {
                    const Key& k = Ll.bkeys[q];
                    if (k[2] != wl) continue;
                    const Sec bra{k[0], k[1]}, ket{k[3], k[4]};
                    const int rq = Rl->block(ket, wr, bra);
                    if (rq < 0) continue;
                    const auto &lb = Ll.blocks[q], &rb = Rl->blocks[rq];
                    htn_trdot_item it;
                    memset(&it, 0, sizeof(it));
                    it.a_off = lb.off, it.b_off = rb.off;
                    it.rows = lb.m, it.cols = lb.n, it.lda = lb.m, it.ldb = rb.m;
                    it.out = out;
                    it.w_re = (double)sym.qdim(bra) / (double)sym.qdim(ket);
                    mc->items.push_back(it);
                }
            };
            pair(1, 0, 0);
            for (int j = b; j < b + n_open; ++j) pair(3, first + (j - b), 1 + (j - i));
            if (!(mc->items_dev = upload_vec(be, mc->items))) return nullptr;
            return mc;
        });
        if (!m) return 1;
        if (be->block_trdots(Hbuf[b].ptr(), Rb.ptr(), (const htn_trdot_item*)m->items_dev->p, m->items.data(), (int)m->items.size(),
                             table.ptr() + ((int64_t)i * L + i), L - i + 1))
            return 1;
        Hbuf[b] = DView();
    }
    std::vector<cplx> t((size_t)L * L + 1);
    if (be->download(t.data(), table.ptr(), sizeof(cplx) * t.size())) return 1;
    const int rows = two ? L - 3 : L - 2;                          // rows i that met a right half
    for (int i = 0; i < L; ++i) {
        const cplx nrm = i < rows ? t[(size_t)i * L + i] : one;
        if (!(std::abs(nrm) > 0.0)) return set_error("%s: <psi|psi> = %g on bond %d", who, nrm.real(), i + 2);
        if (i == 0 && norm_host) *norm_host = nrm.real();
        for (int j = 0; j < L; ++j) out_host[(size_t)i * L + j] = i < rows && j >= i + 2 ? t[1 + (size_t)i * L + j] / nrm : cplx(0.0, 0.0);
    }
    return 0;
}
