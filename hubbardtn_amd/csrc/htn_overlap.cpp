// Overlaps of an htn_mps (htn_engine.h): overlap environments <psi|phi>, the states attached to an orthogonalised sweep
// (htn_mps_set_orthogonal, htn_mps_overlap).  Correlation functions: htn_correlator.cpp.
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
