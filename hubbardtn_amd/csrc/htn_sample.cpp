// Perfect sampling of a finite MPS (htn_mps_sample; Ferris, Vidal, Phys. Rev. B 85, 165146).  Host C++ (no
// HIP): the planner below writes the per-site item lists of Backend::sample_step from the stored site layouts; the device work is
// one sample_step per site and batch.
// NOT a translation unit of its own: #included by htn_engine.cpp (one unit, see its head); never name it on a build line.
//
// With the centre on site 0 and every other site right-canonical, the probability of the multiplets s_0 .. s_i (everything to
// the right traced) is a plain sum over the paths of sectors of |A_0[(c_0, s_0); c_1] .. A_i[(c_i, s_i); c_{i+1}]|_F^2: the
// left-coupled basis states of different paths or site multiplets are orthonormal, the stored ("tilde") blocks carry
// sqrt(2J + 1) along every path in all (ovl_step's note in htn_overlap.cpp), and the right tensors have orthonormal rows in the
// plain sense, so the right norm environment a level closes against is the identity with weight 1 in every sector.  The
// coefficient of a sub-block is what plan_left_env gives the identity between two scalar levels, coef_left(l, 0, l, s, s, 0, r,
// 0, r): it evaluates to 1 in all three kinds and is taken from there, not assumed.  So per sample a density matrix rho with one
// block per sector of the current bond, trace 1, and per site T_s = rho_l A, p(s) = sum Re<A, T_s>, rho'_r = sum_l A^H T_{s*} / p(s*).
#include "htn_engine.h"

namespace {

struct SampC {                     // the items of one site and their device copy
    std::vector<htn_sample_item> items;
    DBufP items_dev;
    int64_t rho_stride = 0, next_stride = 0, t_stride = 0;
    bool uncovered = false;        // a sector of the right bond no sub-block ends in: the next rho is zeroed before the step
};

// offsets of the per-sector blocks of a density matrix on `bond` (sector order, n_c x n_c each) -> elements in all
int64_t rho_offsets(const Bond& bond, std::vector<int64_t>& off) {
    off.resize(bond.secs.size());
    int64_t pos = 0;
    for (size_t k = 0; k < bond.secs.size(); ++k) {
        off[k] = pos;
        pos += (int64_t)bond.dims[k] * bond.dims[k];
    }
    return pos;
}

std::shared_ptr<SampC> samp_plan(htn_mps* m, int i) {
    const SiteLayout& lay = *m->site_lay[i];
    return m->cached<SampC>(std::string("smp") + lay.kind + m->bonds[i]->key + "|" + m->bonds[i + 1]->key, [&]() -> std::shared_ptr<SampC> {
        const Sym& sym = m->mpo->sym;
        auto c = std::make_shared<SampC>();
        std::vector<int64_t> loff, roff;
        c->rho_stride = rho_offsets(*lay.bl, loff);
        c->next_stride = rho_offsets(*lay.br, roff);
        struct Ref {
            int r, s, l, blk;
        };
        std::vector<Ref> refs;
        for (size_t bi = 0; bi < lay.blocks.size(); ++bi) {
            const Key& k = lay.bkeys[bi];
            const int l = lay.bl->find(Sec{k[0], k[1]}), r = lay.br->find(Sec{k[3], k[4]});
            if (l < 0 || r < 0 || lay.blocks[bi].m < 1 || lay.blocks[bi].n < 1) continue;
            refs.push_back({r, k[2], l, (int)bi});
        }
        std::sort(refs.begin(), refs.end(), [](const Ref& a, const Ref& b) {
            return a.r != b.r ? a.r < b.r : (a.s != b.s ? a.s < b.s : a.l < b.l);
        });
        if (refs.empty()) {
            set_error("htn_mps_sample: site %d has no sub-block", i);
            return nullptr;
        }
        std::vector<char> covered(lay.br->secs.size(), 0);
        int64_t pu = 0, cu = 0, run_units = 0;
        for (size_t q = 0; q < refs.size(); ++q) {
            const Ref& f = refs[q];
            const BlockRec& b = lay.blocks[f.blk];
            const Sec lsec = lay.bl->secs[f.l], rsec = lay.br->secs[f.r];
            const int js = sym.jeff(sym.site[f.s].j);
            htn_sample_item it;
            memset(&it, 0, sizeof(it));
            it.rho_off = loff[f.l], it.a_off = b.off, it.t_off = c->t_stride, it.out_off = roff[f.r];
            it.n_l = b.m, it.n_r = b.n, it.lda = b.ld, it.s = f.s;
            it.coef = coef_left(sym.jeff(lsec.j), 0, sym.jeff(lsec.j), js, js, 0, sym.jeff(rsec.j), 0, sym.jeff(rsec.j));
            const bool first = q == 0 || refs[q - 1].r != f.r;
            if (first) cu += run_units, run_units = HTN_SAMPLE_UNITS(b.n, b.n);
            it.probe_unit0 = (int32_t)pu;
            it.close_unit0 = (int32_t)(first ? cu : cu + run_units);
            pu += HTN_SAMPLE_UNITS(b.m, b.n);
            c->t_stride += (int64_t)b.m * b.n;
            covered[f.r] = 1;
            if (pu > INT32_MAX / 2 || cu + run_units > INT32_MAX / 2) {
                set_error("htn_mps_sample: too many work units on site %d", i);
                return nullptr;
            }
            c->items.push_back(it);
        }
        for (char v : covered) c->uncovered = c->uncovered || !v;
        if (!(c->items_dev = upload_vec(m->be, c->items))) return nullptr;
        return c;
    });
}

}  // namespace

int htn_mps::sample(int32_t n_samples, const double* u_host, const int32_t* measure_host, int32_t batch, int32_t* out_host, double* logp_host,
                    double* split_host) {
    const char* who = "htn_mps_sample";
    if (ctx->world > 1 || ctx->shard || ctx->exch || be->has_comm())
        return set_error("%s: not available on a context with a communicator or an exchange hook", who);
    if (!orth.empty()) return set_error("%s: not available for a state with attached orthogonal states", who);
    if (Llay[0]->size != 0 || Rlay[L]->size != 0) return set_error("%s: needs a finite chain with open ends (no boundary environments)", who);
    if (bonds[0]->multiplets() != 1 || bonds[0]->dim_full(mpo->sym) != 1)
        return set_error("%s: the left end bond must be one sector of dimension 1 (a finite chain)", who);
    if (centre != 0) return set_error("%s: the centre is on site %d, not on site 0", who, centre);
    for (int i = 1; i < L; ++i)
        if (site_lay[i]->kind != 'R') return set_error("%s: site %d is not in right layout (the centre is on site 0)", who, i);
    if (raw_n2 == 0.0) return set_error("%s: the state has norm 0", who);
    if (n_samples < 0) return set_error("%s: negative number of samples", who);
    if (n_samples == 0) return 0;
    if (batch <= 0) batch = 256;
    batch = std::min(std::min(batch, n_samples), 65535);

    double t0 = now(), t_plan = 0.0;
    std::vector<std::shared_ptr<SampC>> plans((size_t)L);
    int64_t max_rho = 1, max_t = 1;
    for (int i = 0; i < L; ++i) {
        if (!(plans[i] = samp_plan(this, i))) return 1;
        max_rho = std::max(max_rho, std::max(plans[i]->rho_stride, plans[i]->next_stride));
        max_t = std::max(max_t, plans[i]->t_stride);
    }
    t_plan = now() - t0;
    t0 = now();
    DView rho[2] = {zalloc(max_rho * batch, false), zalloc(max_rho * batch, false)};
    DView T = zalloc(max_t * batch, false);
    DBufP ud = dalloc(sizeof(double) * (size_t)L * batch), cd = dalloc(sizeof(int32_t) * (size_t)L * batch), ld = dalloc(sizeof(double) * batch);
    if (!rho[0].base || !rho[1].base || !T.base || !ud || !cd || !ld) return set_error("%s: device allocation failed", who);
    std::vector<double> ut((size_t)L * batch);
    std::vector<int32_t> ch((size_t)L * batch);
    const std::vector<cplx> ones((size_t)batch, cplx(1.0, 0.0));
    for (int32_t b0 = 0; b0 < n_samples; b0 += batch) {
        const int nb = std::min(batch, n_samples - b0);
        for (int i = 0; i < L; ++i)
            for (int b = 0; b < nb; ++b) ut[(size_t)i * nb + b] = u_host[(size_t)(b0 + b) * L + i];
        if (be->upload(ud->p, ut.data(), sizeof(double) * (size_t)L * nb) || be->upload(rho[0].ptr(), ones.data(), sizeof(cplx) * nb) ||
            be->zero(ld->p, sizeof(double) * nb))
            return 1;
        for (int i = 0; i < L; ++i) {
            const SampC& c = *plans[i];
            const DView &in = rho[i & 1], &out = rho[(i + 1) & 1];
            if (c.uncovered && be->zero(out.ptr(), sizeof(cplx) * (size_t)(c.next_stride * nb))) return 1;
            if (be->sample_step(out.ptr(), in.ptr(), site_buf[i].ptr(), T.ptr(), (const htn_sample_item*)c.items_dev->p, c.items.data(),
                                (int)c.items.size(), mpo->sym.n_site, nb, c.rho_stride, c.next_stride, c.t_stride, (const double*)ud->p + (size_t)i * nb,
                                measure_host ? (measure_host[i] != 0) : 1, (int32_t*)cd->p + (size_t)i * nb, (double*)ld->p))
                return 1;
        }
        if (be->download(ch.data(), cd->p, sizeof(int32_t) * (size_t)L * nb) || be->download(logp_host + b0, ld->p, sizeof(double) * nb)) return 1;
        for (int b = 0; b < nb; ++b)
            for (int i = 0; i < L; ++i) out_host[(size_t)(b0 + b) * L + i] = ch[(size_t)i * nb + b];
    }
    if (split_host) split_host[0] = t_plan, split_host[1] = now() - t0;
    return 0;
}
