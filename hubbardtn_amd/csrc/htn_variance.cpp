// Two-site energy variance of a finite MPS (htn_mps_variance; Hubig, Haegeman, Schollwoeck, Phys. Rev. B 97, 045125; DESIGN.md
// section 4d).  Host C++ (no HIP): the planner below writes the per-bond item lists of Backend::block_nullproj from the theta
// layout and the site layouts; the device work is the engine's own theta formation and H_eff applies, the non-optimising bond
// moves, and the projection launches.
// NOT a translation unit of its own: #included by htn_engine.cpp (one unit, see its head); never name it on a build line.
//
// With the centre on site i as M_i (theta = M_i B_{i+1}, y = H_eff2 theta, both in the theta layout: per mid sector c one matrix
// with rows (a, s1) and columns (s2, b)) the rows of sector c are the rows of the left-layout matrix of A_i for right sector c,
// in the same order, and its columns are the columns of the right-layout matrix of B_{i+1} for left sector c (the layouts sort
// their groups alike; plan_finalize relies on the same fact).  In the tilde normalisation A_i has orthonormal columns and B_{i+1}
// orthonormal rows in the plain sense, and the norm of the state is the plain norm of theta, so per sector
//   y <- (1 - A A^H) y           (side 0; the coefficients removed are not needed)
//   y <- y - (y B^H) B           (side 1; |y B^H|^2 = site[i], the left-null part of H_eff1(M_i); |y|^2 afterwards = bond[i])
// without a sector weight.  A_i is the isometry the non-optimising move of bond i leaves on site i; B_{i+1} is the tensor that
// was stored there before that move (its buffer is kept alive until the bond is done).
#include "htn_engine.h"

namespace {

struct VarC {                      // the projection items of one launch and their device copy
    std::vector<htn_nullproj_item> items;
    DBufP items_dev;
};

htn_nullproj_item var_item(int64_t r_off, int32_t m, int32_t n, int32_t ldr, int64_t q_off, int32_t k, int32_t ldq, int32_t side) {
    htn_nullproj_item it;
    memset(&it, 0, sizeof(it));
    it.r_off = r_off, it.q_off = q_off, it.m = m, it.n = n, it.k = k, it.ldr = ldr, it.ldq = std::max(ldq, 1), it.side = side, it.out = 0;
    return it;
}

// side 0: Q = the left-layout matrices of `lay` (rows x k per right sector c); side 1: the right-layout matrices (k x cols per left
// sector c); lay == nullptr: no isometry at all (k = 0: the norm of the blocks).  A sector the site does not hold gets k = 0.
std::shared_ptr<VarC> var_plan(htn_mps* m, const char* tag, const ThetaLayout& tl, const SiteLayout* lay, int side) {
    std::string key = std::string(tag) + tl.bl->key + "|" + tl.br->key;
    if (lay) key += "|" + (side == 0 ? lay->br->key : lay->bl->key);
    return m->cached<VarC>(key, [&]() -> std::shared_ptr<VarC> {
        auto v = std::make_shared<VarC>();
        for (const auto& M : tl.mats) {
            int64_t q_off = 0;
            int32_t k = 0, ldq = 1;
            const int qi = lay ? lay->mat(M.c) : -1;
            if (qi >= 0) {
                const SiteLayout::Mat& Qm = lay->mats[qi];
                if (side == 0 ? Qm.rows != M.rows : Qm.cols != M.cols) {
                    set_error("htn_mps_variance: internal error (sector (%d, %d): the site matrix is %d x %d, the block %d x %d)", M.c.N, M.c.j,
                              Qm.rows, Qm.cols, M.rows, M.cols);
                    return nullptr;
                }
                q_off = Qm.off, k = side == 0 ? Qm.cols : Qm.rows, ldq = Qm.rows;
            }
            v->items.push_back(var_item(M.off, M.rows, M.cols, M.rows, q_off, k, ldq, side));
        }
        if (!(v->items_dev = upload_vec(m->be, v->items))) return nullptr;
        return v;
    });
}
int var_run(htn_mps* m, const VarC& v, cplx* R, const cplx* Q, double* out) {
    return m->be->block_nullproj(R, Q, (const htn_nullproj_item*)v.items_dev->p, v.items.data(), (int)v.items.size(), out, 1);
}

}  // namespace

int htn_mps::variance(double* site_host, double* bond_host, double* energy_host, double* split_host) {
    const char* who = "htn_mps_variance";
    if (ctx->world > 1 || ctx->shard || ctx->exch || be->has_comm())
        return set_error("%s: not available on a context with a communicator or an exchange hook", who);
    if (!orth.empty()) return set_error("%s: not available for a state with attached orthogonal states", who);
    if (L < 2) return set_error("%s: a chain of %d site(s) has no bond", who, L);
    if (Llay[0]->size != 0 || Rlay[L]->size != 0) return set_error("%s: needs a finite chain with open ends (no boundary environments)", who);
    for (int i = 0; i < L; ++i)
        if (i != centre && site_lay[i]->kind != (i < centre ? 'L' : 'R'))
            return set_error("%s: site %d is not in %s layout (the centre is on site %d)", who, i, i < centre ? "left" : "right", centre);
    if (raw_n2 == 0.0) return set_error("%s: the state has norm 0", who);
    // The moves never write into a buffer the state holds: every update installs fresh ones.  So the state as it stands is kept
    // by its handles (layouts and device buffers, reference counted) and put back on every return, errors included: the caller's
    // state is bit for bit what it was, centre, norm factor, stored energy, spectra and hints with it, and the centre need not
    // be carried back by moves.  Only the plan cache grows.
    struct Keep {
        htn_mps* m;
        std::vector<BondP> bonds;
        std::vector<SiteLayoutP> site_lay;
        std::vector<DView> site_buf, Lbuf, Rbuf;
        std::vector<EnvLayoutP> Llay, Rlay;
        int centre, orth_dropped;
        double amp, raw_n2, energy;
        std::map<int, Spectrum> spectra;
        std::map<int, std::pair<std::pair<int, double>, double>> cut_hint;
        std::map<int, int> sweeps_hint;
        ~Keep() {
            m->bonds.swap(bonds), m->site_lay.swap(site_lay), m->site_buf.swap(site_buf), m->Lbuf.swap(Lbuf), m->Rbuf.swap(Rbuf);
            m->Llay.swap(Llay), m->Rlay.swap(Rlay);
            m->centre = centre, m->orth_dropped = orth_dropped, m->amp = amp, m->raw_n2 = raw_n2, m->energy = energy;
            m->spectra.swap(spectra), m->cut_hint.swap(cut_hint), m->sweeps_hint.swap(sweeps_hint);
        }
    } keep{this, bonds, site_lay, site_buf, Lbuf, Rbuf, Llay, Rlay, centre, orth_dropped, amp, raw_n2, energy, spectra, cut_hint, sweeps_hint};
    const htn_sweep_opts o = norm_opts(nullptr);        // no dimension limit, no cutoff: only the relative floor of `truncate` cuts
    double t_apply = 0.0, t_proj = 0.0, t_move = 0.0, t_last = now();
    auto lap = [&](double& acc) {
        if (!split_host) return;
        be->sync();
        const double t = now();
        acc += t - t_last;
        t_last = t;
    };
    for (int i = centre - 1; i >= 0; --i)
        if (update_bond(i, -1, false, false, o, nullptr)) return 1;
    lap(t_move);
    // results on the device: (site[i], bond[i]) for i < L - 1, (., site[L - 1]), a pair nobody reads, (., |theta_0|^2)
    const int n_res = 2 * L + 4;
    DBufP res = dalloc(sizeof(double) * (size_t)n_res);
    if (!res || be->zero(res->p, sizeof(double) * (size_t)n_res)) return set_error("%s: device allocation failed", who);
    double* resd = (double*)res->p;
    double E = 0.0;
    for (int i = 0; i + 1 < L; ++i) {
        ThetaLayoutP tl = theta_layout(bonds[i], bonds[i + 2]);
        const int64_t n = tl->size;
        if (n <= 0) return set_error("%s: empty two-site tensor on bond %d", who, i);
        auto ap = make_apply(i, *tl);
        if (!ap) return 1;
        DView th = zalloc(n, false), y = zalloc(n, true), z = zalloc(ap->zsize, false);
        if (!th.base || !y.base || !z.base) return set_error("%s: device allocation failed", who);
        if (theta_into(i, *tl, th.ptr())) return 1;
        if (ap->has_z && gemm(ap->dz, {{BUF_X, th.ptr()}, {BUF_L, Lbuf[i].ptr()}, {BUF_Z, z.ptr()}})) return 1;
        if (gemm(ap->dy, {{BUF_X, th.ptr()}, {BUF_Y, y.ptr()}, {BUF_L, Lbuf[i].ptr()}, {BUF_R, Rbuf[i + 2].ptr()}, {BUF_Z, z.ptr()}})) return 1;
        lap(t_apply);
        if (i == 0) {              // a state that no update has normalised yet (an applied state, an upload): its norm
            auto vn = var_plan(this, "varN", *tl, nullptr, 0);
            if (!vn || var_run(this, *vn, th.ptr(), nullptr, resd + 2 * L + 2)) return 1;
            lap(t_proj);
        }
        const SiteLayoutP b_lay = site_lay[i + 1];
        const DView b_buf = site_buf[i + 1];             // B_{i+1} as stored: the move replaces it by the next centre
        if (update_bond(i, +1, true, false, o, nullptr)) return 1;
        E = energy;
        lap(t_move);
        auto va = var_plan(this, "varA", *tl, site_lay[i].get(), 0), vb = var_plan(this, "varB", *tl, b_lay.get(), 1);
        if (!va || !vb) return 1;
        if (var_run(this, *va, y.ptr(), site_buf[i].ptr(), resd + 2 * L)) return 1;
        if (var_run(this, *vb, y.ptr(), b_buf.ptr(), resd + 2 * i)) return 1;
        lap(t_proj);
    }
    {       // last site: r = H_eff1(M) - <M|H_eff1(M)> M by the same projection with Q = M as one column (the moves normalised M)
        const int i = L - 1;
        const SiteLayout& lay = *site_lay[i];
        const int64_t n = lay.size;
        if (n <= 0 || n > INT32_MAX) return set_error("%s: the last site tensor has %lld elements", who, (long long)n);
        auto ap = make_apply1(i, lay);
        if (!ap) return 1;
        DView y = zalloc(n, true), z = zalloc(ap->zsize, false);
        if (!y.base || !z.base) return set_error("%s: device allocation failed", who);
        const cplx* x = site_buf[i].ptr();
        if (ap->has_z && gemm(ap->dz, {{BUF_X, x}, {BUF_L, Lbuf[i].ptr()}, {BUF_Z, z.ptr()}})) return 1;
        if (gemm(ap->dy, {{BUF_X, x}, {BUF_Y, y.ptr()}, {BUF_L, Lbuf[i].ptr()}, {BUF_R, Rbuf[i + 1].ptr()}, {BUF_Z, z.ptr()}})) return 1;
        lap(t_apply);
        auto v1 = cached<VarC>(std::string("var1") + lay.kind + lay.bl->key + "|" + lay.br->key, [&]() -> std::shared_ptr<VarC> {
            auto v = std::make_shared<VarC>();
            v->items.push_back(var_item(0, (int32_t)n, 1, (int32_t)n, 0, 1, (int32_t)n, 0));
            if (!(v->items_dev = upload_vec(be, v->items))) return nullptr;
            return v;
        });
        if (!v1 || var_run(this, *v1, y.ptr(), x, resd + 2 * i)) return 1;
        lap(t_proj);
    }
    std::vector<double> h((size_t)n_res);
    if (be->download(h.data(), res->p, sizeof(double) * h.size())) return 1;      // (the one download of the call)
    const double n2 = h[(size_t)(2 * L + 3)];
    if (!(n2 > 0.0)) return set_error("%s: the state has norm 0 (or is not finite)", who);
    for (int i = 0; i + 1 < L; ++i) {
        const double f = i == 0 ? 1.0 / n2 : 1.0;
        if (site_host) site_host[i] = h[(size_t)(2 * i)] * f;
        if (bond_host) bond_host[i] = h[(size_t)(2 * i + 1)] * f;
    }
    if (site_host) site_host[L - 1] = h[(size_t)(2 * (L - 1) + 1)];
    if (energy_host) *energy_host = E;
    if (split_host) split_host[0] = t_apply, split_host[1] = t_proj, split_host[2] = t_move;
    return 0;
}
