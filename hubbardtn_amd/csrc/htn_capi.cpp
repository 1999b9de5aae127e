// The C entry points of the bond-update / sweep level and of the IDMRG2 driver, grouped and ordered as the sections of
// include/hubbardtn_hip.h.  Argument checks and forwarding; what an entry does lives with the htn_mps members it calls
// (htn_engine.cpp, htn_site.cpp, htn_overlap.cpp, htn_correlator.cpp, htn_applyop.cpp, htn_variance.cpp, htn_sample.cpp,
// htn_idmrg.cpp).  The kernel-level entries that the CPU baseline library
// exports too (htn_krylov_expm_z, htn_krylov_solve_z, htn_qr_blocks_z, htn_block_nullproj_z) are in htn_backend_host.cpp.  Host C++ (no HIP).
// NOT a translation unit of its own: #included by htn_engine.cpp (one unit, see its head); never name it on a build line.
#include "htn_engine.h"

extern "C" {

const char* htn_last_error(void) { return err_buf(); }
int htn_abi_version(void) { return HTN_ABI_VERSION; }

// ---- contexts ------------------------------------------------------------------------------------------------------
int htn_ctx_create(int32_t backend, int32_t device, void* stream, htn_ctx** out) {
    if (!out) return set_error("htn_ctx_create: out is NULL");
    Backend* be = make_backend(backend, device, stream);
    if (!be) return 1;
    htn_ctx* c = new htn_ctx();
    c->be.reset(be);
    *out = c;
    return 0;
}
void htn_ctx_destroy(htn_ctx* ctx) { ctx_release(ctx); }
int htn_ctx_backend(const htn_ctx* ctx) { return ctx->be->kind(); }
int htn_ctx_set_timing(htn_ctx* ctx, int32_t on) {
    ctx->be->timing = on != 0;
    return 0;
}
int htn_ctx_set_comm(htn_ctx* ctx, int32_t rank, int32_t world, const void* id_host) {
    if (world < 1 || rank < 0 || rank >= world) return set_error("htn_ctx_set_comm: bad rank %d / world %d", rank, world);
    if (ctx->be->activate()) return 1;
    if (ctx->be->set_comm(rank, world, id_host)) return 1;
    ctx->rank = rank;
    ctx->world = world;
    ctx->shard = true;
    ctx->exch = nullptr;
    return 0;
}
int htn_ctx_set_exchange(htn_ctx* ctx, int32_t rank, int32_t world, htn_exchange2_fn fn, void* user) {
    if (world < 1 || rank < 0 || rank >= world) return set_error("htn_ctx_set_exchange: bad rank %d / world %d", rank, world);
    ctx->rank = rank;
    ctx->world = world;
    ctx->exch = fn;
    ctx->exch_user = user;
    ctx->shard = fn != nullptr;
    return 0;
}

// ---- MPO and state handles -----------------------------------------------------------------------------------------
int htn_mpo_create(htn_ctx* ctx, const htn_symmetry* sym, int32_t nsites, const htn_site_op* ops, int32_t n_ops,
                   const int32_t* level_ptr, const int32_t* levels, const int32_t* entry_ptr, const htn_mpo_entry* entries,
                   htn_mpo** out) {
    if (!ctx || !sym || !out || nsites < 2) return set_error("htn_mpo_create: bad arguments");
    if (sym->n_site < 1 || sym->n_site > HTN_MAX_SITE || sym->kind < 0 || sym->kind > 2) return set_error("htn_mpo_create: bad symmetry");
    auto m = std::make_unique<htn_mpo>();
    m->ctx = ctx;
    m->mpo.sym.kind = sym->kind;
    m->mpo.sym.n_site = sym->n_site;
    for (int s = 0; s < sym->n_site; ++s) m->mpo.sym.site[s] = {sym->site_N[s], sym->site_j[s]};
    for (int k = 0; k < n_ops; ++k) {
        SiteOp o;
        o.k = ops[k].k;
        o.dN = ops[k].dN;
        for (int a = 0; a < HTN_MAX_SITE; ++a)
            for (int b = 0; b < HTN_MAX_SITE; ++b) o.red[a][b] = ops[k].red[a * HTN_MAX_SITE + b];
        m->mpo.ops.push_back(o);
    }
    auto lv = [&](int b) {
        std::vector<Lvl> v;
        for (int q = level_ptr[b]; q < level_ptr[b + 1]; ++q) v.push_back({levels[2 * q], levels[2 * q + 1]});
        return v;
    };
    for (int i = 0; i < nsites; ++i) {
        MpoSite s;
        s.left = lv(i);
        s.right = lv(i + 1);
        if (s.left.empty() || s.right.empty()) return set_error("htn_mpo_create: site %d has an empty MPO bond", i);
        for (int q = entry_ptr[i]; q < entry_ptr[i + 1]; ++q) {
            const htn_mpo_entry& e = entries[q];
            if (e.wl < 0 || e.wl >= (int)s.left.size() || e.wr < 0 || e.wr >= (int)s.right.size() || e.op < 0 || e.op >= n_ops)
                return set_error("htn_mpo_create: entry %d of site %d out of range", q - entry_ptr[i], i);
            s.entries.push_back({e.wl, e.wr, e.op, cplx(e.coef_re, e.coef_im)});
        }
        s.key.append((const char*)s.left.data(), sizeof(Lvl) * s.left.size());
        s.key.append("|");
        s.key.append((const char*)s.right.data(), sizeof(Lvl) * s.right.size());
        s.key.append("|");
        for (auto& e : s.entries) {
            int32_t r[3] = {e.wl, e.wr, e.op};
            double c[2] = {e.coef.real(), e.coef.imag()};
            s.key.append((const char*)r, sizeof(r));
            s.key.append((const char*)c, sizeof(c));
        }
        m->mpo.sites.push_back(std::move(s));
    }
    // (a window inside a larger system (iDMRG) has full-width boundary bonds: allowed, the boundary environments then must be
    // supplied to htn_mps_create)
    ++ctx->refs;
    *out = m.release();
    return 0;
}
void htn_mpo_destroy(htn_mpo* mpo) { mpo_release(mpo); }

int htn_mps_create(htn_ctx* ctx, const htn_mpo* mpo, int32_t nsites, const int32_t* bond_ptr, const htn_sector* sectors,
                   const int32_t* sub_ptr, const htn_subblock* subs, const int64_t* data_ptr, const void* data_host,
                   const void* left_env_host, const void* right_env_host, htn_mps** out) {
    if (!ctx || !mpo || !out) return set_error("htn_mps_create: NULL argument");
    if (nsites != (int)mpo->mpo.sites.size()) return set_error("htn_mps_create: %d sites but the MPO has %d", nsites, (int)mpo->mpo.sites.size());
    if (ctx->be->activate()) return 1;
    // (errors below return through the guard: it drops the references the half-built object took)
    MpsGuard guard{mps_new(ctx, mpo)};
    htn_mps* e = guard.p;
    if (mps_load_bonds(e, bond_ptr, sectors) || mps_load_sites(e, sub_ptr, subs, data_ptr, data_host)) return 1;
    if (mps_finish(e, left_env_host, right_env_host, nullptr, nullptr)) return 1;
    guard.p = nullptr;
    *out = e;
    return 0;
}
void htn_mps_destroy(htn_mps* mps) {
    if (!mps || --mps->refs > 0) return;
    htn_ctx* c = mps->ctx;
    htn_mpo* m = mps->mpo_handle;
    if (mps->be) (void)mps->be->activate();
    mps->orth_detach();      // references to attached states
    delete mps;              // device buffers go back to the backend's pool first ...
    mpo_release(m);          // ... then the references that kept the backend alive
    ctx_release(c);
}

// ---- two-site updates and sweeps -----------------------------------------------------------------------------------
int htn_bond_update(htn_mps* mps, int32_t i, int32_t direction, int32_t placement, int32_t optimise, const htn_sweep_opts* opts,
                    htn_bond_stats* stats) {
    if (mps->be->activate()) return 1;
    return mps->update_bond(i, direction, placement == 0, optimise != 0, norm_opts(opts), stats);
}
int htn_dmrg2_sweep(htn_mps* mps, const htn_sweep_opts* opts, htn_bond_stats* stats, double* energy) {
    if (mps->be->activate()) return 1;
    return mps->sweep(norm_opts(opts), stats, energy);
}

// ---- one-site updates and sweeps -----------------------------------------------------------------------------------
int htn_site_update(htn_mps* mps, int32_t i, int32_t direction, int32_t optimise, const htn_sweep_opts* opts, htn_bond_stats* stats) {
    if (!mps) return set_error("htn_site_update: bad arguments");
    if (mps->be->activate()) return 1;
    return mps->update_site(i, direction, optimise != 0, norm_opts(opts), stats);
}
int htn_dmrg1_sweep(htn_mps* mps, const htn_sweep_opts* opts, htn_bond_stats* stats, double* energy) {
    if (!mps) return set_error("htn_dmrg1_sweep: bad arguments");
    if (mps->be->activate()) return 1;
    return mps->sweep1(norm_opts(opts), stats, energy);
}
int32_t htn_mps_centre(const htn_mps* mps) { return mps->centre; }
int64_t htn_mps_site_theta_size(htn_mps* mps, int32_t i) {
    if (i < 0 || i >= mps->L) return -1;
    return mps->site_lay[i]->size;
}
int htn_heff1_apply(htn_mps* mps, int32_t i, const void* x_host, void* y_host) {
    if (!mps || !x_host || !y_host) return set_error("htn_heff1_apply: bad arguments");
    if (site1_checks(mps, i, "htn_heff1_apply")) return 1;
    if (mps->be->activate()) return 1;
    const SiteLayout& lay = *mps->site_lay[i];
    auto ap = mps->make_apply1(i, lay);
    if (!ap) return 1;
    return mps->apply_once(*ap, mps->Lbuf[i], mps->Rbuf[i + 1], lay.size, x_host, y_host, false);
}

// ---- time evolution ------------------------------------------------------------------------------------------------
int htn_bond_evolve(htn_mps* mps, int32_t i, int32_t direction, int32_t placement, double dt_re, double dt_im, const htn_sweep_opts* opts,
                    htn_bond_stats* stats) {
    if (!mps) return set_error("htn_bond_evolve: bad arguments");
    if (mps->be->activate()) return 1;
    const htn_sweep_opts o = norm_opts(opts);
    if (mps->evolve_checks(o, "htn_bond_evolve")) return 1;
    const cplx dt(dt_re, dt_im);
    return mps->update_bond(i, direction, placement == 0, true, o, stats, &dt, nullptr);
}
int htn_site_evolve(htn_mps* mps, int32_t i, double dt_re, double dt_im, const htn_sweep_opts* opts, htn_bond_stats* stats) {
    if (!mps) return set_error("htn_site_evolve: bad arguments");
    if (mps->be->activate()) return 1;
    return mps->evolve_site(i, cplx(dt_re, dt_im), norm_opts(opts), stats, nullptr);
}
int htn_tdvp2_sweep(htn_mps* mps, double dt_re, double dt_im, const htn_sweep_opts* opts, htn_bond_stats* stats, double* energy,
                    double* log_norm) {
    if (!mps) return set_error("htn_tdvp2_sweep: bad arguments");
    if (mps->be->activate()) return 1;
    return mps->tdvp2_sweep(cplx(dt_re, dt_im), norm_opts(opts), stats, energy, log_norm);
}
int htn_site_evolve_move(htn_mps* mps, int32_t i, int32_t direction, double fwd_re, double fwd_im, double back_re, double back_im,
                         const htn_sweep_opts* opts, htn_bond_stats* stats) {
    if (!mps) return set_error("htn_site_evolve_move: bad arguments");
    if (mps->be->activate()) return 1;
    return mps->evolve_site_move(i, direction, cplx(fwd_re, fwd_im), cplx(back_re, back_im), norm_opts(opts), stats, nullptr);
}
int htn_tdvp1_sweep(htn_mps* mps, double dt_re, double dt_im, const htn_sweep_opts* opts, htn_bond_stats* stats, double* energy,
                    double* log_norm) {
    if (!mps) return set_error("htn_tdvp1_sweep: bad arguments");
    if (mps->be->activate()) return 1;
    return mps->tdvp1_sweep(cplx(dt_re, dt_im), norm_opts(opts), stats, energy, log_norm);
}
int64_t htn_mps_bond_size(htn_mps* mps, int32_t b) {
    if (!mps || b < 0 || b > mps->L) return -1;
    int64_t n = 0;
    for (int d : mps->bonds[b]->dims) n += (int64_t)d * d;
    return n;
}
int htn_heff0_apply(htn_mps* mps, int32_t b, const void* x_host, void* y_host) {
    if (!mps || !x_host || !y_host) return set_error("htn_heff0_apply: bad arguments");
    if (mps->bond0_checks(b, "htn_heff0_apply")) return 1;
    if (mps->be->activate()) return 1;
    auto ap = mps->make_apply0(b);
    if (!ap) return 1;
    return mps->apply_once(*ap, mps->Lbuf[b], mps->Rbuf[b], htn_mps_bond_size(mps, b), x_host, y_host, false);
}
// ---- correction-vector sweeps ---------------------------------------------------------------------------------------
int htn_bond_solve(htn_mps* x, int32_t i, int32_t direction, int32_t placement, double z_re, double z_im, const htn_sweep_opts* opts,
                   htn_bond_stats* stats, double* amp_host, double* bx_host) {
    if (!x) return set_error("htn_bond_solve: bad arguments");
    if (x->be->activate()) return 1;
    const htn_sweep_opts o = norm_opts(opts);
    if (x->cv_checks(o, "htn_bond_solve")) return 1;
    if (!(z_re - z_re == 0.0) || !(z_im - z_im == 0.0)) return set_error("htn_bond_solve: z is not finite");
    const cplx z(z_re, z_im);
    double out[3] = {0.0, 0.0, 0.0};
    if (x->update_bond(i, direction, placement == 0, false, o, stats, nullptr, nullptr, &z, out)) return 1;
    if (amp_host) *amp_host = out[0];
    if (bx_host) bx_host[0] = out[1], bx_host[1] = out[2];
    return 0;
}
int htn_cv_sweep(htn_mps* x, double z_re, double z_im, const htn_sweep_opts* opts, htn_bond_stats* stats, double* amp_host, double* bx_host) {
    if (!x) return set_error("htn_cv_sweep: bad arguments");
    if (x->be->activate()) return 1;
    if (!(z_re - z_re == 0.0) || !(z_im - z_im == 0.0)) return set_error("htn_cv_sweep: z is not finite");
    double out[3] = {0.0, 0.0, 0.0};
    if (x->cv_sweep(cplx(z_re, z_im), norm_opts(opts), stats, out)) return 1;
    if (amp_host) *amp_host = out[0];
    if (bx_host) bx_host[0] = out[1], bx_host[1] = out[2];
    return 0;
}
int htn_mps_set_mpo(htn_mps* mps, const htn_mpo* mpo) {
    if (!mps || !mpo) return set_error("htn_mps_set_mpo: bad arguments");
    if (mps->be->activate()) return 1;
    return mps->set_mpo(const_cast<htn_mpo*>(mpo));
}

// ---- excited states, overlaps, correlation functions ---------------------------------------------------------------
int htn_mps_set_orthogonal(htn_mps* mps, const htn_mps* const* others, int32_t n) {
    if (!mps || n < 0 || (n > 0 && !others)) return set_error("htn_mps_set_orthogonal: bad arguments");
    if (n > 8) return set_error("htn_mps_set_orthogonal: at most 8 attached states (%d given)", n);
    return mps->set_orthogonal(others, n);
}
int32_t htn_mps_orthogonal_count(const htn_mps* mps, int32_t* dropped_host) {
    if (dropped_host) *dropped_host = mps->orth_dropped;
    return (int32_t)mps->orth.size();
}
int htn_mps_overlap(htn_mps* a, const htn_mps* b, double* out_host) {
    if (!a || !b || !out_host) return set_error("htn_mps_overlap: bad arguments");
    return a->overlap(b, out_host);
}
int htn_mps_correlator(htn_mps* mps, const htn_corr_channel* ch, void* out_host, double* norm_host) {
    if (!mps || !ch || !out_host) return set_error("htn_mps_correlator: bad arguments");
    if (mps->be->activate()) return 1;
    return mps->correlator(*ch, (cplx*)out_host, norm_host);
}
int htn_mps_correlator2(htn_mps* mps, const htn_corr_channel2* ch, void* out_host, double* norm_host) {
    if (!mps || !ch || !out_host) return set_error("htn_mps_correlator2: bad arguments");
    if (mps->be->activate()) return 1;
    return mps->correlator2(*ch, (cplx*)out_host, norm_host);
}
int htn_mps_apply_op(const htn_mps* src, int32_t site, const htn_site_op* op, htn_mps** out, double* norm2_host) {
    if (!src || !op || !out) return set_error("htn_mps_apply_op: bad arguments");
    if (src->be->activate()) return 1;
    return const_cast<htn_mps*>(src)->apply_op(site, op, out, norm2_host);      // (the source's plan cache is the only thing written)
}
int htn_mps_transition(htn_mps* bra, const htn_site_op* op, const htn_mps* ket, void* out_host) {
    if (!bra || !op || !ket || !out_host) return set_error("htn_mps_transition: bad arguments");
    if (bra->be->activate()) return 1;
    return bra->transition(op, ket, (cplx*)out_host);
}
int htn_mps_variance(htn_mps* mps, double* site_host, double* bond_host, double* energy_host, double* split_host) {
    if (!mps) return set_error("htn_mps_variance: bad arguments");
    if (mps->be->activate()) return 1;
    return mps->variance(site_host, bond_host, energy_host, split_host);
}
int htn_mps_sample(htn_mps* mps, int32_t n_samples, const double* u_host, const int32_t* measure_host, int32_t batch, int32_t* out_host,
                   double* logp_host, double* split_host) {
    if (!mps || (n_samples > 0 && (!u_host || !out_host || !logp_host))) return set_error("htn_mps_sample: bad arguments");
    if (mps->be->activate()) return 1;
    return mps->sample(n_samples, u_host, measure_host, batch, out_host, logp_host, split_host);
}

// ---- queries of the state ------------------------------------------------------------------------------------------
int64_t htn_mps_theta_size(htn_mps* mps, int32_t i) {
    if (i < 0 || i + 1 >= mps->L) return -1;
    return mps->theta_layout(mps->bonds[i], mps->bonds[i + 2])->size;
}
int htn_heff2_apply(htn_mps* mps, int32_t i, const void* x_host, void* y_host) {
    if (i < 0 || i + 1 >= mps->L) return set_error("htn_heff2_apply: bond out of range");
    if (mps->be->activate()) return 1;
    ThetaLayoutP tl = mps->theta_layout(mps->bonds[i], mps->bonds[i + 2]);
    auto ap = mps->make_apply(i, *tl);
    if (!ap) return 1;
    return mps->apply_once(*ap, mps->Lbuf[i], mps->Rbuf[i + 2], tl->size, x_host, y_host, mps->ctx->shard);
}
int htn_mps_get_theta(htn_mps* mps, int32_t i, void* theta_host) {
    if (i < 0 || i + 1 >= mps->L) return set_error("htn_mps_get_theta: bond out of range");
    if (mps->be->activate()) return 1;
    ThetaLayoutP tl = mps->theta_layout(mps->bonds[i], mps->bonds[i + 2]);
    DView t = mps->zalloc(tl->size, false);
    if (!t.base) return set_error("device allocation failed");
    if (mps->theta_into(i, *tl, t.ptr())) return 1;
    return mps->be->download(theta_host, t.ptr(), sizeof(cplx) * tl->size);
}

int32_t htn_mps_nsites(const htn_mps* mps) { return mps->L; }
int32_t htn_mps_bond(const htn_mps* mps, int32_t b, htn_sector* out) {
    if (b < 0 || b > mps->L) return -1;
    const Bond& B = *mps->bonds[b];
    if (out)
        for (size_t k = 0; k < B.secs.size(); ++k) out[k] = {B.secs[k].N, B.secs[k].j, B.dims[k]};
    return (int32_t)B.secs.size();
}
int64_t htn_mps_spectrum(const htn_mps* mps, int32_t b, htn_sector* secs, double* values) {
    auto it = mps->spectra.find(b);
    if (it == mps->spectra.end()) return 0;
    int64_t tot = 0;
    for (size_t k = 0; k < it->second.secs.size(); ++k) {
        const auto& v = it->second.vals[k];
        if (secs) secs[k] = {it->second.secs[k].N, it->second.secs[k].j, (int32_t)v.size()};
        if (values) memcpy(values + tot, v.data(), sizeof(double) * v.size());
        tot += (int64_t)v.size();
    }
    return tot;
}
int64_t htn_mps_site_size(const htn_mps* mps, int32_t i, int32_t* kind) {
    if (i < 0 || i >= mps->L) return -1;
    if (kind) *kind = mps->site_lay[i]->kind;
    return mps->site_lay[i]->size;
}
int32_t htn_mps_get_site(const htn_mps* mps, int32_t i, htn_subblock* subs, void* data_host) {
    if (i < 0 || i >= mps->L) return -1;
    const SiteLayout& lay = *mps->site_lay[i];
    if (subs)
        for (size_t q = 0; q < lay.blocks.size(); ++q) {
            const Key& k = lay.bkeys[q];
            subs[q] = {k[0], k[1], k[2], k[3], k[4], lay.blocks[q].ld, lay.blocks[q].off};
        }
    if (data_host && lay.size && mps->be->activate()) return -1;
    if (data_host && lay.size && mps->be->download(data_host, mps->site_buf[i].ptr(), sizeof(cplx) * lay.size)) return -1;
    return (int32_t)lay.blocks.size();
}
int64_t htn_mps_env_size(const htn_mps* mps, int32_t side, int32_t b) {
    if (b < 0 || b > mps->L) return -1;
    const EnvLayoutP& l = side == 0 ? mps->Llay[b] : mps->Rlay[b];
    return l ? l->size : -1;
}
int htn_mps_get_env(const htn_mps* mps, int32_t side, int32_t b, void* data_host) {
    if (b < 0 || b > mps->L) return set_error("htn_mps_get_env: bond out of range");
    const EnvLayoutP& l = side == 0 ? mps->Llay[b] : mps->Rlay[b];
    if (!l) return set_error("htn_mps_get_env: environment %d of bond %d does not exist yet", side, b);
    if (l->size == 0) return 0;
    if (mps->be->activate()) return 1;
    return mps->be->download(data_host, (side == 0 ? mps->Lbuf[b] : mps->Rbuf[b]).ptr(), sizeof(cplx) * l->size);
}
int32_t htn_mps_env_blocks(const htn_mps* mps, int32_t side, int32_t b, htn_env_block* out) {
    if (b < 0 || b > mps->L) return -1;
    const EnvLayoutP& l = side == 0 ? mps->Llay[b] : mps->Rlay[b];
    if (!l) return -1;
    if (out)
        for (size_t q = 0; q < l->blocks.size(); ++q) {
            const Key& k = l->bkeys[q];
            out[q] = {k[0], k[1], k[2], k[3], k[4], l->blocks[q].m, l->blocks[q].n, 0, l->blocks[q].off};
        }
    return (int32_t)l->blocks.size();
}
int32_t htn_mps_env_bond(const htn_mps* mps, int32_t side, int32_t b, htn_sector* out) {
    if (b < 0 || b > mps->L) return -1;
    const EnvLayoutP& l = side == 0 ? mps->Llay[b] : mps->Rlay[b];
    if (!l) return -1;
    const Bond& B = *l->bond;
    if (out)
        for (size_t k = 0; k < B.secs.size(); ++k) out[k] = {B.secs[k].N, B.secs[k].j, B.dims[k]};
    return (int32_t)B.secs.size();
}
int htn_plan_apply_dump(htn_mps* mps, int32_t i, int32_t stage, int32_t* n_tiles, htn_tile* tiles, int32_t* n_segs, htn_seg* segs,
                        int64_t* z_size, int64_t* flops) {
    if (i < 0 || i + 1 >= mps->L) return set_error("htn_plan_apply_dump: bond out of range");
    ThetaLayoutP tl = mps->theta_layout(mps->bonds[i], mps->bonds[i + 2]);
    ApplyPlan p;
    plan_apply(*mps->mpo, *tl, *mps->Llay[i], *mps->Rlay[i + 2], mps->mpo->sites[i], mps->mpo->sites[i + 1], p);
    const Tasks& t = stage == 0 ? p.tz : p.ty;
    const bool have = stage != 0 || p.has_z;
    if (n_tiles) *n_tiles = have ? t.ntiles : 0;
    if (n_segs) *n_segs = have ? t.nsegs : 0;
    if (have && tiles) memcpy(tiles, t.tiles.data(), sizeof(htn_tile) * t.ntiles);
    if (have && segs) memcpy(segs, t.segs.data(), sizeof(htn_seg) * t.nsegs);
    if (z_size) *z_size = p.zsize;
    if (flops) *flops = have ? t.flops : 0;
    return 0;
}
int32_t htn_balance_tiles(const htn_tile* tiles, int32_t n_tiles, int32_t n_cus, htn_tile* out, int32_t out_cap, int32_t* n_out) {
    Tasks t;
    t.tiles.assign(tiles, tiles + std::max(n_tiles, 0));
    t.ntiles = n_tiles;
    const int ws = balance_tiles(t, n_cus > 0 ? n_cus : 256);
    if (n_out) *n_out = t.ntiles;
    if (out) {
        if (t.ntiles > out_cap) {
            set_error("htn_balance_tiles: %d records do not fit the output array (%d)", t.ntiles, out_cap);
            return -1;
        }
        memcpy(out, t.tiles.data(), sizeof(htn_tile) * (size_t)t.ntiles);
    }
    return ws;
}
int htn_mps_cache_stats(const htn_mps* mps, int64_t* hits, int64_t* misses) {
    if (hits) *hits = mps->hits;
    if (misses) *misses = mps->misses;
    return 0;
}

// ---- IDMRG2 driver -------------------------------------------------------------------------------------------------
int htn_idmrg_create(htn_ctx* ctx, const htn_mpo* mpo, const htn_idmrg_opts* opts, htn_idmrg** out) { return idmrg_create(ctx, mpo, opts, out); }
void htn_idmrg_destroy(htn_idmrg* d) { idmrg_free(d); }
int32_t htn_idmrg_boundary(const htn_idmrg* d, int32_t side, htn_sector* out) { return idmrg_boundary(d, side, out); }
int htn_idmrg_step(htn_idmrg* d, const int32_t* bond_ptr, const htn_sector* sectors, const int32_t* sub_ptr, const htn_subblock* subs,
                   const int64_t* data_ptr, const void* data_host, htn_idmrg_stats* stats) {
    return idmrg_step(d, bond_ptr, sectors, sub_ptr, subs, data_ptr, data_host, stats);
}
int htn_idmrg_window(htn_idmrg* d, htn_mps** out) { return idmrg_window(d, out); }

}  // extern "C"
