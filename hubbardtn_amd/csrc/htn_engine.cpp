// Bond-update / sweep driver behind the C ABI (include/hubbardtn_hip.h, "Bond-update / sweep level").
//
// Stands in for MPSKit's two-site sweep body reached from
//     find_groundstate(psi0, H, IDMRG2(; trscheme, tol))                src/HubbardFunctions.jl:1010
// per bond: form theta, Lanczos lowest eigenpair of the AC2 effective Hamiltonian, per-sector SVD + global truncation,
// write back, move the environment.  Sweep order follows MPSKit's DMRG2: bonds 1..L-1 going
// right, L-2..1 going left (2L-3 updates).  All tensors stay on the device between bonds; the host sees the Lanczos
// tridiagonal coefficients and the singular values (needed for the global truncation rule, App. A.6).
// This file is the core of the htn_mps state: the plan cache's users, the environments, the H_eff applies and the two-site
// update step by step.  The rest of the host core sits in one file per concern and is compiled as part of
// THIS translation unit (included below): htn_backend_host.cpp (host statements of Backend methods), htn_site.cpp (one-site
// updates, time evolution), htn_overlap.cpp (overlaps, attached states), htn_correlator.cpp (correlation functions: one probe
// pass), htn_applyop.cpp (local operators applied to a state), htn_variance.cpp (the two-site energy variance), htn_sample.cpp
// (perfect sampling), htn_idmrg.cpp (the infinite-chain growth loop), htn_capi.cpp (the C entry points).  One unit on purpose:
// a build line names htn_plan.cpp (the planner, which includes its own parts in the same way) and this file, as it always did,
// and g++ -O3 contracts the same fused multiply-adds in the host arithmetic as before the split -- across separate units the
// CPU baseline library changes its last bits (profiles/r07_engine_refactor_identity.txt, r09_engine_split_identity.txt).
// Host C++ (no HIP): device work goes through htn::Backend.
#include "htn_engine.h"
#include "htn_backend_host.cpp"

// One step of the H environment across site i.  side 'L': GL on bond i+1 from GL on bond i and the left-layout tensor of
// site i; side 'R': GR on bond i from GR on bond i+1 and the right-layout tensor of site i
int htn_mps::env_step(char side, int i) {
    const bool left = side == 'L';
    const SiteLayout& lay = *site_lay[i];
    if (lay.kind != side)
        return left ? set_error("left_env: site %d is not in left layout", i) : set_error("right_env: site %d is not in right layout", i);
    const MpoSite& W = mpo->sites[i];
    const int from = left ? i : i + 1, to = left ? i + 1 : i;
    std::vector<EnvLayoutP>& elay = left ? Llay : Rlay;
    std::vector<DView>& ebuf = left ? Lbuf : Rbuf;
    auto c = cached<EnvC>(ikey(left ? "lenv" : "renv", i) + bonds[i]->key + "|" + bonds[i + 1]->key, [&]() -> std::shared_ptr<EnvC> {
        auto e = std::make_shared<EnvC>();
        e->lay = build_env_layout(mpo->sym, side, bonds[to], left ? W.right : W.left);
        EnvPlan p;
        (left ? plan_left_env : plan_right_env)(*mpo, *elay[from], lay, W, *e->lay, p);
        return compile2(e, p);
    });
    if (!c || env_launch(left, *c, ebuf[from].ptr(), site_buf[i].ptr(), &ebuf[to])) return 1;
    elay[to] = c->lay;
    return 0;
}
// The launch half of an environment step, the Hamiltonian's or a probe's (htn_correlator.cpp): stage 1 takes the environment
// `in` and the site tensor to z, stage 2 the site tensor and z to the new environment, a fresh pool block
int htn_mps::env_launch(bool left, const EnvC& c, const cplx* in, const cplx* site, DView* out) {
    DView z = zalloc(c.zsize, false), o = zalloc(c.lay->size, false);
    if (!z.base || !o.base) return set_error("device allocation failed (%s environment)", left ? "left" : "right");
    if (gemm(c.d1, {{left ? BUF_L : BUF_R, in}, {BUF_S1, site}, {BUF_Z, z.ptr()}})) return 1;
    if (gemm(c.d2, {{BUF_S1, site}, {BUF_Z, z.ptr()}, {BUF_Y, o.ptr()}})) return 1;
    *out = o;
    return 0;
}

// ---- H_eff applies -----------------------------------------------------------------------------------------------------
// ApplyPlan -> ApplyC: counts for the statistics, then the Z and Y lists on the device.  deal_y (the two-site apply): with
// more than one rank the Y-stage tiles are dealt round-robin over the ranks first (tiles are in LPT order, so dealing
// balances MACs; every rank keeps the full segment table and the full Z stage; an empty deal keeps one tile)
std::shared_ptr<ApplyC> htn_mps::compile_apply(ApplyPlan& p, bool deal_y) {
    auto a = std::make_shared<ApplyC>();
    a->has_z = p.has_z;
    a->zsize = p.zsize;
    a->flops = p.ty.flops + (p.has_z ? p.tz.flops : 0);
    a->ntiles = p.ty.ntiles + (p.has_z ? p.tz.ntiles : 0);
    a->nsegs = p.ty.nsegs + (p.has_z ? p.tz.nsegs : 0);
    if (deal_y && ctx->world > 1) {
        std::vector<htn_tile> sel;
        for (int t = ctx->rank; t < p.ty.ntiles; t += ctx->world) sel.push_back(p.ty.tiles[t]);
        p.ty.ntiles = (int32_t)sel.size();
        if (sel.empty()) sel.push_back(p.ty.tiles[0]);
        p.ty.tiles.swap(sel);
    }
    if (p.has_z && upload_tasks(p.tz, a->dz)) return nullptr;
    if (upload_tasks(p.ty, a->dy)) return nullptr;
    return a;
}

// compiled H_eff apply of bond (i, i+1)
std::shared_ptr<ApplyC> htn_mps::make_apply(int i, const ThetaLayout& tl) {
    return cached<ApplyC>(ikey("apply", i) + bonds[i]->key + "|" + bonds[i + 2]->key, [&]() -> std::shared_ptr<ApplyC> {
        ApplyPlan p;
        plan_apply(*mpo, tl, *Llay[i], *Rlay[i + 2], mpo->sites[i], mpo->sites[i + 1], p);
        return compile_apply(p, true);
    });
}
// compiled one-site H_eff apply of site i in the layout `lay`
std::shared_ptr<ApplyC> htn_mps::make_apply1(int i, const SiteLayout& lay) {
    return cached<ApplyC>(ikey("apply1", i) + lay.kind + bonds[i]->key + "|" + bonds[i + 1]->key, [&]() -> std::shared_ptr<ApplyC> {
        ApplyPlan p;
        plan_apply1(*mpo, lay, *Llay[i], *Rlay[i + 1], mpo->sites[i], p);
        return compile_apply(p, false);
    });
}
// compiled zero-site H_eff apply of bond b (between sites b - 1 and b), in bond layout
std::shared_ptr<ApplyC> htn_mps::make_apply0(int b) {
    return cached<ApplyC>(ikey("apply0", b) + bonds[b]->key, [&]() -> std::shared_ptr<ApplyC> {
        ApplyPlan p;
        plan_apply0(*mpo, *bonds[b], *Llay[b], *Rlay[b], p);
        return compile_apply(p, false);
    });
}

// stage table of an apply between the environments L and R (the Z stage if the plan has one, then the Y stage), split-K
// workspace ensured; the Lanczos driver fills in x and y.  -> number of stages, < 0 on error
int htn_mps::apply_stages(const ApplyC& ap, const DView& L, const DView& R, const DView& z, htn_gemm_launch* stages) {
    if (ensure_ws(std::max(ap.dy.ws_slots, ap.has_z ? ap.dz.ws_slots : 0))) return -1;
    memset(stages, 0, 2 * sizeof(htn_gemm_launch));
    stages[0].bufs[HTN_BUF_WS] = stages[1].bufs[HTN_BUF_WS] = ws.ptr();
    int ns = 0;
    if (ap.has_z) {
        stages[ns].bufs[BUF_L] = L.ptr();
        stages[ns].bufs[BUF_Z] = z.ptr();
        stages[ns].tiles = ap.dz.tiles, stages[ns].segs = ap.dz.segs, stages[ns].n_tiles = ap.dz.ntiles;
        ++ns;
    }
    stages[ns].bufs[BUF_L] = L.ptr();
    stages[ns].bufs[BUF_R] = R.ptr();
    stages[ns].bufs[BUF_Z] = z.ptr();
    stages[ns].tiles = ap.dy.tiles, stages[ns].segs = ap.dy.segs, stages[ns].n_tiles = ap.dy.ntiles;
    return ns + 1;
}

int htn_mps::theta_into(int i, const ThetaLayout& tl, cplx* dst) {
    const SiteLayout &l1 = *site_lay[i], &l2 = *site_lay[i + 1];
    const char mode[3] = {l1.kind, l2.kind, 0};
    if (strcmp(mode, "RR") && strcmp(mode, "LL") && strcmp(mode, "LR")) return set_error("theta: centre is not on sites (%d, %d)", i, i + 1);
    auto d = cached<DevTasks>(std::string("theta") + mode + bonds[i]->key + "|" + bonds[i + 1]->key + "|" + bonds[i + 2]->key,
                              [&]() -> std::shared_ptr<DevTasks> {
                                  Tasks t;
                                  plan_theta(mode, l1, l2, tl, t);
                                  auto dt = std::make_shared<DevTasks>();
                                  if (upload_tasks(t, *dt)) return nullptr;
                                  return dt;
                              });
    if (!d) return 1;
    return gemm(*d, {{BUF_S1, site_buf[i].ptr()}, {BUF_S2, site_buf[i + 1].ptr()}, {BUF_Y, dst}});
}

static int exchange_tramp(void* y, int64_t n, void* user) {
    htn_ctx* ctx = (htn_ctx*)user;
    if (ctx->exch) return ctx->exch(y, n, ctx->exch_user);
    return ctx->be->allreduce(y, n);
}

// y = H_eff x once, host to host (htn_heff1_apply / htn_heff2_apply): upload x, Z stage, Y stage, download y; `exchange`:
// sum y over the ranks first (only the two-site entry shards its apply)
int htn_mps::apply_once(const ApplyC& ap, const DView& L, const DView& R, int64_t n, const void* x_host, void* y_host, bool exchange) {
    DView x = zalloc(n, false), y = zalloc(n, true), z = zalloc(ap.zsize, false);
    if (!x.base || !y.base || !z.base) return set_error("device allocation failed");
    if (be->upload(x.ptr(), x_host, sizeof(cplx) * n)) return 1;
    if (ap.has_z && gemm(ap.dz, {{BUF_X, x.ptr()}, {BUF_L, L.ptr()}, {BUF_Z, z.ptr()}})) return 1;
    if (gemm(ap.dy, {{BUF_X, x.ptr()}, {BUF_Y, y.ptr()}, {BUF_L, L.ptr()}, {BUF_R, R.ptr()}, {BUF_Z, z.ptr()}})) return 1;
    if (exchange && exchange_tramp(y.ptr(), n, ctx)) return set_error("htn_heff2_apply: exchange failed");
    return be->download(y_host, y.ptr(), sizeof(cplx) * n);
}

void htn_mps::fill_stats(htn_bond_stats* st, int bond, int direction, const Solve& sol, int64_t env_elems, int jacobi_sweeps,
                         int64_t svd_flops, double trunc_weight, const StageClock& clk) {
    memset(st, 0, sizeof(*st));
    st->bond = bond, st->direction = direction;
    st->n_matvec = sol.nmv, st->jacobi_sweeps = jacobi_sweeps;
    st->chi_full = (int32_t)bonds[bond]->dim_full(mpo->sym), st->multiplets = bonds[bond]->multiplets();
    st->n_tiles = sol.ap->ntiles, st->n_segs = sol.ap->nsegs;
    st->theta_size = sol.n;
    st->apply_flops = sol.ap->flops, st->apply_bytes = 16 * (2 * sol.n + env_elems), st->svd_flops = svd_flops;
    st->energy = sol.E, st->residual = sol.res, st->trunc_weight = trunc_weight;
    st->t_plan = clk.plan, st->t_lanczos = clk.lanczos, st->t_env = clk.env;
    st->t_total = now() - clk.t0;
    st->t_svd = clk.svd >= 0.0 ? clk.svd : st->t_total - clk.plan - clk.lanczos - clk.env;
    st->matvec_ms = sol.mv_ms > 0.0 ? sol.mv_ms : 0.0;      // (0: none of this solve's launches fell on the 1-in-8 timing sample)
}

// ---- two-site update, step by step ----------------------------------------------------------------
// solve: theta -> V[0], the compiled apply, the projector rows of attached states (optimising updates), Lanczos
int htn_mps::bond_solve(int i, bool optimise, const htn_sweep_opts& o, StageClock& clk, BondWork& w, const cplx* evolve_dt, const cplx* solve_z) {
    w.tl = theta_layout(bonds[i], bonds[i + 2]);
    const ThetaLayout& tl = *w.tl;
    Solve& s = w.sol;
    const int64_t n = s.n = tl.size;
    const int kd = o.krylovdim;
    if (n <= 0) return set_error("htn_bond_update: empty two-site tensor on bond %d", i);
    w.V = zalloc((int64_t)(kd + 2) * n, false);
    if (!w.V.base) return set_error("device allocation of the Krylov basis failed (%lld elements)", (long long)((kd + 2) * n));
    if (solve_z) {
        // correction-vector update: V[0] = p = amplitude(b) x O_L theta_b O_R, the projected right-hand side (kept in Qb for
        // <p|theta_new>); the start value is the state as it is, amplitude x theta
        const OrthState& os = orth[0];
        w.Qb = zalloc(n, false), w.X = zalloc(n, false);
        if (!w.Qb.base || !w.X.base) return set_error("device allocation failed (right-hand side of the solve)");
        if (ovl_project(os, i, tl, w.Qb.ptr())) return 1;
        if (os.phi->amp != 1.0 && be->scale(w.Qb.ptr(), n, os.phi->amp)) return 1;
        auto cp = cached<RelayC>(std::string("cvcopy") + std::string((const char*)&n, sizeof(n)), [&]() -> std::shared_ptr<RelayC> {
            auto r = std::make_shared<RelayC>();
            std::vector<htn_copy_item> items;
            for (int64_t off = 0; off < n; off += 1 << 30) {
                const int32_t rows = (int32_t)std::min<int64_t>(n - off, 1 << 30);
                items.push_back(copy_item(off, rows, off, rows, rows, 1));
            }
            r->n = (int)items.size();
            if (!(r->items = upload_vec(be, items))) return nullptr;
            return r;
        });
        if (!cp || be->batched_copy(w.V.ptr(), w.Qb.ptr(), nullptr, nullptr, (const htn_copy_item*)cp->items->p, cp->n, 1.0)) return 1;
        if (theta_into(i, tl, w.X.ptr())) return 1;
        if (amp != 1.0 && be->scale(w.X.ptr(), n, amp)) return 1;
    } else if (theta_into(i, tl, w.V.ptr())) return 1;         // theta -> V[0] (the Lanczos driver normalises it)
    s.ap = make_apply(i, tl);
    if (!s.ap) return 1;
    w.z = zalloc(s.ap->zsize, false);
    htn_gemm_launch stages[2];
    const int ns = apply_stages(*s.ap, Lbuf[i], Rbuf[i + 2], w.z, stages);
    if (ns < 0) return 1;
    clk.plan = clk.lap();
    const bool shard = ctx->shard;
    int n_frozen = 0;
    if (!orth.empty() && optimise) {
        // orthogonalised update: p_k = <phi_k| carried into this bond's bases, one row each; Gram-Schmidt (rows that depend on
        // the ones before them are dropped); then the lowest eigenpair of H_eff inside the complement of those rows
        const int na = (int)orth.size();
        if (kd + na > 31)
            return set_error("htn_bond_update: krylovdim + attached states = %d + %d > 31 (row limit of the projected Lanczos step)", kd, na);
        w.Qb = zalloc((int64_t)na * n, false);
        if (!w.Qb.base) return set_error("device allocation of the projector rows failed");
        for (int k = 0; k < na; ++k)
            if (ovl_project(orth[k], i, tl, w.Qb.ptr() + (int64_t)k * n)) return 1;
        if (be->orthonormalise_rows(w.Qb.ptr(), n, na, 1e-12, &n_frozen)) return 1;
        orth_dropped = na - n_frozen;
    }
    if (solve_z) {              // (theta <- (z - H_eff)^-1 p; E = Im <p|theta_new>, the spectral weight)
        double bx[2];
        if (be->krylov_solve(stages, ns, BUF_X, BUF_Y, w.V.ptr(), n, kd, solve_z->real(), solve_z->imag(), o.lanczos_tol, o.maxrestart,
                             w.X.ptr(), 1, 0, nullptr, ctx, &s.xnorm, &s.res, &s.nmv, be->timing ? &s.mv_ms : nullptr))
            return 1;
        if (be->dotc(w.Qb.ptr(), w.X.ptr(), n, bx)) return 1;
        s.bx = cplx(bx[0], bx[1]);
        s.E = bx[1];
    } else if (evolve_dt) {     // (evolving update: theta <- exp(-i dt H_eff) theta; E = <theta|H_eff|theta> before the step)
        if (be->krylov_expm(stages, ns, BUF_X, BUF_Y, w.V.ptr(), n, kd, evolve_dt->real(), evolve_dt->imag(), o.lanczos_tol, o.maxrestart, 0,
                            nullptr, ctx, &s.growth, &s.E, &s.nmv, &s.res, be->timing ? &s.mv_ms : nullptr))
            return 1;
    } else if (n_frozen > 0) {
        if (be->lanczos_orth(stages, ns, BUF_X, BUF_Y, w.V.ptr(), n, kd, o.lanczos_tol, o.maxrestart, shard ? 1 : 0,
                             shard ? exchange_tramp : nullptr, ctx, w.Qb.ptr(), n_frozen, &s.E, &s.nmv, &s.res,
                             be->timing ? &s.mv_ms : nullptr))
            return 1;
    } else if (be->lanczos(stages, ns, BUF_X, BUF_Y, w.V.ptr(), n, kd, optimise ? o.lanczos_tol : 1e300, o.maxrestart, shard ? 1 : 0,
                           shard ? exchange_tramp : nullptr, ctx, &s.E, &s.nmv, &s.res, be->timing ? &s.mv_ms : nullptr))
        return 1;
    clk.lanczos = clk.lap();
    return 0;
}

// compiled SVD of the theta layout: staging items and block descriptors on the device; with more than one rank also the
// lists of the blocks this rank owns
std::shared_ptr<SvdC> htn_mps::make_svd(int i, const ThetaLayout& tl, bool right) {
    return cached<SvdC>(std::string(right ? "svdR" : "svdL") + bonds[i]->key + "|" + bonds[i + 2]->key, [&]() -> std::shared_ptr<SvdC> {
        auto s = std::make_shared<SvdC>();
        if (plan_svd(tl, right, s->sp)) return nullptr;
        if (!(s->stage = upload_vec(be, s->sp.stage)) || !(s->desc = upload_vec(be, s->sp.desc))) return nullptr;
        if (ctx->world > 1) {
            // owner of every block: longest first onto the least loaded rank (deterministic: every rank computes the same map)
            const int nbk = (int)s->sp.mids.size();
            std::vector<int> ord(nbk);
            for (int b = 0; b < nbk; ++b) ord[b] = b;
            auto cost = [&](int b) { return (double)s->sp.desc[b].m * s->sp.desc[b].n * s->sp.desc[b].n; };
            std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return cost(a) > cost(b); });
            std::vector<double> load(ctx->world, 0.0);
            std::vector<htn_copy_item> st_own;
            for (int b : ord) {
                int r = 0;
                for (int q = 1; q < ctx->world; ++q)
                    if (load[q] < load[r]) r = q;
                load[r] += cost(b);
                if (r == ctx->rank) {
                    s->own_desc.push_back(s->sp.desc[b]);
                    st_own.push_back(s->sp.stage[b]);
                }
            }
            s->n_own = (int)s->own_desc.size();
            if (s->n_own && (!(s->own_stage = upload_vec(be, st_own)) || !(s->own_desc_dev = upload_vec(be, s->own_desc)))) return nullptr;
        }
        return s;
    });
}

// SVD: stage the optimised theta block by block, Jacobi, ONE download (singular values + per-block sweep counts share a
// buffer: one device-to-host copy, one stream sync per bond), convergence check
int htn_mps::bond_svd(int i, bool right, const htn_sweep_opts& o, BondWork& w) {
    w.sc = make_svd(i, *w.tl, right);
    if (!w.sc) return 1;
    const SvdC& sc = *w.sc;
    const SvdPlan& sp = sc.sp;
    const int nb = (int)sp.mids.size();
    w.G = zalloc(sp.g_size, false), w.Vj = zalloc(sp.v_size, false);
    w.s_elems = ((size_t)std::max<int64_t>(sp.s_size, 1) + 1) & ~(size_t)1;
    const size_t s_elems = w.s_elems, i_elems = (size_t)std::max(nb, 1);
    const size_t s_bytes = sizeof(double) * s_elems + sizeof(int32_t) * i_elems;
    w.S = dalloc(s_bytes);
    if (!w.G.base || !w.Vj.base || !w.S) return set_error("device allocation failed (SVD workspace)");
    int32_t* info_dev = (int32_t*)((double*)w.S->p + s_elems);
    // Sector-sharded SVD (world > 1): every rank stages and decomposes only the blocks it owns; everything else
    // in G / S (and the rotation workspace of accumulate-mode blocks) stays zero and ONE sum over ranks per buffer
    // hands every rank the complete result -- bit-identical everywhere (x + 0 + ... + 0), so the ranks stay in lock step.
    const bool svd_shard = ctx->world > 1 && ctx->shard;
    const DBufP& stage = svd_shard ? sc.own_stage : sc.stage;
    const DBufP& desc_dev = svd_shard ? sc.own_desc_dev : sc.desc;
    const htn_svd_block* desc_host = svd_shard ? sc.own_desc.data() : sp.desc.data();
    const int n_run = svd_shard ? sc.n_own : nb;               // (sharded: may be 0, then this rank only takes part in the sums)
    const bool run = n_run > 0 || !svd_shard;
    if (svd_shard) {
        if (be->zero(w.G.ptr(), sizeof(cplx) * (size_t)std::max<int64_t>(sp.g_size, 1))) return 1;
        if (be->zero(w.S->p, s_bytes)) return 1;
        if (sp.any_accumulate && be->zero(w.Vj.ptr(), sizeof(cplx) * (size_t)std::max<int64_t>(sp.v_size, 1))) return 1;
    }
    if (run && be->batched_copy(w.G.ptr(), w.V.ptr(), nullptr, nullptr, (const htn_copy_item*)stage->p, n_run, 1.0)) return 1;
    // Singular directions far below what the truncation keeps need not be resolved (optional, OFF by default).
    // truncbelow(eta): everything below eta goes anyway.  truncdim(D): if the previous update of this bond (same D) was
    // limited by D, its smallest kept value is where the cut will fall again.  x is normalised: values compare across sweeps.
    int32_t jac_used = 0;
    htn_svd_opts so = {o.svd_split_elems, 0, 0.0, &jac_used};      // split_elems, sweeps_hint, rank_cut, sweeps_used
    {       // the previous update of this bond tells how many outer sweeps the large blocks will need (speculation bound)
        auto h = sweeps_hint.find(i + 1);
        if (h != sweeps_hint.end()) so.sweeps_hint = h->second;
    }
    if (o.rank_cut > 0.0) {
        double cut = 0.0;
        auto h = cut_hint.find(i + 1);
        if (h != cut_hint.end() && h->second.first.first == o.chi_full && h->second.first.second == o.cutoff)
            cut = o.rank_cut * h->second.second;
        so.rank_cut = std::max(cut, o.rank_cut * o.cutoff);
    }
    if (run && be->jacobi_svd(w.G.ptr(), w.Vj.ptr(), (double*)w.S->p, (const htn_svd_block*)desc_dev->p, desc_host, n_run, sp.max_m,
                              o.jacobi_max_sweeps, o.jacobi_tol, info_dev, &so))
        return 1;
    if (svd_shard) {
        if (exchange_tramp(w.G.ptr(), std::max<int64_t>(sp.g_size, 1), ctx)) return set_error("sharded SVD: exchange of the blocks failed");
        if (exchange_tramp(w.S->p, (int64_t)(s_elems / 2), ctx)) return set_error("sharded SVD: exchange of the singular values failed");
        if (sp.any_accumulate && exchange_tramp(w.Vj.ptr(), std::max<int64_t>(sp.v_size, 1), ctx)) return 1;
    }
    if (jac_used > 0) sweeps_hint[i + 1] = jac_used;
    w.tA = now();
    w.s_host.resize(s_elems + (i_elems + 1) / 2);
    if (be->download(w.s_host.data(), w.S->p, s_bytes)) return 1;
    w.tB = now();
    const int32_t* info_h = (const int32_t*)(w.s_host.data() + s_elems);
    for (int b = 0; b < n_run; ++b) {                          // (sharded: the counts of this rank's own blocks)
        if (info_h[b] < 0) return set_error("Jacobi SVD did not converge (bond %d, block %d, %d sweeps)", i + 1, b, -info_h[b]);
        w.jac_sweeps = std::max(w.jac_sweeps, (int)info_h[b]);
    }
    return 0;
}

// truncate (host only): per-block descending order (ties: original column index ascending), the global truncation rule,
// the new middle bond, the hint for the next visit of this bond
int htn_mps::bond_truncate(int i, const htn_sweep_opts& o, BondWork& w) {
    const SvdPlan& sp = w.sc->sp;
    const int nb = (int)sp.mids.size();
    w.lens.resize(nb), w.qd.resize(nb), w.order.resize(nb);
    w.vals.reserve((size_t)sp.s_size);
    std::vector<std::pair<double, int>> tmp;
    for (int b = 0; b < nb; ++b) {
        const int len = sp.desc[b].n;
        const double* sv = w.s_host.data() + sp.desc[b].s_off;
        w.lens[b] = len;
        w.qd[b] = mpo->sym.qdim(sp.mids[b]);
        tmp.resize(len);
        for (int k = 0; k < len; ++k) tmp[k] = {sv[k], k};
        std::sort(tmp.begin(), tmp.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& c) {
            return a.first != c.first ? a.first > c.first : a.second < c.second;
        });
        w.order[b].resize(len);
        for (int k = 0; k < len; ++k) {
            w.order[b][k] = tmp[k].second;
            w.vals.push_back(tmp[k].first);
        }
    }
    truncate(w.vals, w.lens, w.qd, o.chi_full, o.cutoff, o.weighting, w.counts, w.tw, w.nrm);
    std::vector<std::pair<Sec, int>> mid_items;
    int64_t kept_tot = 0, positive = 0;
    for (int b = 0; b < nb; ++b) {
        if (w.counts[b] > 0) mid_items.push_back({sp.mids[b], w.counts[b]});
        kept_tot += w.counts[b];
    }
    for (double v : w.vals) positive += v > 0.0;
    if (kept_tot == 0 || !(w.nrm > 0.0)) return set_error("htn_bond_update: nothing kept by the truncation on bond %d", i + 1);
    w.mid = std::make_shared<Bond>(mid_items);
    w.tC = now();
    // hint for the next visit of this bond: the smallest kept value, valid only if the dimension limit (not the number
    // of available states) ended the kept set
    if (o.chi_full > 0 && w.tw > 0.0 && kept_tot < positive) {
        double smin = 1e300;
        size_t p = 0;
        for (int b = 0; b < nb; ++b) {
            if (w.counts[b] > 0) smin = std::min(smin, w.vals[p + w.counts[b] - 1]);
            p += w.lens[b];
        }
        cut_hint[i + 1] = {{o.chi_full, o.cutoff}, smin};
    } else
        cut_hint.erase(i + 1);
    return 0;
}

// finalise: the copy items of the kept counts (memoised: the plan depends on the COUNTS only, not on which columns carry
// them), gather of the kept columns into the two site tensors, the centre GEMM, store sites and bond
int htn_mps::bond_finalise(int i, bool right, BondWork& w) {
    const ThetaLayout& tl = *w.tl;
    const SvdPlan& sp = w.sc->sp;
    const std::vector<int>& counts = w.counts;
    const BondP bl = bonds[i], br = bonds[i + 2], mid = w.mid;
    std::string ckey((const char*)counts.data(), sizeof(int) * counts.size());
    auto fc = cached<FinC>(std::string(right ? "finR" : "finL") + bl->key + "|" + br->key + "|" + ckey, [&]() -> std::shared_ptr<FinC> {
        auto f = std::make_shared<FinC>();
        f->layA = site_layout('L', bl, mid);
        f->layB = site_layout('R', mid, br);
        FinalizePlan fp;
        plan_finalize(tl, sp, counts, *f->layA, *f->layB, right, 0, f->layA->size, fp);
        f->n_ig = (int)fp.iso_g.size(), f->n_cg = (int)fp.cen_g.size(), f->n_iv = (int)fp.iso_v.size();
        if (f->n_ig + f->n_cg + f->n_iv) {
            std::vector<htn_copy_item> all;
            all.insert(all.end(), fp.iso_g.begin(), fp.iso_g.end());
            all.insert(all.end(), fp.cen_g.begin(), fp.cen_g.end());
            all.insert(all.end(), fp.iso_v.begin(), fp.iso_v.end());
            if (!(f->items = upload_vec(be, all))) return nullptr;
            f->ig = (const htn_copy_item*)f->items->p;
            f->cg = f->ig + f->n_ig;
            f->iv = f->cg + f->n_cg;
        }
        f->has_cen = fp.has_cen;
        if (fp.has_cen && upload_tasks(fp.cen, f->cen)) return nullptr;
        return f;
    });
    if (!fc) return 1;
    w.tD = now();
    idx_host.clear();
    for (size_t b = 0; b < counts.size(); ++b)
        for (int k = 0; k < counts[b]; ++k) idx_host.push_back(w.order[b][k]);
    w.idx = upload_vec(be, idx_host);
    const int64_t sizeA = fc->layA->size, sizeB = fc->layB->size;
    DView out = zalloc(sizeA + sizeB, true);
    if (!w.idx || !out.base) return set_error("device allocation failed (site tensors)");
    const int32_t* idxp = (const int32_t*)w.idx->p;
    const double* Sp = (const double*)w.S->p;
    cplx* x = w.V.ptr();
    const int64_t n = tl.size;
    if (fc->n_ig && be->batched_copy(out.ptr(), w.G.ptr(), idxp, Sp, fc->ig, fc->n_ig, 1.0)) return 1;
    if (fc->n_cg && be->batched_copy(out.ptr(), w.G.ptr(), idxp, Sp, fc->cg, fc->n_cg, 1.0 / w.nrm)) return 1;
    if (fc->n_iv && be->batched_copy(out.ptr(), w.Vj.ptr(), idxp, Sp, fc->iv, fc->n_iv, 1.0)) return 1;
    if (fc->has_cen) {
        if (be->scale(x, n, 1.0 / w.nrm)) return 1;             // centre = U^H (M / nrm)
        if (gemm(fc->cen, {{BUF_X, x}, {BUF_S1, out.ptr()}, {BUF_Y, out.ptr()}})) return 1;
    }
    bonds[i + 1] = mid;
    site_lay[i] = fc->layA;
    site_buf[i] = DView{out.base, out.off};
    site_lay[i + 1] = fc->layB;
    site_buf[i + 1] = DView{out.base, out.off + sizeA};
    return 0;
}

// advance: the H environment across the site that became an isometry, and the overlap environments of attached states
// with it (non-optimising moves too)
int htn_mps::bond_advance(int i, bool right) {
    if (right ? left_env(i) : right_env(i + 1)) return 1;
    for (auto& os : orth)
        if (right ? ovl_step('L', os.phi, i, os.Llay[i], os.Lbuf[i], &os.Llay[i + 1], &os.Lbuf[i + 1])
                  : ovl_step('R', os.phi, i + 1, os.Rlay[i + 2], os.Rbuf[i + 2], &os.Rlay[i + 1], &os.Rbuf[i + 1]))
            return 1;
    return 0;
}

// Schmidt spectrum of the new middle bond: the kept values of the normalised state, per sector
void htn_mps::bond_spectrum(int i, const BondWork& w) {
    const SvdPlan& sp = w.sc->sp;
    Spectrum spec;
    size_t p = 0;
    for (size_t b = 0; b < w.counts.size(); ++b) {
        if (w.counts[b] > 0) {
            spec.secs.push_back(sp.mids[b]);
            std::vector<double> v(w.counts[b]);
            const double f = 1.0 / w.nrm / sqrt((double)w.qd[b]);
            for (int k = 0; k < w.counts[b]; ++k) v[k] = w.vals[p + k] * f;
            spec.vals.push_back(std::move(v));
        }
        p += w.lens[b];
    }
    spectra[i + 1] = std::move(spec);
}

int htn_mps::update_bond(int i, int direction, bool right, bool optimise, const htn_sweep_opts& o, htn_bond_stats* st,
                         const cplx* evolve_dt, double* log_growth, const cplx* solve_z, double* cv_out) {
    if (i < 0 || i + 1 >= L) return set_error("htn_bond_update: bond index %d out of range", i);
    StageClock clk(be, o.profile);
    BondWork w;
    if (bond_solve(i, optimise, o, clk, w, evolve_dt, solve_z)) return 1;          // (laps clk.plan and clk.lanczos)
    if (log_growth) *log_growth += log(w.sol.growth);
    const double t_svd0 = clk.last;
    if (bond_svd(i, right, o, w)) return 1;
    if (bond_truncate(i, o, w)) return 1;
    if (bond_finalise(i, right, w)) return 1;
    static const bool dbg_timers = getenv("HTN_DEBUG_HOST_TIMERS") != nullptr;
    if (dbg_timers)
        fprintf(stderr, "bond %d: svd call %.1f us, download %.1f, sort+truncate %.1f, finalize plan %.1f, enqueue %.1f  misses %lld hits %lld nvals %zu\n", i + 1,
                (w.tA - t_svd0) * 1e6, (w.tB - w.tA) * 1e6, (w.tC - w.tB) * 1e6, (w.tD - w.tC) * 1e6, (now() - w.tD) * 1e6, (long long)misses, (long long)hits, w.vals.size());
    clk.svd = clk.lap();
    if (bond_advance(i, right)) return 1;
    clk.env = clk.lap();
    if (!solve_z) energy = w.sol.E;
    centre = right ? i + 1 : i;
    norm_absorbed();
    if (solve_z) {              // the tensors are normalised; the norm of the solution is the state's amplitude
        amp = w.sol.xnorm;
        if (cv_out) cv_out[0] = amp, cv_out[1] = w.sol.bx.real(), cv_out[2] = w.sol.bx.imag();
    }
    bond_spectrum(i, w);
    if (st) fill_stats(st, i + 1, direction, w.sol, Llay[i]->size + Rlay[i + 2]->size, w.jac_sweeps, w.sc->sp.flops, w.tw, clk);
    return 0;
}

int htn_mps::sweep(const htn_sweep_opts& o, htn_bond_stats* st, double* E) {
    int k = 0;
    for (int i = 0; i < L - 1; ++i, ++k)
        if (update_bond(i, +1, i < L - 2, true, o, st ? st + k : nullptr)) return 1;
    for (int i = L - 3; i >= 0; --i, ++k)
        if (update_bond(i, -1, false, true, o, st ? st + k : nullptr)) return 1;
    if (E) *E = energy;
    return 0;
}

htn_sweep_opts norm_opts(const htn_sweep_opts* o) {
    htn_sweep_opts d;
    memset(&d, 0, sizeof(d));
    d.krylovdim = 30;
    d.maxrestart = 3;
    d.lanczos_tol = 1e-12;
    d.jacobi_tol = 1e-14;
    d.jacobi_max_sweeps = 40;
    if (!o) return d;
    htn_sweep_opts r = *o;
    if (r.krylovdim <= 0) r.krylovdim = d.krylovdim;
    if (r.lanczos_tol <= 0.0) r.lanczos_tol = d.lanczos_tol;
    if (r.jacobi_tol <= 0.0) r.jacobi_tol = d.jacobi_tol;
    if (r.jacobi_max_sweeps <= 0) r.jacobi_max_sweeps = d.jacobi_max_sweeps;
    if (r.maxrestart < 0) r.maxrestart = 0;
    return r;
}

// ---- construction of an htn_mps: shared by htn_mps_create and the IDMRG2 driver ------------------------------------
htn_mps* mps_new(htn_ctx* ctx, const htn_mpo* mpo) {
    htn_mps* e = new htn_mps();
    e->ctx = ctx;
    ++ctx->refs;
    e->mpo_handle = const_cast<htn_mpo*>(mpo);
    ++e->mpo_handle->refs;
    e->be = ctx->be.get();
    e->mpo = &mpo->mpo;
    const int nsites = e->L = (int)mpo->mpo.sites.size();
    e->site_lay.resize(nsites);
    e->site_buf.resize(nsites);
    e->Llay.resize(nsites + 1);
    e->Rlay.resize(nsites + 1);
    e->Lbuf.resize(nsites + 1);
    e->Rbuf.resize(nsites + 1);
    return e;
}
int mps_load_bonds(htn_mps* e, const int32_t* bond_ptr, const htn_sector* sectors) {
    e->bonds.clear();
    for (int b = 0; b <= e->L; ++b) {
        std::vector<std::pair<Sec, int>> items;
        for (int q = bond_ptr[b]; q < bond_ptr[b + 1]; ++q) items.push_back({{sectors[q].N, sectors[q].j}, sectors[q].count});
        e->bonds.push_back(std::make_shared<Bond>(items));
        if (e->bonds.back()->secs.empty()) return set_error("htn_mps_create: bond %d is empty", b);
    }
    return 0;
}
// site tensors from the caller's sub-block tables, uploaded in right layout
int mps_load_sites(htn_mps* e, const int32_t* sub_ptr, const htn_subblock* subs, const int64_t* data_ptr, const void* data_host) {
    const cplx* data = (const cplx*)data_host;
    std::vector<cplx> flat;
    for (int i = 0; i < e->L; ++i) {
        SiteLayoutP lay = e->site_layout('R', e->bonds[i], e->bonds[i + 1]);
        flat.assign((size_t)std::max<int64_t>(lay->size, 1), cplx(0.0, 0.0));
        for (int q = sub_ptr[i]; q < sub_ptr[i + 1]; ++q) {
            const htn_subblock& sb = subs[q];
            const int bi = lay->block({sb.lN, sb.lj}, sb.s, {sb.rN, sb.rj});
            if (bi < 0) continue;          // a sub-block between sectors the bond tables do not hold
            const BlockRec& r = lay->blocks[bi];
            if (sb.ld < r.m) return set_error("htn_mps_create: sub-block of site %d has ld %d < %d rows", i, sb.ld, r.m);
            const cplx* src = data + data_ptr[i] + sb.off;
            for (int c = 0; c < r.n; ++c)
                for (int rr = 0; rr < r.m; ++rr) flat[(size_t)(r.off + rr + (int64_t)c * r.ld)] = src[rr + (int64_t)c * sb.ld];
        }
        e->site_lay[i] = lay;
        e->site_buf[i] = e->zalloc(lay->size, false);
        if (!e->site_buf[i].base) return set_error("htn_mps_create: device allocation failed");
        if (e->be->upload(e->site_buf[i].ptr(), flat.data(), sizeof(cplx) * flat.size())) return 1;
    }
    return 0;
}
// boundaries: an open end (no environment blocks: only the implicit identity level), or -- for a window inside a
// larger system -- the environment of the block beyond that end, in this library's block order: from the host
// (htn_mps_create) or a device buffer the IDMRG2 driver keeps (shared, never written); then the right environments
int mps_finish(htn_mps* e, const void* left_env_host, const void* right_env_host, const DView* left_dev, const DView* right_dev) {
    const int nsites = e->L;
    const Mpo& mpo = *e->mpo;
    e->Llay[0] = build_env_layout(mpo.sym, 'L', e->bonds[0], mpo.sites[0].left);
    e->Rlay[nsites] = build_env_layout(mpo.sym, 'R', e->bonds[nsites], mpo.sites[nsites - 1].right);
    if (left_dev)
        e->Lbuf[0] = *left_dev;
    else {
        e->Lbuf[0] = e->zalloc(e->Llay[0]->size, true);
        if (left_env_host && e->Llay[0]->size && e->Lbuf[0].base && e->be->upload(e->Lbuf[0].ptr(), left_env_host, sizeof(cplx) * e->Llay[0]->size))
            return 1;
        if (!left_env_host && e->Llay[0]->size) return set_error("htn_mps_create: the left MPO bond is not a boundary: left_env required");
    }
    if (right_dev)
        e->Rbuf[nsites] = *right_dev;
    else {
        e->Rbuf[nsites] = e->zalloc(e->Rlay[nsites]->size, true);
        if (right_env_host && e->Rlay[nsites]->size && e->Rbuf[nsites].base &&
            e->be->upload(e->Rbuf[nsites].ptr(), right_env_host, sizeof(cplx) * e->Rlay[nsites]->size))
            return 1;
        if (!right_env_host && e->Rlay[nsites]->size) return set_error("htn_mps_create: the right MPO bond is not a boundary: right_env required");
    }
    if (!e->Lbuf[0].base || !e->Rbuf[nsites].base) return set_error("htn_mps_create: device allocation failed");
    for (int i = nsites - 1; i >= 1; --i)
        if (e->right_env(i)) return 1;
    return e->be->sync();
}

// the quench: another Hamiltonian under the same state.  Everything that was planned or contracted with the old MPO goes (the
// plan cache, the environments); the boundaries and the right environments are rebuilt as mps_finish builds them.
int htn_mps::set_mpo(htn_mpo* m) {
    const Mpo& nm = m->mpo;
    if (m->ctx != ctx) return set_error("htn_mps_set_mpo: the MPO lives in a different context");
    if ((int)nm.sites.size() != L) return set_error("htn_mps_set_mpo: the MPO has %d sites, the state %d", (int)nm.sites.size(), L);
    const Sym &a = mpo->sym, &b = nm.sym;
    bool same = a.kind == b.kind && a.n_site == b.n_site;
    for (int q = 0; same && q < a.n_site; ++q) same = a.site[q] == b.site[q];
    if (!same) return set_error("htn_mps_set_mpo: the MPO has a different symmetry or other site multiplets");
    if (centre != 0) return set_error("htn_mps_set_mpo: the centre is on site %d, not on site 0", centre);
    if (Llay[0]->size != 0 || Rlay[L]->size != 0 || nm.sites.front().left.size() != 1 || nm.sites.back().right.size() != 1)
        return set_error("htn_mps_set_mpo: a chain with boundary environments (an iDMRG window) cannot change its Hamiltonian");
    for (int i = 1; i < L; ++i)
        if (site_lay[i]->kind != 'R') return set_error("htn_mps_set_mpo: site %d is not in right layout", i);
    // the new environments are built first, with the old ones set aside: a failure puts everything back
    htn_mpo* old = mpo_handle;
    const Mpo* old_mpo = mpo;
    auto old_cache = std::move(cache);
    auto oLl = Llay, oRl = Rlay;
    auto oLb = Lbuf, oRb = Rbuf;
    ++m->refs;
    mpo_handle = m;
    mpo = &m->mpo;
    cache.clear();
    for (int b2 = 0; b2 <= L; ++b2) {
        Llay[b2] = nullptr, Rlay[b2] = nullptr;
        Lbuf[b2] = DView(), Rbuf[b2] = DView();
    }
    if (mps_finish(this, nullptr, nullptr, nullptr, nullptr)) {
        mpo_handle = old;
        mpo = old_mpo;
        cache = std::move(old_cache);
        Llay = oLl, Rlay = oRl, Lbuf = oLb, Rbuf = oRb;
        mpo_release(m);
        return 1;
    }
    mpo_release(old);
    energy = NAN;                  // (no energy of the new Hamiltonian is known until an update reports one)
    return 0;
}

// ---- the rest of the engine, one file per concern (see the head of this file) ---------------------------------------------
#include "htn_site.cpp"
#include "htn_overlap.cpp"
#include "htn_correlator.cpp"
#include "htn_applyop.cpp"
#include "htn_variance.cpp"
#include "htn_sample.cpp"
#include "htn_idmrg.cpp"
#include "htn_capi.cpp"
