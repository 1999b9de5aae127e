// One-site updates and time evolution of an htn_mps (htn_engine.h): htn_site_update / htn_dmrg1_sweep, and htn_site_evolve /
// htn_tdvp2_sweep, whose backward step is the same one-site solve under an exponential, and htn_site_evolve_move /
// htn_tdvp1_sweep, one-site TDVP, whose backward step is a zero-site solve on the bond.  Host C++ (no HIP).
// NOT a translation unit of its own: #included by htn_engine.cpp (one unit, see its head); never name it on a build line.
#include "htn_engine.h"

// =====================================================================================================================
// One-site DMRG at fixed bond tables (htn_site_update / htn_dmrg1_sweep).  The Lanczos vector is the centre site's stored
// data; the gauge move is an unpivoted QR (rightwards, left layout: one matrix [(l, s) ; n_r] per right sector) or LQ
// (leftwards, right layout: [n_l ; (s, r)] per left sector) through Backend::qr_blocks, the triangular factor goes into
// the neighbour by one grouped GEMM.  No scale factors: in the tilde normalisation left isometries carry 1, the centre
// sqrt(2S_r + 1) in both layout kinds and right tensors sqrt((2S_r + 1) / (2S_l + 1)), so R (carrying sqrt(2S_c + 1))
// times B_{i+1} and A_{i-1} times L are centres again and Q is orthonormal in the plain sense.
// =====================================================================================================================
// dst (layout `to`) = src (layout `from`), block by block: the two kinds hold the same (l, s, r) blocks with the same values
int htn_mps::relay(const SiteLayout& from, const cplx* src, const SiteLayout& to, cplx* dst) {
    auto rc = cached<RelayC>(std::string("relay") + from.kind + to.kind + from.bl->key + "|" + from.br->key, [&]() -> std::shared_ptr<RelayC> {
        std::vector<htn_copy_item> items;
        for (size_t q = 0; q < to.blocks.size(); ++q) {
            const Key& k = to.bkeys[q];
            const int sq = from.block({k[0], k[1]}, k[2], {k[3], k[4]});
            if (sq < 0) continue;
            const BlockRec &D = to.blocks[q], &S = from.blocks[sq];
            items.push_back(copy_item(D.off, D.ld, S.off, S.ld, D.m, D.n));
        }
        auto r = std::make_shared<RelayC>();
        r->n = (int)items.size();
        if (!(r->items = upload_vec(be, items))) return nullptr;
        return r;
    });
    if (!rc) return 1;
    return rc->n ? be->batched_copy(dst, src, nullptr, nullptr, (const htn_copy_item*)rc->items->p, rc->n, 1.0) : 0;
}

int site1_checks(const htn_mps* m, int i, const char* who) {
    if (i < 0 || i >= m->L) return set_error("%s: site %d out of range", who, i);
    if (m->centre != i) return set_error("%s: the centre is on site %d, not on site %d", who, m->centre, i);
    if (!m->orth.empty()) return set_error("%s: one-site updates of a state with attached orthogonal states are not supported", who);
    if (m->ctx->world > 1 || m->ctx->shard || m->be->has_comm())
        return set_error("%s: one-site updates on a context with a communicator are not supported", who);
    if (!m->Llay[i] || !m->Rlay[i + 1] || m->Llay[i]->bond->key != m->bonds[i]->key || m->Rlay[i + 1]->bond->key != m->bonds[i + 1]->key)
        return set_error("%s: the environments of site %d were built on other bond tables: run a two-site sweep first", who, i);
    return 0;
}

struct SiteWork {                  // what the solve of a one-site update leaves for what follows it
    Solve sol;
    // device buffers: live until the update returns and go back to the pool in reverse order of declaration
    DView V, z, out;               // Krylov basis (row 0: the site tensor, then the result); Z stage of the apply; the new site tensor
};

// solve: the site tensor (stored in layout `from`) -> V[0] in layout `lay`, the compiled one-site apply, then Lanczos
// (optimise = false: <x|H_eff|x> only) or, with evolve_dt, x <- exp(-i dt H_eff) x; the result in layout `lay` -> a fresh w.out
int htn_mps::site_solve(int i, const SiteLayout& from, const SiteLayout& lay, bool optimise, const cplx* evolve_dt, const htn_sweep_opts& o,
                        StageClock& clk, SiteWork& w) {
    Solve& s = w.sol;
    const int64_t n = s.n = lay.size;
    const int kd = o.krylovdim;
    w.V = zalloc((int64_t)(kd + 2) * n, false);
    if (!w.V.base) return set_error("device allocation of the Krylov basis failed (%lld elements)", (long long)((kd + 2) * n));
    if (relay(from, site_buf[i].ptr(), lay, w.V.ptr())) return 1;
    s.ap = make_apply1(i, lay);
    if (!s.ap) return 1;
    w.z = zalloc(s.ap->zsize, false);
    if (!w.z.base) return set_error("device allocation failed (one-site apply)");
    htn_gemm_launch stages[2];
    const int ns = apply_stages(*s.ap, Lbuf[i], Rbuf[i + 1], w.z, stages);
    if (ns < 0) return 1;
    clk.plan = clk.lap();
    if (evolve_dt) {
        if (be->krylov_expm(stages, ns, BUF_X, BUF_Y, w.V.ptr(), n, kd, evolve_dt->real(), evolve_dt->imag(), o.lanczos_tol, o.maxrestart, 0,
                            nullptr, ctx, &s.growth, &s.E, &s.nmv, &s.res, be->timing ? &s.mv_ms : nullptr))
            return 1;
    } else if (be->lanczos(stages, ns, BUF_X, BUF_Y, w.V.ptr(), n, kd, optimise ? o.lanczos_tol : 1e300, o.maxrestart, 0, nullptr, ctx, &s.E,
                           &s.nmv, &s.res, be->timing ? &s.mv_ms : nullptr))
        return 1;
    clk.lanczos = clk.lap();
    w.out = zalloc(n, false);
    if (!w.out.base) return set_error("device allocation failed (site tensor)");
    return relay(lay, w.V.ptr(), lay, w.out.ptr());
}

int htn_mps::update_site(int i, int direction, bool optimise, const htn_sweep_opts& o, htn_bond_stats* st) {
    if (site1_checks(this, i, "htn_site_update")) return 1;
    if (direction < -1 || direction > 1) return set_error("htn_site_update: direction %d (must be -1, 0 or +1)", direction);
    if ((direction > 0 && i + 1 >= L) || (direction < 0 && i == 0))
        return set_error("htn_site_update: site %d has no neighbour in direction %d", i, direction);
    StageClock clk(be, o.profile);
    const SiteLayoutP cur = site_lay[i];
    const SiteLayoutP lay = direction == 0 ? cur : site_layout(direction > 0 ? 'L' : 'R', bonds[i], bonds[i + 1]);
    if (lay->size <= 0) return set_error("htn_site_update: empty site tensor on site %d", i);
    for (const auto& M : lay->mats)      // a full-rank gauge move needs the long side along the orthonormal direction
        if (direction != 0 && (lay->kind == 'L' ? M.rows < M.cols : M.cols < M.rows))
            return set_error("htn_site_update: sector (%d, %d) of site %d is a %d x %d block, its bond is wider than the rest of the "
                             "site supports: run a two-site sweep first", M.c.N, M.c.j, i, M.rows, M.cols);
    if (direction != 0 && site_lay[i + direction]->kind != (direction > 0 ? 'R' : 'L'))
        return set_error("htn_site_update: site %d is not in %s layout", i + direction, direction > 0 ? "right" : "left");
    SiteWork w;
    if (site_solve(i, *cur, *lay, optimise, nullptr, o, clk, w)) return 1;         // (laps clk.plan and clk.lanczos)
    const Solve& s = w.sol;
    const DView& out = w.out;
    // ---- the optimised centre is in `out`; now the gauge move ----
    const int crossed = direction > 0 ? i + 1 : i;
    if (direction != 0) {
        const int j = i + direction;
        const SiteLayoutP nl = site_lay[j];
        auto gc = cached<Gauge1C>(std::string(direction > 0 ? "gauge1R" : "gauge1L") + lay->bl->key + "|" + lay->br->key + "|" +
                                      (direction > 0 ? nl->br->key : nl->bl->key),
                                  [&]() -> std::shared_ptr<Gauge1C> {
                                      auto g = std::make_shared<Gauge1C>();
                                      Tasks t;
                                      plan_gauge1(*lay, *nl, g->desc, g->rsize, t);
                                      if (!(g->desc_dev = upload_vec(be, g->desc)) || upload_tasks(t, g->absorb)) return nullptr;
                                      return g;
                                  });
        if (!gc) return 1;
        DView Rf = zalloc(gc->rsize, false), nb_out = zalloc(nl->size, false);
        if (!Rf.base || !nb_out.base) return set_error("device allocation failed (gauge move)");
        if (be->qr_blocks(out.ptr(), Rf.ptr(), (const htn_qr_block*)gc->desc_dev->p, gc->desc.data(), (int)gc->desc.size())) return 1;
        if (gemm(gc->absorb, {{BUF_S1, Rf.ptr()}, {BUF_S2, site_buf[j].ptr()}, {BUF_Y, nb_out.ptr()}})) return 1;
        site_lay[i] = lay;
        site_buf[i] = out;
        site_buf[j] = nb_out;
        centre = j;
        clk.lap();                       // (the QR / LQ and the absorption: t_svd is what the other stages leave of the total)
        if (direction > 0 ? left_env(i) : right_env(i)) return 1;
        clk.env = clk.lap();
    } else {
        site_lay[i] = lay;
        site_buf[i] = out;
    }
    energy = s.E;
    norm_absorbed();
    if (st) fill_stats(st, crossed, direction, s, Llay[i]->size + Rlay[i + 1]->size, 0, 0, 0.0, clk);
    return 0;
}

int htn_mps::sweep1(const htn_sweep_opts& o, htn_bond_stats* st, double* E) {
    if (L < 2) return set_error("htn_dmrg1_sweep: a chain of %d site(s) has no bond to sweep over", L);
    if (centre != 0) return set_error("htn_dmrg1_sweep: the centre is on site %d, not on site 0", centre);
    int k = 0;
    for (int i = 0; i < L - 1; ++i, ++k)
        if (update_site(i, +1, true, o, st ? st + k : nullptr)) return 1;
    for (int i = L - 1; i >= 1; --i, ++k)
        if (update_site(i, -1, true, o, st ? st + k : nullptr)) return 1;
    if (E) *E = energy;
    return 0;
}

// =====================================================================================================================
// Time evolution: two-site TDVP (htn_bond_evolve / htn_site_evolve / htn_tdvp2_sweep).  A bond step is
// update_bond with Backend::krylov_expm in the place of the eigen-solve, the backward step the one-site apply of update_site
// (direction 0) under the same exponential; the state stays normalised and the growth factors are handed out as logarithms.
// =====================================================================================================================
int htn_mps::evolve_checks(const htn_sweep_opts& o, const char* who) const {
    if (ctx->world > 1 || ctx->shard || ctx->exch || be->has_comm())
        return set_error("%s: time evolution on a context with a communicator or an exchange hook is not supported", who);
    if (!orth.empty()) return set_error("%s: time evolution of a state with attached orthogonal states is not supported", who);
    if (Llay[0]->size != 0 || Rlay[L]->size != 0)
        return set_error("%s: time evolution of a chain with boundary environments (an iDMRG window) is not supported", who);
    if (o.krylovdim < 2 || o.krylovdim > 31) return set_error("%s: krylovdim = %d (must be in 2..31)", who, o.krylovdim);
    return 0;
}

int htn_mps::evolve_site(int i, cplx dt, const htn_sweep_opts& o, htn_bond_stats* st, double* log_growth) {
    if (evolve_checks(o, "htn_site_evolve") || site1_checks(this, i, "htn_site_evolve")) return 1;
    StageClock clk(be, o.profile);
    const SiteLayoutP lay = site_lay[i];
    if (lay->size <= 0) return set_error("htn_site_evolve: empty site tensor on site %d", i);
    SiteWork w;
    if (site_solve(i, *lay, *lay, true, &dt, o, clk, w)) return 1;
    const Solve& s = w.sol;
    site_buf[i] = w.out;
    norm_absorbed();
    if (log_growth) *log_growth += log(s.growth);
    if (st) fill_stats(st, i, 0, s, Llay[i]->size + Rlay[i + 1]->size, 0, 0, 0.0, clk);
    return 0;
}

int htn_mps::tdvp2_sweep(cplx dt, const htn_sweep_opts& o, htn_bond_stats* st, double* E, double* log_norm) {
    if (evolve_checks(o, "htn_tdvp2_sweep")) return 1;
    if (L < 2) return set_error("htn_tdvp2_sweep: a chain of %d site(s) has no bond to sweep over", L);
    if (centre != 0) return set_error("htn_tdvp2_sweep: the centre is on site %d, not on site 0", centre);
    const cplx half = 0.5 * dt, back = -0.5 * dt;
    double lg = 0.0;
    htn_bond_stats site_st;
    int k = 0;
    auto bond = [&](int i, int direction, bool right, int site) -> int {
        htn_bond_stats* rec = st ? st + k : nullptr;
        ++k;
        if (update_bond(i, direction, right, true, o, rec, &half, &lg)) return 1;
        if (site < 0) return 0;
        if (evolve_site(site, back, o, rec ? &site_st : nullptr, &lg)) return 1;
        if (rec) rec->n_matvec += site_st.n_matvec, rec->t_total += site_st.t_total, rec->t_lanczos += site_st.t_lanczos;
        return 0;
    };
    for (int i = 0; i < L - 1; ++i)
        if (bond(i, +1, true, i < L - 2 ? i + 1 : -1)) return 1;
    for (int i = L - 2; i >= 0; --i)
        if (bond(i, -1, false, i > 0 ? i : -1)) return 1;
    if (E) *E = energy;
    if (log_norm) *log_norm = lg;
    return 0;
}

// =====================================================================================================================
// Time evolution at fixed bond tables: one-site TDVP (htn_site_evolve_move / htn_tdvp1_sweep).  A move is
// the one-site exponential of evolve_site, the QR / LQ gauge move of update_site, and -- before the triangular factor C goes
// into the neighbour -- the backward step C <- exp(-i dt_back H_eff0) C on the bond, H_eff0 = GL_b . GR_b with the left
// environment that already holds the new isometry (plan_apply0).  C is the Krylov row 0 of that solve where the QR wrote it.
// =====================================================================================================================
// what the zero-site apply of bond b asks of the state: the centre next to the bond, both environments on the bond's table
int htn_mps::bond0_checks(int b, const char* who) const {
    if (b < 1 || b >= L) return set_error("%s: bond %d out of range (1..%d)", who, b, L - 1);
    if (centre != b - 1 && centre != b) return set_error("%s: the centre is on site %d, not next to bond %d", who, centre, b);
    if (!Llay[b] || !Rlay[b] || Llay[b]->bond->key != bonds[b]->key || Rlay[b]->bond->key != bonds[b]->key)
        return set_error("%s: bond %d does not have both environments on its bond table", who, b);
    return 0;
}

int htn_mps::evolve_site_move(int i, int direction, cplx dt_fwd, cplx dt_back, const htn_sweep_opts& o, htn_bond_stats* st,
                              double* log_growth) {
    const char* who = "htn_site_evolve_move";
    if (evolve_checks(o, who) || site1_checks(this, i, who)) return 1;
    if (direction != -1 && direction != 1) return set_error("%s: direction %d (must be -1 or +1)", who, direction);
    if ((direction > 0 && i + 1 >= L) || (direction < 0 && i == 0)) return set_error("%s: site %d has no neighbour in direction %d", who, i, direction);
    StageClock clk(be, o.profile);
    const SiteLayoutP cur = site_lay[i];
    const SiteLayoutP lay = site_layout(direction > 0 ? 'L' : 'R', bonds[i], bonds[i + 1]);
    if (lay->size <= 0) return set_error("%s: empty site tensor on site %d", who, i);
    for (const auto& M : lay->mats)      // a full-rank gauge move needs the long side along the orthonormal direction
        if (lay->kind == 'L' ? M.rows < M.cols : M.cols < M.rows)
            return set_error("%s: sector (%d, %d) of site %d is a %d x %d block, its bond is wider than the rest of the "
                             "site supports: run a two-site sweep first", who, M.c.N, M.c.j, i, M.rows, M.cols);
    const int j = i + direction, b = direction > 0 ? i + 1 : i;
    const SiteLayoutP nl = site_lay[j];
    if (nl->kind != (direction > 0 ? 'R' : 'L')) return set_error("%s: site %d is not in %s layout", who, j, direction > 0 ? "right" : "left");
    auto gc = cached<Gauge1C>(std::string(direction > 0 ? "gauge1R" : "gauge1L") + lay->bl->key + "|" + lay->br->key + "|" +
                                  (direction > 0 ? nl->br->key : nl->bl->key),
                              [&]() -> std::shared_ptr<Gauge1C> {
                                  auto g = std::make_shared<Gauge1C>();
                                  Tasks t;
                                  plan_gauge1(*lay, *nl, g->desc, g->rsize, t);
                                  if (!(g->desc_dev = upload_vec(be, g->desc)) || upload_tasks(t, g->absorb)) return nullptr;
                                  return g;
                              });
    if (!gc) return 1;
    // the triangular factors are in bond layout only if the site reaches every sector of the bond (any state a two-site sweep shaped)
    int64_t n0 = 0;
    for (int d : bonds[b]->dims) n0 += (int64_t)d * d;
    if (gc->desc.size() != bonds[b]->secs.size() || gc->rsize != n0)
        return set_error("%s: site %d does not reach every sector of bond %d: run a two-site sweep first", who, i, b);
    // ---- forward step on the site ----
    SiteWork w;
    if (site_solve(i, *cur, *lay, true, &dt_fwd, o, clk, w)) return 1;             // (laps clk.plan and clk.lanczos)
    const Solve& s = w.sol;
    // ---- gauge move: Q stays on the site, C = R (or L) is row 0 of the bond's Krylov basis ----
    const int kd = o.krylovdim;
    DView V0 = zalloc((int64_t)(kd + 2) * n0, false), nb_out = zalloc(nl->size, false);
    if (!V0.base || !nb_out.base) return set_error("device allocation failed (gauge move)");
    if (be->qr_blocks(w.out.ptr(), V0.ptr(), (const htn_qr_block*)gc->desc_dev->p, gc->desc.data(), (int)gc->desc.size())) return 1;
    site_lay[i] = lay;
    site_buf[i] = w.out;
    clk.lap();                           // (the QR / LQ and, below, the absorption: t_svd is what the other stages leave of the total)
    if (direction > 0 ? left_env(i) : right_env(i)) return 1;
    clk.env = clk.lap();
    // ---- backward step on the bond ----
    Solve s0;
    s0.n = n0;
    s0.ap = make_apply0(b);
    if (!s0.ap) return 1;
    DView z0 = zalloc(s0.ap->zsize, false);
    if (!z0.base) return set_error("device allocation failed (zero-site apply)");
    htn_gemm_launch stages[2];
    const int ns = apply_stages(*s0.ap, Lbuf[b], Rbuf[b], z0, stages);
    if (ns < 0) return 1;
    if (be->krylov_expm(stages, ns, BUF_X, BUF_Y, V0.ptr(), n0, kd, dt_back.real(), dt_back.imag(), o.lanczos_tol, o.maxrestart, 0, nullptr,
                        ctx, &s0.growth, &s0.E, &s0.nmv, &s0.res, be->timing ? &s0.mv_ms : nullptr))
        return 1;
    clk.lanczos += clk.lap();
    // ---- the evolved C goes into the neighbour, which becomes the centre ----
    if (gemm(gc->absorb, {{BUF_S1, V0.ptr()}, {BUF_S2, site_buf[j].ptr()}, {BUF_Y, nb_out.ptr()}})) return 1;
    site_buf[j] = nb_out;
    centre = j;
    energy = s.E;
    norm_absorbed();
    if (log_growth) *log_growth += log(s.growth) + log(s0.growth);
    if (st) {
        fill_stats(st, b, direction, s, Llay[i]->size + Rlay[i + 1]->size, 0, 0, 0.0, clk);
        st->n_matvec += s0.nmv;
    }
    return 0;
}

int htn_mps::tdvp1_sweep(cplx dt, const htn_sweep_opts& o, htn_bond_stats* st, double* E, double* log_norm) {
    if (evolve_checks(o, "htn_tdvp1_sweep")) return 1;
    if (L < 2) return set_error("htn_tdvp1_sweep: a chain of %d site(s) has no bond to sweep over", L);
    if (centre != 0) return set_error("htn_tdvp1_sweep: the centre is on site %d, not on site 0", centre);
    const cplx half = 0.5 * dt, back = -0.5 * dt;
    double lg = 0.0;
    int k = 0;
    for (int i = 0; i < L - 1; ++i, ++k)
        if (evolve_site_move(i, +1, half, back, o, st ? st + k : nullptr, &lg)) return 1;
    for (int i = L - 1; i >= 1; --i, ++k)          // (site L-1: its two forward half steps as one solve of length dt)
        if (evolve_site_move(i, -1, i == L - 1 ? dt : half, back, o, st ? st + k : nullptr, &lg)) return 1;
    htn_bond_stats site_st;
    if (evolve_site(0, half, o, &site_st, &lg)) return 1;
    energy = site_st.energy;
    if (st) {
        htn_bond_stats* rec = st + k - 1;
        rec->n_matvec += site_st.n_matvec, rec->t_total += site_st.t_total, rec->t_lanczos += site_st.t_lanczos;
    }
    if (E) *E = energy;
    if (log_norm) *log_norm = lg;
    return 0;
}

// =====================================================================================================================
// Correction-vector sweeps (htn_bond_solve / htn_cv_sweep).  A bond step is update_bond with
// Backend::krylov_solve in the place of the eigen-solve: (z - H_eff) theta = p, p the row the attached-state machinery forms for
// the ONE attached state b (times its amplitude, before any orthonormalisation), started from the state as it is.  The tensors
// stay normalised; the norm of the last solution is the state's amplitude.
// =====================================================================================================================
int htn_mps::cv_checks(const htn_sweep_opts& o, const char* who) const {
    if (ctx->world > 1 || ctx->shard || ctx->exch || be->has_comm())
        return set_error("%s: a correction-vector solve on a context with a communicator or an exchange hook is not supported", who);
    if (orth.size() != 1)
        return set_error("%s: the state has %d attached state(s): exactly one is read as the right-hand side (htn_mps_set_orthogonal)", who,
                         (int)orth.size());
    if (Llay[0]->size != 0 || Rlay[L]->size != 0)
        return set_error("%s: a chain with boundary environments (an iDMRG window) is not supported", who);
    if (o.krylovdim < 2 || o.krylovdim > 31) return set_error("%s: krylovdim = %d (must be in 2..31)", who, o.krylovdim);
    return 0;
}

int htn_mps::cv_sweep(cplx z, const htn_sweep_opts& o, htn_bond_stats* st, double* cv_out) {
    if (cv_checks(o, "htn_cv_sweep")) return 1;
    if (L < 2) return set_error("htn_cv_sweep: a chain of %d site(s) has no bond to sweep over", L);
    if (centre != 0) return set_error("htn_cv_sweep: the centre is on site %d, not on site 0", centre);
    int k = 0;
    for (int i = 0; i < L - 1; ++i, ++k)
        if (update_bond(i, +1, true, false, o, st ? st + k : nullptr, nullptr, nullptr, &z, cv_out)) return 1;
    for (int i = L - 2; i >= 0; --i, ++k)
        if (update_bond(i, -1, false, false, o, st ? st + k : nullptr, nullptr, nullptr, &z, cv_out)) return 1;
    return 0;
}
