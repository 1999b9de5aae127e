// Infinite-chain growth loop around the two-site sweep, behind htn_idmrg_* (include/hubbardtn_hip.h).  Host C++ (no HIP).
// NOT a translation unit of its own: #included by htn_engine.cpp (one unit, see its head); never name it on a build line.
#include "htn_engine.h"

// =====================================================================================================================
// IDMRG2 growth driver (htn_idmrg_*): hubbardtn_amd/idmrg.py's idmrg2 / _absorb, rule for rule, with the boundary
// environments and the site tensors kept on the device from one step to the next.  Per step the host sees the
// singular values of the bond updates (as in every sweep), the centre spectrum, the scalars and the n_c x n_c products
// B''_T B'_T^H of the centre bond whose polar factors D^H are taken on the host (small; one-sided Jacobi below).
// =====================================================================================================================
namespace {

typedef std::map<Sec, std::vector<double>> SecVals;

// unitary polar factor P = U V^H of the n x n column-major matrix M (M = U S V^H), by one-sided Jacobi on the columns of
// M; directions of numerically zero weight get an orthonormal completion (Gram-Schmidt over the unit vectors)
void polar_factor(int n, const cplx* M, cplx* P) {
    std::vector<cplx> G(M, M + (size_t)n * n), J((size_t)n * n, cplx(0.0, 0.0));
    for (int i = 0; i < n; ++i) J[(size_t)i * n + i] = 1.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                cplx* gp = &G[(size_t)p * n];
                cplx* gq = &G[(size_t)q * n];
                double a = 0.0, b = 0.0;
                cplx g = 0.0;
                for (int i = 0; i < n; ++i) {
                    a += std::norm(gp[i]);
                    b += std::norm(gq[i]);
                    g += std::conj(gp[i]) * gq[i];
                }
                const double ag = std::abs(g);
                if (!(ag > 1e-15 * sqrt(a * b)) || ag == 0.0) continue;
                rotated = true;
                const cplx e = g / ag;
                const double zeta = (b - a) / (2.0 * ag);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                auto rot = [&](cplx* xp, cplx* xq) {             // [x_p, x_q] <- [x_p, x_q] [[c, s e], [-s conj(e), c]]
                    for (int i = 0; i < n; ++i) {
                        const cplx u = xp[i], v = xq[i];
                        xp[i] = c * u - s * std::conj(e) * v;
                        xq[i] = s * e * u + c * v;
                    }
                };
                rot(gp, gq);
                rot(&J[(size_t)p * n], &J[(size_t)q * n]);
            }
        if (!rotated) break;
    }
    std::vector<double> nrm(n);
    double nmax = 0.0;
    for (int j = 0; j < n; ++j) {
        double a = 0.0;
        for (int i = 0; i < n; ++i) a += std::norm(G[(size_t)j * n + i]);
        nrm[j] = sqrt(a);
        nmax = std::max(nmax, nrm[j]);
    }
    std::vector<char> have(n, 0);
    for (int j = 0; j < n; ++j)
        if (nrm[j] > 1e-13 * nmax && nrm[j] > 0.0) {
            for (int i = 0; i < n; ++i) G[(size_t)j * n + i] /= nrm[j];
            have[j] = 1;
        }
    int unit = 0;
    for (int j = 0; j < n; ++j) {
        if (have[j]) continue;
        cplx* u = &G[(size_t)j * n];
        for (; unit < n; ++unit) {
            for (int i = 0; i < n; ++i) u[i] = i == unit ? 1.0 : 0.0;
            for (int pass = 0; pass < 2; ++pass)
                for (int q = 0; q < n; ++q) {
                    if (!have[q]) continue;
                    const cplx* v = &G[(size_t)q * n];
                    cplx d = 0.0;
                    for (int i = 0; i < n; ++i) d += std::conj(v[i]) * u[i];
                    for (int i = 0; i < n; ++i) u[i] -= d * v[i];
                }
            double a = 0.0;
            for (int i = 0; i < n; ++i) a += std::norm(u[i]);
            if (a > 1e-2) {
                const double f = 1.0 / sqrt(a);
                for (int i = 0; i < n; ++i) u[i] *= f;
                ++unit;
                break;
            }
        }
        have[j] = 1;
    }
    for (int b = 0; b < n; ++b)
        for (int a = 0; a < n; ++a) {
            cplx acc = 0.0;
            for (int j = 0; j < n; ++j) acc += G[(size_t)j * n + a] * std::conj(J[(size_t)j * n + b]);
            P[(size_t)b * n + a] = acc;
        }
}

// 1 / sigma where sigma is not numerically zero (relative to the sector's largest value), else 0 (idmrg._absorb's inv)
std::vector<double> inv_values(const std::vector<double>& v) {
    double mx = 0.0;
    for (double x : v) mx = std::max(mx, x);
    const double thr = 1e-13 * std::max(mx, 1e-300);
    std::vector<double> r(v.size());
    for (size_t i = 0; i < v.size(); ++i) r[i] = v[i] > thr ? 1.0 / std::max(v[i], 1e-300) : 0.0;
    return r;
}

// output tiles (<= 32 x 32) of one m x n block, all reading the segment range [seg_begin, seg_begin + seg_count)
void add_block_tiles(Tasks& t, int64_t c_off, int ldc, int m, int n, int seg_begin, int seg_count) {
    for (int c0 = 0; c0 < n; c0 += HTN_TILE)
        for (int r0 = 0; r0 < m; r0 += HTN_TILE) {
            htn_tile tl;
            memset(&tl, 0, sizeof(tl));
            tl.c_off = c_off;
            tl.buf_c = BUF_Y;
            tl.ldc = ldc;
            tl.m = std::min(HTN_TILE, m - r0);
            tl.n = std::min(HTN_TILE, n - c0);
            tl.row0 = r0;
            tl.col0 = c0;
            tl.seg_begin = seg_begin;
            tl.seg_count = seg_count;
            t.tiles.push_back(tl);
        }
    t.ntiles = (int32_t)t.tiles.size();
}
int add_gemm_seg(Tasks& t, int64_t a_off, int lda, int op_a, int64_t b_off, int ldb, int op_b, int k, int m, int n) {
    htn_seg sg;
    memset(&sg, 0, sizeof(sg));
    sg.a_off = a_off;
    sg.b_off = b_off;
    sg.buf_a = BUF_S1;
    sg.buf_b = BUF_S2;
    sg.lda = lda;
    sg.ldb = ldb;
    sg.k = k;
    sg.op_a = op_a;
    sg.op_b = op_b;
    sg.type = HTN_SEG_GEMM;
    sg.alpha_re = 1.0;
    t.segs.push_back(sg);
    t.nsegs = (int32_t)t.segs.size();
    t.flops += 8 * (int64_t)m * n * k;
    return t.nsegs - 1;
}

}  // namespace

struct htn_idmrg {
    htn_ctx* ctx = nullptr;
    htn_mpo* mpo = nullptr;
    Backend* be = nullptr;
    htn_idmrg_opts o;
    htn_sweep_opts so;                 // normalised sweep options of every window update
    int T = 0, W = 0, dNw = 0;
    BondP bL, bR;                      // tables the next window must have at its ends
    DView Lenv, Renv;                  // their boundary environments (device; shared with the windows, never written)
    htn_mps* win = nullptr;            // current window
    htn_mps* guess = nullptr;          // predicted next window (nullptr: the host supplies one)
    bool have_carry = true;            // sigma_0 / D_prev of the next prediction (idmrg._absorb's carry)
    SecVals carry_sig;
    std::map<Sec, std::vector<cplx>> carry_D;
    bool have_prev = false;
    double E_prev = 0.0, delta_prev = INFINITY;
    Spectrum spec_prev;
    int step = 0, stall = 0;
    bool finished = false, failed = false;

    const Sym& sym() const { return mpo->mpo.sym; }
    Sec sh(Sec c) const { return {sym().wrapN(c.N + dNw), c.j}; }
    BondP shifted(const Bond& b) const {
        std::vector<std::pair<Sec, int>> items;
        for (size_t k = 0; k < b.secs.size(); ++k) items.push_back({sh(b.secs[k]), b.dims[k]});
        return std::make_shared<Bond>(items);
    }
    SecVals tilde(int b) const {       // Schmidt values of bond b of the window in the Euclidean normalisation
        SecVals r;
        auto it = win->spectra.find(b);
        if (it == win->spectra.end()) return r;
        for (size_t k = 0; k < it->second.secs.size(); ++k) {
            std::vector<double> v = it->second.vals[k];
            const double f = sqrt((double)sym().qdim(it->second.secs[k]));
            for (double& x : v) x *= f;
            r[it->second.secs[k]] = std::move(v);
        }
        return r;
    }
    double distance(const Spectrum& a, const Spectrum& b, int dN) const;     // idmrg._spectrum_distance
    int check_end(const Bond& got, const Bond& want, int bond, const char* side) const;
    int absorb(bool predict);
    int predict(const std::vector<BondP>& ob, const std::vector<DView>& A, const std::vector<SiteLayoutP>& Alay,
                const std::vector<SecVals>& sig, const DView& CT, const SiteLayoutP& CTlay, const std::vector<DView>& Bs,
                const std::vector<SiteLayoutP>& Bslay, const SecVals& sig0, const std::map<Sec, std::vector<cplx>>& Dprev,
                const std::map<Sec, std::vector<cplx>>& Dnew);
    int run_step(const int32_t* bond_ptr, const htn_sector* sectors, const int32_t* sub_ptr, const htn_subblock* subs,
                 const int64_t* data_ptr, const void* data, htn_idmrg_stats* st);
};

double htn_idmrg::distance(const Spectrum& a, const Spectrum& b, int dN) const {
    std::map<Sec, std::pair<const std::vector<double>*, const std::vector<double>*>> keys;
    for (size_t k = 0; k < a.secs.size(); ++k) keys[a.secs[k]].first = &a.vals[k];
    for (size_t k = 0; k < b.secs.size(); ++k) keys[{b.secs[k].N - dN, b.secs[k].j}].second = &b.vals[k];
    double d2 = 0.0;
    for (auto& kv : keys) {
        const size_t nx = kv.second.first ? kv.second.first->size() : 0, ny = kv.second.second ? kv.second.second->size() : 0;
        double s = 0.0;
        for (size_t i = 0; i < std::max(nx, ny); ++i) {
            const double x = i < nx ? (*kv.second.first)[i] : 0.0, y = i < ny ? (*kv.second.second)[i] : 0.0;
            s += (x - y) * (x - y);
        }
        d2 += sym().qdim(kv.first) * s;
    }
    return sqrt(d2);
}

int htn_idmrg::check_end(const Bond& got, const Bond& want, int bond, const char* side) const {
    if (got.key == want.key) return 0;
    std::map<Sec, std::pair<int, int>> all;
    for (size_t k = 0; k < got.secs.size(); ++k) all[got.secs[k]].first = got.dims[k];
    for (size_t k = 0; k < want.secs.size(); ++k) all[want.secs[k]].second = want.dims[k];
    for (auto& kv : all)
        if (kv.second.first != kv.second.second)
            return set_error("htn_idmrg_step: bond %d of the window, sector (N, j) = (%d, %d): %d multiplets, the %s boundary "
                             "(htn_idmrg_boundary) has %d", bond, kv.first.N, kv.first.j, kv.second.first, side, kv.second.second);
    return set_error("htn_idmrg_step: bond %d of the window differs from the %s boundary", bond, side);
}

// absorb the halves of the converged window (centre on site 0) into the boundaries and, with `want`, predict the next
// window: idmrg._absorb.  The window is left as the non-optimising moves leave it.
int htn_idmrg::absorb(bool want) {
    htn_mps* w = win;
    const htn_sweep_opts& mo = so;                           // (the run's own truncation: the state already satisfies it)
    for (int i = 0; i < T; ++i)                              // centre 0 -> T
        if (w->update_bond(i, +1, true, false, mo, nullptr)) return 1;
    std::vector<DView> A(w->site_buf.begin(), w->site_buf.begin() + T);
    std::vector<SiteLayoutP> Alay(w->site_lay.begin(), w->site_lay.begin() + T);
    std::vector<SecVals> sig(T + 1);                         // sig[0]: the carry's
    for (int k = 1; k <= T; ++k) sig[k] = tilde(k);
    const DView CT = w->site_buf[T];                         // sigma_T B'_T
    const SiteLayoutP CTlay = w->site_lay[T];
    std::vector<DView> Bs(w->site_buf.begin() + T + 1, w->site_buf.end());
    std::vector<SiteLayoutP> Bslay(w->site_lay.begin() + T + 1, w->site_lay.end());
    const DView Lnew = w->Lbuf[T];
    const BondP bLn = w->Llay[T]->bond;
    const std::vector<BondP> ob = w->bonds;
    if (w->update_bond(T - 1, +1, false, false, mo, nullptr)) return 1;      // centre back to T-1: B''_T, right env on T
    const DView B2 = w->site_buf[T];
    const SiteLayoutP B2lay = w->site_lay[T];
    const DView Rnew = w->Rbuf[T];
    const BondP bRt = w->Rlay[T]->bond;
    Lenv = Lnew;
    bL = bLn;
    Renv = Rnew;                                             // relabelled N -> N + dNw: same blocks, same order, same buffer
    bR = shifted(*bRt);
    const bool old_carry = have_carry;
    const SecVals sig0 = carry_sig;
    const std::map<Sec, std::vector<cplx>> Dprev = carry_D;
    bool ok = bRt->key == bLn->key && B2lay->bl->key == CTlay->bl->key && B2lay->br->key == CTlay->br->key;
    for (size_t k = 0; ok && k < bLn->secs.size(); ++k) {
        auto it = sig[T].find(bLn->secs[k]);
        ok = it != sig[T].end() && (int)it->second.size() == bLn->dims[k];
    }
    if (!ok) {
        have_carry = false;
        carry_sig.clear();
        carry_D.clear();
        return 0;
    }
    // D^H = polar factor of B''_T B'_T^H per left sector c, B'_T = sigma_T^-1 C_T: acc_c = B''_c C_c^H (one GEMM per sector on
    // the device, R layout = one [n_c ; (s, r)] matrix per sector), columns scaled by sigma_T^-1 and factorised on the host
    Tasks t;
    std::vector<int64_t> aoff(bLn->secs.size());
    int64_t asz = 0;
    for (size_t q = 0; q < bLn->secs.size(); ++q) {
        const int n = bLn->dims[q];
        aoff[q] = asz;
        asz += (int64_t)n * n;
        const int mi = CTlay->mat(bLn->secs[q]), mb = B2lay->mat(bLn->secs[q]);
        if (mi < 0 || mb < 0) {
            add_block_tiles(t, aoff[q], n, n, n, 0, 0);      // (no blocks: zero)
            continue;
        }
        const auto &mc = CTlay->mats[mi], &m2 = B2lay->mats[mb];
        const int sidx = add_gemm_seg(t, m2.off, n, HTN_OP_N, mc.off, n, HTN_OP_C, m2.cols, n, n);
        add_block_tiles(t, aoff[q], n, n, n, sidx, 1);
    }
    DevTasks dt;
    DView acc = w->zalloc(asz, true);
    if (!acc.base) return set_error("htn_idmrg_step: device allocation failed (centre products)");
    if (w->upload_tasks(t, dt) || w->gemm(dt, {{BUF_S1, B2.ptr()}, {BUF_S2, CT.ptr()}, {BUF_Y, acc.ptr()}})) return 1;
    std::vector<cplx> acc_h((size_t)std::max<int64_t>(asz, 1));
    if (be->download(acc_h.data(), acc.ptr(), sizeof(cplx) * (size_t)asz)) return 1;
    std::map<Sec, std::vector<cplx>> Dnew;
    for (size_t q = 0; q < bLn->secs.size(); ++q) {
        const int n = bLn->dims[q];
        const std::vector<double> inv = inv_values(sig[T][bLn->secs[q]]);
        cplx* m = acc_h.data() + aoff[q];
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) m[i + (size_t)j * n] *= inv[j];
        std::vector<cplx> P((size_t)n * n);
        polar_factor(n, m, P.data());
        Dnew[bLn->secs[q]] = std::move(P);
    }
    have_carry = true;
    carry_sig = sig[T];
    carry_D = Dnew;
    if (!old_carry || !want) return 0;
    return predict(ob, A, Alay, sig, CT, CTlay, Bs, Bslay, sig0, Dprev, Dnew);
}

// the next window [sigma B'_T] B_{T+1} .. B_{2T-1} . [D_prev^H sigma_0^-1 A_0 sigma_1] .. [sigma_{T-1}^-1 A_{T-1} sigma_T D],
// built on the device; refusals (no prediction, the host supplies the next window) as in idmrg._absorb
int htn_idmrg::predict(const std::vector<BondP>& ob, const std::vector<DView>& A, const std::vector<SiteLayoutP>& Alay,
                       const std::vector<SecVals>& sig_in, const DView& CT, const SiteLayoutP& CTlay, const std::vector<DView>& Bs,
                       const std::vector<SiteLayoutP>& Bslay, const SecVals& sig0, const std::map<Sec, std::vector<cplx>>& Dprev,
                       const std::map<Sec, std::vector<cplx>>& Dnew) {
    std::vector<SecVals> sig = sig_in;
    sig[0] = sig0;
    std::vector<BondP> nb(W + 1);
    nb[0] = bL;
    for (int k = 1; k <= T; ++k) {
        nb[k] = ob[T + k];
        nb[T + k] = shifted(*ob[k]);
    }
    if (nb[T]->key != shifted(*ob[0])->key || nb[W]->key != bR->key) return 0;
    for (size_t k = 0; k < ob[0]->secs.size(); ++k) {
        auto it = sig0.find(ob[0]->secs[k]);
        if (it == sig0.end() || (int)it->second.size() != ob[0]->dims[k]) return 0;
    }
    for (int k = 0; k < T; ++k)
        for (const Key& key : Alay[k]->bkeys)
            if (!sig[k].count({key[0], key[1]}) || !sig[k + 1].count({key[3], key[4]})) return 0;
    for (auto& c : ob[0]->secs)
        if (!Dprev.count(c)) return 0;
    if (CTlay->bl->key != nb[0]->key || CTlay->br->key != nb[1]->key) return 0;
    MpsGuard g{mps_new(ctx, mpo)};
    htn_mps* e = g.p;
    e->bonds = nb;
    e->site_lay[0] = CTlay;
    e->site_buf[0] = CT;
    for (int k = 1; k < T; ++k) {
        e->site_lay[k] = Bslay[k - 1];
        e->site_buf[k] = Bs[k - 1];
    }
    for (int k = 0; k < T; ++k) {
        const SiteLayoutP lay = e->site_layout('R', nb[T + k], nb[T + k + 1]);
        const SiteLayout& al = *Alay[k];
        // sigma scalings: rows by sigma_k^-1 into tmp, columns by sigma_{k+1} into x (L layout -> R layout, labels shifted)
        std::vector<double> scl;
        std::vector<htn_copy_item> rows, cols;
        std::vector<std::pair<int, int>> pairs;              // (A block, new block)
        for (size_t q = 0; q < al.bkeys.size(); ++q) {
            const Key& key = al.bkeys[q];
            const Sec l{key[0], key[1]}, r{key[3], key[4]};
            const int bi = lay->block(sh(l), key[2], sh(r));
            if (bi < 0) continue;
            const BlockRec &src = al.blocks[q], &dst = lay->blocks[bi];
            htn_copy_item it = copy_item(dst.off, dst.ld, src.off, src.ld, dst.m, dst.n);
            it.scale_dim = 0;
            it.scl_off = (int64_t)scl.size();
            const std::vector<double> inv = inv_values(sig[k].at(l));
            scl.insert(scl.end(), inv.begin(), inv.end());
            rows.push_back(it);
            it.src_off = dst.off;
            it.lds = dst.ld;
            it.scale_dim = 1;
            it.scl_off = (int64_t)scl.size();
            const std::vector<double>& sr = sig[k + 1].at(r);
            scl.insert(scl.end(), sr.begin(), sr.end());
            cols.push_back(it);
            pairs.push_back({(int)q, bi});
        }
        std::vector<htn_copy_item> items(rows);
        items.insert(items.end(), cols.begin(), cols.end());
        DBufP items_d = upload_vec(be, items), scl_d = upload_vec(be, scl);
        DView tmp = e->zalloc(lay->size, true), x = e->zalloc(lay->size, true);
        if (!items_d || !scl_d || !tmp.base || !x.base) return set_error("htn_idmrg_step: device allocation failed (prediction)");
        const htn_copy_item* itd = (const htn_copy_item*)items_d->p;
        if (!rows.empty() && (be->batched_copy(tmp.ptr(), A[k].ptr(), nullptr, (const double*)scl_d->p, itd, (int)rows.size(), 1.0) ||
                              be->batched_copy(x.ptr(), tmp.ptr(), nullptr, (const double*)scl_d->p, itd + rows.size(), (int)cols.size(), 1.0)))
            return 1;
        if (k == 0) {                                        // D_prev^H from the left, per left sector (one R-layout matrix each)
            std::vector<cplx> dh;
            Tasks t;
            for (const Sec& l : ob[0]->secs) {
                const int mi = lay->mat(sh(l));
                if (mi < 0) continue;
                const auto& m = lay->mats[mi];
                if (m.rows == 0 || m.cols == 0) continue;
                const std::vector<cplx>& D = Dprev.at(l);
                const int sidx = add_gemm_seg(t, (int64_t)dh.size(), m.rows, HTN_OP_N, m.off, m.rows, HTN_OP_N, m.rows, m.rows, m.cols);
                dh.insert(dh.end(), D.begin(), D.end());
                add_block_tiles(t, m.off, m.rows, m.rows, m.cols, sidx, 1);
            }
            DBufP dd = upload_vec(be, dh);
            DView y = e->zalloc(lay->size, true);
            DevTasks dt;
            if (!dd || !y.base) return set_error("htn_idmrg_step: device allocation failed (prediction)");
            if (t.ntiles && (e->upload_tasks(t, dt) || e->gemm(dt, {{BUF_S1, dd->p}, {BUF_S2, x.ptr()}, {BUF_Y, y.ptr()}}))) return 1;
            x = y;
        }
        if (k == T - 1) {                                    // D from the right, per block (right sector r of bond T)
            std::vector<cplx> dh;
            std::map<Sec, int64_t> doff;
            for (auto& kv : Dnew) {
                doff[kv.first] = (int64_t)dh.size();
                dh.insert(dh.end(), kv.second.begin(), kv.second.end());
            }
            Tasks t;
            for (auto& pr : pairs) {
                const Key& key = al.bkeys[pr.first];
                const Sec r{key[3], key[4]};
                auto it = doff.find(r);
                if (it == doff.end()) return 0;
                const BlockRec& b = lay->blocks[pr.second];
                if (b.m == 0 || b.n == 0) continue;
                const int sidx = add_gemm_seg(t, b.off, b.ld, HTN_OP_N, it->second, b.n, HTN_OP_C, b.n, b.m, b.n);
                add_block_tiles(t, b.off, b.ld, b.m, b.n, sidx, 1);
            }
            DBufP dd = upload_vec(be, dh);
            DView y = e->zalloc(lay->size, true);
            DevTasks dt;
            if (!dd || !y.base) return set_error("htn_idmrg_step: device allocation failed (prediction)");
            if (t.ntiles && (e->upload_tasks(t, dt) || e->gemm(dt, {{BUF_S1, x.ptr()}, {BUF_S2, dd->p}, {BUF_Y, y.ptr()}}))) return 1;
            x = y;
        }
        e->site_lay[T + k] = lay;
        e->site_buf[T + k] = x;
    }
    if (mps_finish(e, nullptr, nullptr, &Lenv, &Renv)) return 1;
    guess = e;
    g.p = nullptr;
    return 0;
}

int htn_idmrg::run_step(const int32_t* bond_ptr, const htn_sector* sectors, const int32_t* sub_ptr, const htn_subblock* subs,
                        const int64_t* data_ptr, const void* data, htn_idmrg_stats* st) {
    htn_mps* w = nullptr;
    bool warm = false;
    if (bond_ptr) {
        if (!sectors || !sub_ptr || !subs || !data_ptr || !data) return set_error("htn_idmrg_step: incomplete window tables");
        MpsGuard g{mps_new(ctx, mpo)};
        if (mps_load_bonds(g.p, bond_ptr, sectors)) return 1;
        if (check_end(*g.p->bonds[0], *bL, 0, "left") || check_end(*g.p->bonds[W], *bR, W, "right")) return 1;
        if (mps_load_sites(g.p, sub_ptr, subs, data_ptr, data) || mps_finish(g.p, nullptr, nullptr, &Lenv, &Renv)) return 1;
        w = g.p;
        g.p = nullptr;
        if (guess) htn_mps_destroy(guess);
        guess = nullptr;
    } else {
        if (sectors || sub_ptr || subs || data_ptr || data) return set_error("htn_idmrg_step: incomplete window tables (bond_ptr is NULL)");
        if (!guess)
            return set_error("htn_idmrg_step: step %d needs a window from the host (needs_window was set), got NULL", step);
        w = guess;
        guess = nullptr;
        warm = true;
    }
    failed = true;                     // (until the step completes: a failed step leaves the driver unusable)
    if (win) htn_mps_destroy(win);
    win = w;
    // the window starts from a random state (or a prediction): sweep until its energy has settled
    int nsw = 0;
    double E_sw = 0.0;
    for (int k = 0; k < o.sweeps_per_step; ++k) {
        double E_new = 0.0;
        if (w->sweep(so, nullptr, &E_new)) return 1;
        ++nsw;
        if (k >= 1 && fabs(E_new - E_sw) <= (warm ? 1e-8 : 1e-11) * std::max(fabs(E_new), 1.0)) break;
        E_sw = E_new;
    }
    // energy of the grown system: <psi|H|psi> of the window as stored, at bond 0 without moving the centre
    htn_sweep_opts o0 = so;
    o0.cutoff = 0.0;
    htn_bond_stats bs;
    if (w->update_bond(0, +1, false, false, o0, &bs)) return 1;
    const double E = bs.energy;
    Spectrum spec;
    auto sit = w->spectra.find(T);
    if (sit != w->spectra.end()) spec = sit->second;
    double e_site = NAN, delta = INFINITY;
    if (have_prev) {
        e_site = (E - E_prev) / W;
        delta = distance(spec_prev, spec, sym().kind == HTN_SYM_SU2 ? 0 : dNw / 2);
    }
    const int it = step;
    const int32_t chi = (int32_t)w->bonds[T]->dim_full(sym());
    have_prev = true;
    E_prev = E;
    spec_prev = spec;
    const bool converged = it + 1 >= o.min_steps && delta < o.tol;
    finished = converged || it + 1 >= o.maxiter;
    if (!finished) {
        if (o.warm_start) {
            // a growth that neither converges nor moves gets a random window again; the second window always does
            if (it >= 1 && delta > 10.0 * o.tol && fabs(delta - delta_prev) <= 0.05 * delta)
                ++stall;
            else
                stall = 0;
            bool want = true;
            if (it == 0 || stall >= 2) {
                want = false;
                stall = 0;
            }
            if (absorb(want)) return 1;
        } else {
            Lenv = w->Lbuf[T];
            bL = w->Llay[T]->bond;
            Renv = w->Rbuf[T];
            bR = shifted(*w->Rlay[T]->bond);
        }
    }
    delta_prev = delta;
    ++step;
    failed = false;
    if (st) {
        memset(st, 0, sizeof(*st));
        st->step = it;
        st->sweeps = nsw;
        st->converged = converged;
        st->finished = finished;
        st->needs_window = finished ? 0 : guess == nullptr;
        st->chi_full = chi;
        st->energy = E;
        st->energy_per_site = e_site;
        st->delta = delta;
    }
    return be->sync();
}

void idmrg_free(htn_idmrg* d) {
    if (!d) return;
    htn_ctx* c = d->ctx;
    htn_mpo* m = d->mpo;
    if (c) (void)c->be->activate();
    if (d->guess) htn_mps_destroy(d->guess);
    if (d->win) htn_mps_destroy(d->win);
    d->Lenv = DView();
    d->Renv = DView();
    delete d;                          // device buffers first, then the references that keep the backend alive
    mpo_release(m);
    ctx_release(c);
}

// ---- what the entry points htn_idmrg_* forward to ---------------------------------------------------------------------
int idmrg_create(htn_ctx* ctx, const htn_mpo* mpo, const htn_idmrg_opts* opts, htn_idmrg** out) {
    if (!ctx || !mpo || !opts || !out) return set_error("htn_idmrg_create: NULL argument");
    const int T = opts->cell_sites;
    if (T < 1 || 2 * T != (int)mpo->mpo.sites.size())
        return set_error("htn_idmrg_create: cell_sites %d, but the window MPO has %d sites (2 T required)", T, (int)mpo->mpo.sites.size());
    if (opts->maxiter < 1 || opts->sweeps_per_step < 1) return set_error("htn_idmrg_create: maxiter and sweeps_per_step must be >= 1");
    if (ctx->be->activate()) return 1;
    htn_idmrg* d = new htn_idmrg();
    d->ctx = ctx;
    ++ctx->refs;
    d->mpo = const_cast<htn_mpo*>(mpo);
    ++d->mpo->refs;
    d->be = ctx->be.get();
    d->o = *opts;
    d->so = norm_opts(&opts->sweep);
    d->T = T;
    d->W = 2 * T;
    d->dNw = opts->window_dN;
    // step 0: the window alone between two empty blocks, one-sector boundary bonds and zero environments (only the
    // implicit identity level is non-zero)
    const Sym& sym = mpo->mpo.sym;
    d->bL = std::make_shared<Bond>(std::vector<std::pair<Sec, int>>{{Sec{0, 0}, 1}});
    d->bR = std::make_shared<Bond>(std::vector<std::pair<Sec, int>>{{Sec{sym.wrapN(d->dNw), 0}, 1}});
    const int64_t nl = build_env_layout(sym, 'L', d->bL, mpo->mpo.sites[0].left)->size;
    const int64_t nr = build_env_layout(sym, 'R', d->bR, mpo->mpo.sites[d->W - 1].right)->size;
    for (int side = 0; side < 2; ++side) {
        DView& v = side ? d->Renv : d->Lenv;
        const size_t bytes = sizeof(cplx) * (size_t)std::max<int64_t>(side ? nr : nl, 1);
        v.base = std::make_shared<DBuf>(d->be, bytes);
        if (!v.base->p || d->be->zero(v.base->p, bytes)) {
            idmrg_free(d);
            return v.base && v.base->p ? 1 : set_error("htn_idmrg_create: device allocation failed");
        }
    }
    d->carry_sig[Sec{0, 0}] = {1.0};
    d->carry_D[Sec{0, 0}] = {cplx(1.0, 0.0)};
    *out = d;
    return 0;
}
int32_t idmrg_boundary(const htn_idmrg* d, int32_t side, htn_sector* out) {
    if (!d || side < 0 || side > 1) return -1;
    const Bond& B = side ? *d->bR : *d->bL;
    if (out)
        for (size_t k = 0; k < B.secs.size(); ++k) out[k] = {B.secs[k].N, B.secs[k].j, B.dims[k]};
    return (int32_t)B.secs.size();
}
int idmrg_step(htn_idmrg* d, const int32_t* bond_ptr, const htn_sector* sectors, const int32_t* sub_ptr, const htn_subblock* subs,
               const int64_t* data_ptr, const void* data_host, htn_idmrg_stats* stats) {
    if (!d) return set_error("htn_idmrg_step: NULL handle");
    if (d->failed) return set_error("htn_idmrg_step: an earlier step failed; the driver cannot continue");
    if (d->finished) return set_error("htn_idmrg_step: the growth has finished (converged or maxiter)");
    if (d->be->activate()) return 1;
    return d->run_step(bond_ptr, sectors, sub_ptr, subs, data_ptr, data_host, stats);
}
int idmrg_window(htn_idmrg* d, htn_mps** out) {
    if (!d || !out) return set_error("htn_idmrg_window: NULL argument");
    if (!d->win) return set_error("htn_idmrg_window: no step has run yet");
    ++d->win->refs;
    *out = d->win;
    return 0;
}
