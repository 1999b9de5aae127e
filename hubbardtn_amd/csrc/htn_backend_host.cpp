// Host statements of the htn::Backend methods that are not pure (htn_core.h), and of the two kernel-level entries that have
// one (htn_krylov_expm_z, htn_krylov_solve_z, htn_qr_blocks_z, htn_block_nullproj_z): vectors downloaded, H applied through the backend's grouped_gemm, the arithmetic
// in plain C++.  The CPU baseline library runs them; the HIP backend overrides every one with its kernels.  Nothing here
// uses the sweep engine's types.  Host C++ (no HIP).
// NOT a translation unit of its own: #included by htn_engine.cpp (one unit, see its head); never name it on a build line.
#include <math.h>

#include <algorithm>

#include "htn_core.h"
#include "htn_expm.h"
#include "htn_resolvent.h"
#include "htn_tridiag.h"

using namespace htn;

namespace {
cplx hdot(const cplx* a, const cplx* b, int64_t n) {
    cplx s = 0.0;
    for (int64_t e = 0; e < n; ++e) s += std::conj(a[e]) * b[e];
    return s;
}
// w -= sum_r rows[r] <rows[r], w>, twice; returns the sum of <rows[pick], w> over both passes.  Out of line, as g++ -O3 kept it
// before the two callers shared a step: inlined into HostKrylov::extend its complex products contract to other FMAs
__attribute__((noinline)) double hproject(const std::vector<const cplx*>& rows, cplx* w, int64_t n, int pick) {
    double got = 0.0;
    std::vector<cplx> c(rows.size());
    for (int pass = 0; pass < 2; ++pass) {
        for (size_t r = 0; r < rows.size(); ++r) c[r] = hdot(rows[r], w, n);
        if (pick >= 0) got += c[(size_t)pick].real();
        for (size_t r = 0; r < rows.size(); ++r)
            for (int64_t e = 0; e < n; ++e) w[e] -= c[r] * rows[r][e];
    }
    return got;
}

// What lanczos_orth and krylov_expm share: host copies B of the basis rows (row 0 downloaded from the caller's V), H through
// the device rows kd (x) and kd + 1 (y) of V, one Lanczos step with full two-pass reorthogonalisation, the combination of the
// rows into the next start vector.  `who` prefixes the error strings.
struct HostKrylov {
    Backend* be;
    const char* who;
    const htn_gemm_launch* stages;
    int n_stages, x_slot, y_slot;
    cplx* Vd;
    int64_t n;
    int kd, zero_y;
    htn_exchange2_fn exchange;
    void* user;
    size_t bytes = sizeof(cplx) * (size_t)n;
    std::vector<cplx> B = std::vector<cplx>((size_t)(kd + 1) * n), x = std::vector<cplx>((size_t)n);
    int n_matvec = 0;
    cplx* row(int j) { return B.data() + (int64_t)j * n; }
    int matvec(const cplx* v, cplx* w) {
        cplx *xd = Vd + (int64_t)kd * n, *yd = Vd + (int64_t)(kd + 1) * n;
        if (be->upload(xd, v, bytes)) return 1;
        if (zero_y && be->zero(yd, bytes)) return 1;
        for (int s = 0; s < n_stages; ++s) {
            const void* bufs[HTN_MAX_BUFS];
            for (int b = 0; b < HTN_MAX_BUFS; ++b) bufs[b] = stages[s].bufs[b];
            bufs[x_slot] = xd;
            bufs[y_slot] = yd;
            if (stages[s].n_tiles > 0 && be->grouped_gemm(bufs, stages[s].tiles, stages[s].n_tiles, stages[s].segs)) return 1;
        }
        if (exchange && exchange(yd, n, user)) return set_error("%s: the exchange hook reported a failure", who);
        return be->download(w, yd, bytes);
    }
    // step j: row j + 1 = H row j, orthogonalised against `frozen` and the rows 0..j -> alpha_j, beta_j (row j + 1 not yet scaled)
    int extend(const std::vector<const cplx*>& frozen, int j, double* alpha, double* beta) {
        cplx* w = row(j + 1);
        if (matvec(row(j), w)) return 1;
        ++n_matvec;
        std::vector<const cplx*> rows = frozen;
        for (int r = 0; r <= j; ++r) rows.push_back(row(r));
        *alpha = hproject(rows, w, n, (int)frozen.size() + j);
        *beta = sqrt(hdot(w, w, n).real());
        if (!(*alpha == *alpha) || !(*beta == *beta)) return set_error("%s: NaN in the tridiagonal coefficients", who);
        return 0;
    }
    void accept(int j, double beta) {                 // the step goes on: row j + 1 becomes a unit vector
        cplx* w = row(j + 1);
        const double inv = 1.0 / beta;
        for (int64_t e = 0; e < n; ++e) w[e] *= inv;
    }
    template <class T>
    void combine(const std::vector<T>& c) {           // x = sum_r c_r B_r
        std::fill(x.begin(), x.end(), cplx(0.0, 0.0));
        for (size_t r = 0; r < c.size(); ++r)
            for (int64_t e = 0; e < n; ++e) x[(size_t)e] += c[r] * B[r * (size_t)n + (size_t)e];
    }
    void restart_from_x() { memcpy((void*)B.data(), x.data(), bytes); }
    int finish() { return be->upload(Vd, B.data(), bytes) || be->sync(); }
};
}  // namespace

int Backend::lanczos_orth(const htn_gemm_launch* stages, int n_stages, int x_slot, int y_slot, void* Vv, int64_t n, int kd, double tol,
                          int max_restart, int zero_y, htn_exchange2_fn exchange, void* user, const void* Qv, int nf, double* eig,
                          int* n_matvec, double* residual, double* matvec_ms) {
    if (kd < 2 || nf < 0) return set_error("lanczos_orth: krylovdim >= 2 and n_frozen >= 0 required");
    HostKrylov K{this, "lanczos_orth", stages, n_stages, x_slot, y_slot, (cplx*)Vv, n, kd, zero_y, exchange, user};
    std::vector<cplx> Q((size_t)nf * n);
    if (nf && download(Q.data(), Qv, K.bytes * nf)) return 1;
    if (download(K.B.data(), K.Vd, K.bytes)) return 1;
    auto normalise = [&](cplx* v) {
        const double nn = hdot(v, v, n).real();
        const double s = nn > 0.0 ? 1.0 / sqrt(nn) : 0.0;
        for (int64_t e = 0; e < n; ++e) v[e] *= s;
        return nn;
    };
    std::vector<const cplx*> qrows;
    for (int r = 0; r < nf; ++r) qrows.push_back(Q.data() + (int64_t)r * n);
    hproject(qrows, K.row(0), n, -1);
    if (!(normalise(K.row(0)) > 0.0)) return set_error("lanczos_orth: the start vector lies in the span of the frozen rows");
    double theta = 0.0, res = 0.0, alpha = 0.0, beta = 0.0, amax = 0.0;
    std::vector<double> y;
    for (int restart = 0; restart <= max_restart; ++restart) {
        std::vector<double> alphas, betas;
        for (int j = 0; j < kd; ++j) {
            if (K.extend(qrows, j, &alpha, &beta)) return 1;
            alphas.push_back(alpha);
            tridiag_lowest(alphas, betas, &theta, y);
            res = fabs(beta * y.back());
            amax = std::max(amax, std::max(fabs(alpha), beta));
            if (res < tol || beta < 1e-14 * std::max(amax, 1e-300) || j == kd - 1) break;
            betas.push_back(beta);
            K.accept(j, beta);
        }
        K.combine(y);
        hproject(qrows, K.x.data(), n, -1);
        normalise(K.x.data());
        K.restart_from_x();
        if (res < tol || beta < 1e-14 * std::max(amax, 1e-300)) break;
    }
    if (K.finish()) return 1;
    *eig = theta;
    *n_matvec = K.n_matvec;
    *residual = res;
    if (matvec_ms) *matvec_ms = 0.0;
    return 0;
}

// x = exp(-i dt H) x0, host statement (htn_core.h): the Lanczos basis with full two-pass reorthogonalisation on host copies of
// the vectors, H through grouped_gemm, the stopping / sub-stepping decisions of htn_expm::Expm -- the ones the device driver takes
int Backend::krylov_expm(const htn_gemm_launch* stages, int n_stages, int x_slot, int y_slot, void* Vv, int64_t n, int kd, double dt_re,
                         double dt_im, double tol, int max_restart, int zero_y, htn_exchange2_fn exchange, void* user, double* growth,
                         double* alpha0, int* n_matvec, double* err, double* matvec_ms) {
    if (kd < 2 || kd > 31) return set_error("krylov_expm: krylovdim must be in 2..31");
    if (!Vv || n <= 0) return set_error("krylov_expm: bad arguments");
    HostKrylov K{this, "krylov_expm", stages, n_stages, x_slot, y_slot, (cplx*)Vv, n, kd, zero_y, exchange, user};
    if (download(K.B.data(), K.Vd, K.bytes)) return 1;
    {
        const double nn = hdot(K.row(0), K.row(0), n).real();
        if (!(nn > 0.0)) return set_error("krylov_expm: the start vector is zero or not finite");
        const double sc = 1.0 / sqrt(nn);
        for (int64_t e = 0; e < n; ++e) K.B[(size_t)e] *= sc;
    }
    htn_expm::Expm ex;
    ex.dt_re = dt_re, ex.dt_im = dt_im, ex.tol = tol;
    const std::vector<const cplx*> none;
    for (int restart = 0;; ++restart) {
        ex.begin_cycle();
        for (int j = 0; j < kd; ++j) {
            double alpha, beta;
            if (K.extend(none, j, &alpha, &beta)) return 1;
            bool bad = false;
            const bool stop = ex.step(alpha, beta, kd, &bad);
            if (bad) return set_error("krylov_expm: the QL iteration of the tridiagonal matrix did not converge");
            if (stop) break;
            K.accept(j, beta);
        }
        if (!ex.converged && restart >= max_restart)
            return set_error("krylov_expm: not converged after %d restart(s) of krylovdim %d: fraction %.3e of dt remains (estimate %.3e, tol %.3e)",
                             std::max(max_restart, 0), kd, ex.remaining, ex.est, tol);
        if (!ex.finish()) return set_error("krylov_expm: no fraction of the step down to 2^-60 meets the tolerance");
        K.combine(ex.c);
        K.restart_from_x();
        if (ex.remaining == 0.0) break;
    }
    if (K.finish()) return 1;
    *growth = ex.growth;
    *alpha0 = ex.alpha0;
    *n_matvec = K.n_matvec;
    *err = ex.err_total;
    if (matvec_ms) *matvec_ms = 0.0;
    return 0;
}

// (z - H) x = b, host statement (htn_core.h): the Lanczos basis with full two-pass reorthogonalisation on host copies of the
// vectors, H through grouped_gemm, the stopping / restart decisions of htn_resolvent::Resolvent -- the ones the device driver takes
int Backend::krylov_solve(const htn_gemm_launch* stages, int n_stages, int x_slot, int y_slot, void* Vv, int64_t n, int kd, double z_re,
                          double z_im, double tol, int max_restart, void* Xv, int use_guess, int zero_y, htn_exchange2_fn exchange,
                          void* user, double* norm, double* residual, int* n_matvec, double* matvec_ms) {
    if (kd < 2 || kd > 31) return set_error("krylov_solve: krylovdim must be in 2..31");
    if (!Vv || !Xv || n <= 0) return set_error("krylov_solve: bad arguments");
    HostKrylov K{this, "krylov_solve", stages, n_stages, x_slot, y_slot, (cplx*)Vv, n, kd, zero_y, exchange, user};
    if (download(K.B.data(), K.Vd, K.bytes)) return 1;
    htn_resolvent::Resolvent rs;
    rs.z = cplx(z_re, z_im), rs.tol = tol;
    rs.bnorm = sqrt(hdot(K.row(0), K.row(0), n).real());
    if (!(rs.bnorm > 0.0)) return set_error("krylov_solve: the right-hand side is zero or not finite");
    std::vector<cplx> X((size_t)n, cplx(0.0, 0.0));
    if (use_guess) {              // r0 = b - z x0 + H x0
        if (download(X.data(), Xv, K.bytes)) return 1;
        cplx *r = K.row(0), *hx = K.row(1);
        if (K.matvec(X.data(), hx)) return 1;
        ++K.n_matvec;
        for (int64_t e = 0; e < n; ++e) r[e] += hx[e] - rs.z * X[(size_t)e];
    }
    double rnorm = sqrt(hdot(K.row(0), K.row(0), n).real());
    if (!(rnorm == rnorm)) return set_error("krylov_solve: NaN in the residual of the start value");
    rs.begin_cycle(rnorm);
    if (rs.converged && !use_guess) return set_error("krylov_solve: tol >= 1 accepts x = 0");
    const std::vector<const cplx*> none;
    for (int restart = 0; !rs.converged; ++restart) {
        for (int64_t e = 0; e < n; ++e) K.B[(size_t)e] *= 1.0 / rnorm;
        double alpha = 0.0, beta = 0.0;
        for (int j = 0; j < kd; ++j) {
            if (K.extend(none, j, &alpha, &beta)) return 1;
            if (rs.step(alpha, beta, kd)) break;
            K.accept(j, beta);
        }
        if (!rs.converged && restart >= max_restart)
            return set_error("krylov_solve: not converged after %d restart(s) of krylovdim %d: relative residual %.3e remains (tol %.3e)",
                             std::max(max_restart, 0), kd, rs.resid, tol);
        rs.finish();
        K.combine(rs.y);
        for (int64_t e = 0; e < n; ++e) X[(size_t)e] += K.x[(size_t)e];
        if (rs.converged) break;
        rnorm = rs.rho_norm();
        if (!(rnorm > 0.0) || !(beta > 0.0)) return set_error("krylov_solve: the residual of an unconverged cycle vanished");
        std::vector<cplx> c = rs.rho;                  // (the newest row is still the raw vector beta_m v_m)
        for (cplx& v : c) v /= rnorm;
        c.back() /= beta;
        K.combine(c);
        K.restart_from_x();
        rnorm = 1.0;                                   // (row 0 is a unit vector already; beta_0 of the next cycle is |rho|)
        rs.begin_cycle(rs.rho_norm());
    }
    const double xn = sqrt(hdot(X.data(), X.data(), n).real());
    for (int64_t e = 0; e < n; ++e) K.B[(size_t)e] = xn > 0.0 ? X[(size_t)e] / xn : cplx(0.0, 0.0);
    if (upload(Xv, X.data(), K.bytes) || K.finish()) return 1;
    *norm = xn;
    *residual = rs.resid;
    *n_matvec = K.n_matvec;
    if (matvec_ms) *matvec_ms = 0.0;
    return 0;
}

int Backend::dotc(const void* a, const void* b, int64_t n, double* out_host) {
    std::vector<cplx> ha((size_t)n), hb((size_t)n);
    if (download(ha.data(), a, sizeof(cplx) * (size_t)n) || download(hb.data(), b, sizeof(cplx) * (size_t)n)) return 1;
    const cplx v = hdot(ha.data(), hb.data(), n);
    out_host[0] = v.real(), out_host[1] = v.imag();
    return 0;
}

int Backend::orthonormalise_rows(void* P, int64_t n, int nvec, double drop_tol, int* kept) {
    std::vector<cplx> h((size_t)nvec * n);
    if (nvec && download(h.data(), P, sizeof(cplx) * h.size())) return 1;
    std::vector<const cplx*> rows;
    int k = 0;
    for (int r = 0; r < nvec; ++r) {
        cplx* dst = h.data() + (int64_t)k * n;
        if (r != k) memcpy((void*)dst, h.data() + (int64_t)r * n, sizeof(cplx) * (size_t)n);
        const double n0 = hdot(dst, dst, n).real();
        hproject(rows, dst, n, -1);
        const double n1 = hdot(dst, dst, n).real();
        if (!(n0 > 0.0) || !(n1 > drop_tol * drop_tol * n0)) continue;
        const double sc = 1.0 / sqrt(n1);
        for (int64_t e = 0; e < n; ++e) dst[e] *= sc;
        rows.push_back(dst);
        ++k;
    }
    if (k && (upload(P, h.data(), sizeof(cplx) * (size_t)k * n) || sync())) return 1;
    *kept = k;
    return 0;
}

// Householder QR of the blocks on host memory (conventions of htn_qr_blocks_z: R / L diagonal real and non-negative, a column
// whose remainder is below 1e-13 of its norm gets an exact zero there and no reflector -- Q stays orthonormal by construction)
void htn::qr_blocks_host(cplx* A, cplx* Rb, const htn_qr_block* desc, int n_blocks) {
    std::vector<cplx> M, Q, V;
    std::vector<double> tau, cn;
    std::vector<cplx> ph;
    for (int b = 0; b < n_blocks; ++b) {
        const htn_qr_block& D = desc[b];
        const int64_t m = D.m, n = D.n;
        if (m <= 0 || n <= 0) continue;
        M.assign((size_t)(m * n), cplx(0.0, 0.0));
        V.assign((size_t)(m * n), cplx(0.0, 0.0));
        tau.assign((size_t)n, 0.0);
        cn.assign((size_t)n, 0.0);
        ph.assign((size_t)n, cplx(1.0, 0.0));
        for (int64_t j = 0; j < n; ++j)
            for (int64_t i = 0; i < m; ++i) {
                M[(size_t)(i + j * m)] = D.trans ? std::conj(A[D.offset + j + i * D.ld]) : A[D.offset + i + j * D.ld];
                cn[(size_t)j] += std::norm(M[(size_t)(i + j * m)]);
            }
        for (int64_t k = 0; k < n; ++k) {
            double n2 = 0.0;
            for (int64_t i = k; i < m; ++i) n2 += std::norm(M[(size_t)(i + k * m)]);
            const double nr = sqrt(n2);
            if (!(nr > 1e-13 * sqrt(cn[(size_t)k]))) {
                for (int64_t i = k; i < m; ++i) M[(size_t)(i + k * m)] = cplx(0.0, 0.0);
                continue;
            }
            const cplx x0 = M[(size_t)(k + k * m)];
            const cplx p = std::abs(x0) > 0.0 ? x0 / std::abs(x0) : cplx(1.0, 0.0);
            const cplx beta = -p * nr;
            double vn2 = 0.0;
            for (int64_t i = k; i < m; ++i) {
                V[(size_t)(i + k * m)] = M[(size_t)(i + k * m)] - (i == k ? beta : cplx(0.0, 0.0));
                vn2 += std::norm(V[(size_t)(i + k * m)]);
            }
            tau[(size_t)k] = 2.0 / vn2;
            ph[(size_t)k] = -p;
            for (int64_t j = k + 1; j < n; ++j) {
                cplx w(0.0, 0.0);
                for (int64_t i = k; i < m; ++i) w += std::conj(V[(size_t)(i + k * m)]) * M[(size_t)(i + j * m)];
                w *= tau[(size_t)k];
                for (int64_t i = k; i < m; ++i) M[(size_t)(i + j * m)] -= V[(size_t)(i + k * m)] * w;
            }
            M[(size_t)(k + k * m)] = beta;
            for (int64_t i = k + 1; i < m; ++i) M[(size_t)(i + k * m)] = cplx(0.0, 0.0);
        }
        Q.assign((size_t)(m * n), cplx(0.0, 0.0));
        for (int64_t j = 0; j < n; ++j) Q[(size_t)(j + j * m)] = cplx(1.0, 0.0);
        for (int64_t k = n - 1; k >= 0; --k) {
            if (tau[(size_t)k] == 0.0) continue;
            for (int64_t j = 0; j < n; ++j) {
                cplx w(0.0, 0.0);
                for (int64_t i = k; i < m; ++i) w += std::conj(V[(size_t)(i + k * m)]) * Q[(size_t)(i + j * m)];
                w *= tau[(size_t)k];
                for (int64_t i = k; i < m; ++i) Q[(size_t)(i + j * m)] -= V[(size_t)(i + k * m)] * w;
            }
        }
        for (int64_t j = 0; j < n; ++j)
            for (int64_t i = 0; i < m; ++i) {
                const cplx q = Q[(size_t)(i + j * m)] * ph[(size_t)j];
                if (D.trans) A[D.offset + j + i * D.ld] = std::conj(q);
                else A[D.offset + i + j * D.ld] = q;
            }
        for (int64_t j = 0; j < n; ++j)
            for (int64_t i = 0; i < n; ++i) {
                cplx r = i <= j ? M[(size_t)(i + j * m)] * std::conj(ph[(size_t)i]) : cplx(0.0, 0.0);
                if (i == j) r = cplx(r.real(), 0.0);
                if (D.trans) Rb[D.r_offset + j + i * D.ldr] = std::conj(r);
                else Rb[D.r_offset + i + j * D.ldr] = r;
            }
    }
}

int Backend::qr_blocks(void* A, void* R, const htn_qr_block* desc_dev, const htn_qr_block* desc_host, int n_blocks) {
    (void)desc_dev;
    if (n_blocks <= 0) return 0;
    if (!desc_host) return set_error("qr_blocks: the host copy of the descriptors is required");
    int64_t a0 = INT64_MAX, a1 = 0, r0 = INT64_MAX, r1 = 0;
    for (int b = 0; b < n_blocks; ++b) {
        const htn_qr_block& D = desc_host[b];
        const int64_t vr = D.trans ? D.n : D.m, vc = D.trans ? D.m : D.n;
        a0 = std::min(a0, D.offset), a1 = std::max(a1, D.offset + (vc - 1) * D.ld + vr);
        r0 = std::min(r0, D.r_offset), r1 = std::max(r1, D.r_offset + (int64_t)(D.n - 1) * D.ldr + D.n);
    }
    std::vector<cplx> ha((size_t)(a1 - a0)), hr((size_t)(r1 - r0));
    if (download(ha.data(), (cplx*)A + a0, sizeof(cplx) * ha.size()) || download(hr.data(), (cplx*)R + r0, sizeof(cplx) * hr.size()))
        return 1;
    std::vector<htn_qr_block> d(desc_host, desc_host + n_blocks);
    for (auto& D : d) D.offset -= a0, D.r_offset -= r0;
    qr_blocks_host(ha.data(), hr.data(), d.data(), n_blocks);
    if (upload((cplx*)A + a0, ha.data(), sizeof(cplx) * ha.size()) || upload((cplx*)R + r0, hr.data(), sizeof(cplx) * hr.size())) return 1;
    return sync();
}

int Backend::block_trdots(const void* A, const void* B, const htn_trdot_item* items_dev, const htn_trdot_item* items, int n_items,
                          void* out, int n_out) {
    (void)items_dev;
    if (n_out <= 0) return 0;
    if (n_items > 0 && !items) return set_error("block_trdots: the host copy of the items is required");
    int64_t a0 = INT64_MAX, a1 = 0, b0 = INT64_MAX, b1 = 0;
    for (int q = 0; q < n_items; ++q) {
        const htn_trdot_item& it = items[q];
        if (it.rows <= 0 || it.cols <= 0) continue;
        a0 = std::min(a0, it.a_off), a1 = std::max(a1, it.a_off + (int64_t)(it.cols - 1) * it.lda + it.rows);
        b0 = std::min(b0, it.b_off), b1 = std::max(b1, it.b_off + (int64_t)(it.rows - 1) * it.ldb + it.cols);
    }
    std::vector<cplx> ha((size_t)std::max<int64_t>(a1 - a0, 0)), hb((size_t)std::max<int64_t>(b1 - b0, 0)), res((size_t)n_out, cplx(0.0, 0.0));
    if (!ha.empty() && download(ha.data(), (const cplx*)A + a0, sizeof(cplx) * ha.size())) return 1;
    if (!hb.empty() && download(hb.data(), (const cplx*)B + b0, sizeof(cplx) * hb.size())) return 1;
    for (int q = 0; q < n_items; ++q) {
        const htn_trdot_item& it = items[q];
        if (it.out < 0 || it.out >= n_out) return set_error("block_trdots: item %d adds to result %d of %d", q, it.out, n_out);
        if (it.rows <= 0 || it.cols <= 0) continue;
        const cplx *a = ha.data() + (it.a_off - a0), *b = hb.data() + (it.b_off - b0);
        double sr = 0.0, si = 0.0;                       // A[r, c] * B[c, r], no conjugation
        for (int64_t c = 0; c < it.cols; ++c)
            for (int64_t r = 0; r < it.rows; ++r) {
                const cplx x = a[r + c * it.lda], y = b[c + r * it.ldb];
                sr += x.real() * y.real() - x.imag() * y.imag();
                si += x.real() * y.imag() + x.imag() * y.real();
            }
        res[(size_t)it.out] += cplx(it.w_re * sr - it.w_im * si, it.w_re * si + it.w_im * sr);
    }
    return upload(out, res.data(), sizeof(cplx) * res.size());
}

int Backend::block_place(void* dst, const void* src, const htn_place_item* items_dev, const htn_place_item* items, int n_items) {
    (void)items_dev;
    if (n_items <= 0) return 0;
    if (!items) return set_error("block_place: the host copy of the items is required");
    int64_t d0 = INT64_MAX, d1 = 0, s0 = INT64_MAX, s1 = 0;
    for (int q = 0; q < n_items; ++q) {
        const htn_place_item& it = items[q];
        if (it.rows <= 0 || it.cols <= 0) continue;
        d0 = std::min(d0, it.dst_off), d1 = std::max(d1, it.dst_off + (int64_t)(it.cols - 1) * it.ldd + it.rows);
        if (it.src_off >= 0) s0 = std::min(s0, it.src_off), s1 = std::max(s1, it.src_off + (int64_t)(it.cols - 1) * it.lds + it.rows);
    }
    std::vector<cplx> hd((size_t)std::max<int64_t>(d1 - d0, 0)), hs((size_t)std::max<int64_t>(s1 - s0, 0));
    if (hd.empty()) return 0;
    // (the views need not cover the range between them: what lies there is read first and written back as it was)
    if (download(hd.data(), (const cplx*)dst + d0, sizeof(cplx) * hd.size())) return 1;
    if (!hs.empty() && download(hs.data(), (const cplx*)src + s0, sizeof(cplx) * hs.size())) return 1;
    for (int q = 0; q < n_items; ++q) {
        const htn_place_item& it = items[q];
        if (it.rows <= 0 || it.cols <= 0) continue;
        cplx* d = hd.data() + (it.dst_off - d0);
        const cplx* s = it.src_off >= 0 ? hs.data() + (it.src_off - s0) : nullptr;
        for (int64_t c = 0; c < it.cols; ++c)
            for (int64_t r = 0; r < it.rows; ++r) {
                const cplx x = s ? s[r + c * it.lds] : cplx(0.0, 0.0);
                d[r + c * it.ldd] = s ? cplx(it.coef * x.real(), it.coef * x.imag()) : cplx(0.0, 0.0);
            }
    }
    return upload((cplx*)dst + d0, hd.data(), sizeof(cplx) * hd.size());
}

// Null-space projection on host memory (conventions of htn_block_nullproj_z): per item W = Q^H R, R -= Q W (side 0) or W = R Q^H,
// R -= W Q (side 1), twice; out[2 o] += |W|^2 of the first pass, out[2 o + 1] += |R|^2 at the end, items in list order
int htn::nullproj_host(cplx* Rb, const cplx* Qb, const htn_nullproj_item* items, int n_items, double* out, int n_out) {
    for (int o = 0; o < 2 * n_out; ++o) out[o] = 0.0;
    std::vector<cplx> W;
    for (int q = 0; q < n_items; ++q) {
        const htn_nullproj_item& it = items[q];
        if (it.out < 0 || it.out >= n_out) return set_error("block_nullproj: item %d adds to result %d of %d", q, it.out, n_out);
        if (it.m <= 0 || it.n <= 0) continue;
        const int64_t m = it.m, n = it.n, k = it.k, ldr = it.ldr, ldq = it.ldq;
        cplx* R = Rb + it.r_off;
        const cplx* Q = Qb + it.q_off;
        double w2 = 0.0, r2 = 0.0;
        for (int pass = 0; pass < 2 && k > 0; ++pass) {
            if (it.side == 0) {
                W.assign((size_t)(k * n), cplx(0.0, 0.0));
                for (int64_t c = 0; c < n; ++c)
                    for (int64_t t = 0; t < k; ++t) {
                        cplx s = 0.0;
                        for (int64_t i = 0; i < m; ++i) s += std::conj(Q[i + t * ldq]) * R[i + c * ldr];
                        W[(size_t)(t + c * k)] = s;
                    }
                for (int64_t c = 0; c < n; ++c)
                    for (int64_t t = 0; t < k; ++t) {
                        const cplx w = W[(size_t)(t + c * k)];
                        for (int64_t i = 0; i < m; ++i) R[i + c * ldr] -= Q[i + t * ldq] * w;
                    }
            } else {
                W.assign((size_t)(m * k), cplx(0.0, 0.0));
                for (int64_t t = 0; t < k; ++t)
                    for (int64_t c = 0; c < n; ++c) {
                        const cplx qc = std::conj(Q[t + c * ldq]);
                        for (int64_t i = 0; i < m; ++i) W[(size_t)(i + t * m)] += R[i + c * ldr] * qc;
                    }
                for (int64_t c = 0; c < n; ++c)
                    for (int64_t t = 0; t < k; ++t) {
                        const cplx qv = Q[t + c * ldq];
                        for (int64_t i = 0; i < m; ++i) R[i + c * ldr] -= W[(size_t)(i + t * m)] * qv;
                    }
            }
            if (pass == 0)
                for (const cplx& w : W) w2 += std::norm(w);
        }
        for (int64_t c = 0; c < n; ++c)
            for (int64_t i = 0; i < m; ++i) r2 += std::norm(R[i + c * ldr]);
        out[2 * it.out] += w2;
        out[2 * it.out + 1] += r2;
    }
    return 0;
}

int Backend::block_nullproj(void* R, const void* Q, const htn_nullproj_item* items_dev, const htn_nullproj_item* items, int n_items,
                            double* out, int n_out) {
    (void)items_dev;
    if (n_out <= 0) return 0;
    if (n_items > 0 && !items) return set_error("block_nullproj: the host copy of the items is required");
    int64_t r0 = INT64_MAX, r1 = 0, q0 = INT64_MAX, q1 = 0;
    for (int q = 0; q < n_items; ++q) {
        const htn_nullproj_item& it = items[q];
        if (it.m <= 0 || it.n <= 0) continue;
        r0 = std::min(r0, it.r_off), r1 = std::max(r1, it.r_off + (int64_t)(it.n - 1) * it.ldr + it.m);
        if (it.k > 0) {
            const int64_t qr = it.side ? it.k : it.m, qc = it.side ? it.n : it.k;
            q0 = std::min(q0, it.q_off), q1 = std::max(q1, it.q_off + (qc - 1) * it.ldq + qr);
        }
    }
    std::vector<cplx> hr((size_t)std::max<int64_t>(r1 - r0, 0)), hq((size_t)std::max<int64_t>(q1 - q0, 0));
    std::vector<double> res((size_t)(2 * n_out), 0.0);
    // (the views need not cover the range between them: what lies there is read first and written back as it was)
    if (!hr.empty() && download(hr.data(), (const cplx*)R + r0, sizeof(cplx) * hr.size())) return 1;
    if (!hq.empty() && download(hq.data(), (const cplx*)Q + q0, sizeof(cplx) * hq.size())) return 1;
    std::vector<htn_nullproj_item> d(items, items + n_items);
    for (auto& it : d) {
        it.r_off -= hr.empty() ? it.r_off : r0;
        it.q_off -= hq.empty() || it.k <= 0 ? it.q_off : q0;
    }
    if (nullproj_host(hr.data(), hq.data(), d.data(), n_items, res.data(), n_out)) return 1;
    if (!hr.empty() && upload((cplx*)R + r0, hr.data(), sizeof(cplx) * hr.size())) return 1;
    return upload(out, res.data(), sizeof(double) * res.size());
}

// One site of perfect sampling (conventions of htn_sample_step_z): per sample T = rho_l A and Re<A, T> per item, p(s) over the
// items in list order, the draw, rho' = scale x sum coef A^H T over the runs of items with one out_off
int Backend::sample_step(void* rho_next, const void* rho, const void* A, void* T, const htn_sample_item* items_dev, const htn_sample_item* items,
                         int n_items, int n_site, int n_samples, int64_t rho_stride, int64_t rho_next_stride, int64_t t_stride, const double* u,
                         int measure, int32_t* choice, double* logp) {
    (void)items_dev, (void)T, (void)t_stride;
    if (n_samples <= 0) return 0;
    if (n_items <= 0 || !items) return set_error("sample_step: the host copy of the items is required");
    if (n_site < 1 || n_site > HTN_MAX_SITE) return set_error("sample_step: %d site multiplets", n_site);
    int64_t a0 = INT64_MAX, a1 = 0;
    for (int q = 0; q < n_items; ++q) {
        const htn_sample_item& it = items[q];
        if (it.n_l < 1 || it.n_r < 1 || it.lda < it.n_l || it.s < 0 || it.s >= n_site) return set_error("sample_step: item %d is malformed", q);
        a0 = std::min(a0, it.a_off), a1 = std::max(a1, it.a_off + (int64_t)(it.n_r - 1) * it.lda + it.n_l);
    }
    const size_t B = (size_t)n_samples;
    std::vector<cplx> hr(B * (size_t)rho_stride), hn(B * (size_t)rho_next_stride), ha((size_t)(a1 - a0));
    std::vector<double> hu(B, 0.0), hl(B);
    std::vector<int32_t> hc(B);
    // (the runs need not cover the next rho: what lies between them is read first and written back as it was)
    if (download(hr.data(), rho, sizeof(cplx) * hr.size()) || download(hn.data(), rho_next, sizeof(cplx) * hn.size()) ||
        download(ha.data(), (const cplx*)A + a0, sizeof(cplx) * ha.size()) || download(hl.data(), logp, sizeof(double) * B))
        return 1;
    if (measure && download(hu.data(), u, sizeof(double) * B)) return 1;
    std::vector<std::vector<cplx>> Ts((size_t)n_items);
    for (size_t b = 0; b < B; ++b) {
        const cplx* R = hr.data() + b * (size_t)rho_stride;
        cplx* O = hn.data() + b * (size_t)rho_next_stride;
        double p[HTN_MAX_SITE] = {0.0, 0.0, 0.0, 0.0};
        for (int q = 0; q < n_items; ++q) {
            const htn_sample_item& it = items[q];
            const int64_t nl = it.n_l, nr = it.n_r;
            const cplx *Rl = R + it.rho_off, *Ab = ha.data() + (it.a_off - a0);
            std::vector<cplx>& Tq = Ts[(size_t)q];
            Tq.assign((size_t)(nl * nr), cplx(0.0, 0.0));
            double dot = 0.0;
            for (int64_t j = 0; j < nr; ++j) {
                for (int64_t k = 0; k < nl; ++k) {
                    const cplx a = Ab[k + j * it.lda];
                    for (int64_t i = 0; i < nl; ++i) Tq[(size_t)(i + j * nl)] += Rl[i + k * nl] * a;
                }
                for (int64_t i = 0; i < nl; ++i) {
                    const cplx a = Ab[i + j * it.lda], t = Tq[(size_t)(i + j * nl)];
                    dot += a.real() * t.real() + a.imag() * t.imag();
                }
            }
            p[it.s] += it.coef * dot;
        }
        double total = 0.0;
        for (int s = 0; s < n_site; ++s) total += p[s];
        int pick = -1;
        double scale = 1.0 / total;
        if (measure) {
            const double target = hu[b] * total;
            int last = -1;
            double cum = 0.0;
            for (int s = 0; s < n_site; ++s) {
                cum += p[s];
                if (p[s] > 0.0) {
                    last = s;
                    if (pick < 0 && cum >= target) pick = s;
                }
            }
            if (pick < 0) pick = last;
            if (pick < 0) return set_error("sample_step: sample %d has no weight on this site", (int)b);
            hl[b] += log(p[pick] / total);
            scale = 1.0 / p[pick];
        }
        hc[b] = pick;
        for (int q = 0; q < n_items;) {
            const int64_t nr = items[q].n_r, out_off = items[q].out_off;
            cplx* Or = O + out_off;
            for (int64_t e = 0; e < nr * nr; ++e) Or[e] = cplx(0.0, 0.0);
            int r = q;
            for (; r < n_items && items[r].out_off == out_off; ++r) {
                const htn_sample_item& it = items[r];
                if (measure && it.s != pick) continue;
                const int64_t nl = it.n_l;
                const cplx* Ab = ha.data() + (it.a_off - a0);
                const std::vector<cplx>& Tr = Ts[(size_t)r];
                for (int64_t j = 0; j < nr; ++j)
                    for (int64_t i = 0; i < nr; ++i) {
                        cplx s = 0.0;
                        for (int64_t k = 0; k < nl; ++k) s += std::conj(Ab[k + i * it.lda]) * Tr[(size_t)(k + j * nl)];
                        Or[i + j * nr] += it.coef * s;
                    }
            }
            for (int64_t e = 0; e < nr * nr; ++e) Or[e] *= scale;
            q = r;
        }
    }
    if (upload(rho_next, hn.data(), sizeof(cplx) * hn.size()) || upload(choice, hc.data(), sizeof(int32_t) * B)) return 1;
    return measure ? upload(logp, hl.data(), sizeof(double) * B) : 0;
}

// ---- the kernel-level entries that have a host-memory statement: what the CPU baseline library exports ------------------
extern "C" {

// Host-memory statement of the kernel-level entry: what the CPU baseline library exports (V and the buffers of the stages are
// host pointers, the stages run through that library's grouped GEMM, scratch and stream are not used).  Weak: in
// libhubbardtn_hip.so the definition of htn_krylov.hip (device pointers, the gfx950 kernels) takes its place at link time.
__attribute__((weak)) int htn_krylov_expm_z(const htn_gemm_launch* stages, int32_t n_stages, int32_t x_slot, int32_t y_slot, void* V, int64_t n,
                                            int32_t krylovdim, double dt_re, double dt_im, double tol, int32_t max_restart, void* scratch,
                                            int32_t zero_y, htn_exchange2_fn exchange, void* user, double* growth_host, double* alpha0_host,
                                            int32_t* n_matvec_host, double* err_host, double* matvec_ms_host, void* stream) {
    (void)scratch, (void)stream;
    if (!stages || !V || !growth_host || !alpha0_host || !n_matvec_host || !err_host) return set_error("htn_krylov_expm_z: bad arguments");
    std::unique_ptr<Backend> be(make_backend(HTN_BACKEND_CPU, 0, nullptr));
    if (!be) return 1;
    int nmv = 0;
    const int rc = be->krylov_expm(stages, n_stages, x_slot, y_slot, V, n, krylovdim, dt_re, dt_im, tol, max_restart, zero_y, exchange, user,
                                   growth_host, alpha0_host, &nmv, err_host, matvec_ms_host);
    *n_matvec_host = nmv;
    return rc;
}

// Host-memory statement of the kernel-level entry (V, X and the buffers of the stages are host pointers; V holds krylovdim + 2
// rows).  Weak: in libhubbardtn_hip.so the definition of htn_krylov.hip takes its place at link time.
__attribute__((weak)) int htn_krylov_solve_z(const htn_gemm_launch* stages, int32_t n_stages, int32_t x_slot, int32_t y_slot, void* V, int64_t n,
                                             int32_t krylovdim, double z_re, double z_im, double tol, int32_t max_restart, void* X,
                                             int32_t use_guess, void* scratch, int32_t zero_y, htn_exchange2_fn exchange, void* user,
                                             double* norm_host, double* residual_host, int32_t* n_matvec_host, double* matvec_ms_host,
                                             void* stream) {
    (void)scratch, (void)stream;
    if (!stages || !V || !X || !norm_host || !residual_host || !n_matvec_host) return set_error("htn_krylov_solve_z: bad arguments");
    if (!(z_re - z_re == 0.0) || !(z_im - z_im == 0.0) || !(tol >= 0.0)) return set_error("htn_krylov_solve_z: z must be finite, tol >= 0");
    std::unique_ptr<Backend> be(make_backend(HTN_BACKEND_CPU, 0, nullptr));
    if (!be) return 1;
    int nmv = 0;
    const int rc = be->krylov_solve(stages, n_stages, x_slot, y_slot, V, n, krylovdim, z_re, z_im, tol, max_restart, X, use_guess, zero_y,
                                    exchange, user, norm_host, residual_host, &nmv, matvec_ms_host);
    *n_matvec_host = nmv;
    return rc;
}

// Host-memory statement of the kernel-level entry (Householder reflections): what the CPU baseline library exports.  Weak: in
// libhubbardtn_hip.so the definition of htn_qr.hip (device pointers, the gfx950 kernel) takes its place at link time.
__attribute__((weak)) int htn_qr_blocks_z(void* A, void* Rbuf, const htn_qr_block* desc, const htn_qr_block* desc_host, int32_t n_blocks,
                                          void* stream) {
    (void)stream;
    if (n_blocks <= 0) return 0;
    if (!A || !Rbuf || (!desc && !desc_host)) return set_error("htn_qr_blocks_z: bad arguments");
    const htn_qr_block* d = desc_host ? desc_host : desc;
    for (int b = 0; b < n_blocks; ++b)
        if (d[b].n < 1 || d[b].m < d[b].n || d[b].ldr < d[b].n || d[b].ld < (d[b].trans ? d[b].n : d[b].m))
            return set_error("htn_qr_blocks_z: block %d: m = %d, n = %d, ld = %d, ldr = %d (need m >= n >= 1)", b, d[b].m, d[b].n, d[b].ld, d[b].ldr);
    qr_blocks_host((cplx*)A, (cplx*)Rbuf, d, n_blocks);
    return 0;
}

// Host-memory statement of the kernel-level entry (plain loops): what the CPU baseline library exports.  Weak: in
// libhubbardtn_hip.so the definition of htn_nullproj.hip (device pointers, the gfx950 kernel) takes its place at link time.
__attribute__((weak)) int htn_block_nullproj_z(void* R, const void* Q, const htn_nullproj_item* items, const htn_nullproj_item* items_host,
                                               int32_t n_items, double* out, int32_t n_out, void* scratch, void* stream) {
    (void)scratch, (void)stream;
    if (n_items < 0 || n_out < 0) return set_error("htn_block_nullproj_z: negative count");
    if (n_out == 0) return 0;
    const htn_nullproj_item* d = items_host ? items_host : items;
    if (!out || (n_items > 0 && (!d || !R))) return set_error("htn_block_nullproj_z: bad arguments");
    for (int q = 0; q < n_items; ++q)
        if (d[q].m < 0 || d[q].n < 0 || d[q].k < 0 || (d[q].side != 0 && d[q].side != 1) ||
            (d[q].m > 0 && d[q].n > 0 && (d[q].ldr < d[q].m || (d[q].k > 0 && (!Q || d[q].ldq < (d[q].side ? d[q].k : d[q].m))))))
            return set_error("htn_block_nullproj_z: item %d: m = %d, n = %d, k = %d, ldr = %d, ldq = %d, side = %d", q, d[q].m, d[q].n, d[q].k,
                             d[q].ldr, d[q].ldq, d[q].side);
    return nullproj_host((cplx*)R, (const cplx*)Q, d, n_items, out, n_out);
}

}  // extern "C"
