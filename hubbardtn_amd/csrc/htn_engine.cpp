// Bond-update / sweep driver behind the C ABI (include/hubbardtn_hip.h, "Bond-update / sweep level").
//
// Stands in for MPSKit's two-site sweep body reached from
//     find_groundstate(psi0, H, IDMRG2(; trscheme, tol))                src/HubbardFunctions.jl:1010
// per bond: form theta, Lanczos lowest eigenpair of the AC2 effective Hamiltonian, per-sector SVD + global truncation,
// write back, move the environment.  Sweep order follows MPSKit's DMRG2: bonds 1..L-1 going
// right, L-2..1 going left (2L-3 updates).  All tensors stay on the device between bonds; the host sees the Lanczos
// tridiagonal coefficients and the singular values (needed for the global truncation rule, App. A.6).
// The infinite-chain growth loop around it (htn_idmrg_*: McCulloch's IDMRG2, hubbardtn_amd/idmrg.py's rules) lives here
// too, so that the CPU baseline library, built from this file, exports it as well.
// Host C++ (no HIP): device work goes through htn::Backend.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>

#include "htn_core.h"
#include "htn_expm.h"

namespace htn {
Backend* make_backend(int backend, int device, void* stream);       // one per library (htn_backend_hip.hip / cpu)
}
using namespace htn;

// ---- host statements of the two Backend methods that are not pure (htn_core.h) ---------------------------------------
namespace {
// lowest eigenpair of the symmetric tridiagonal (alpha, beta): bisection on the Sturm count, then inverse iteration
void tridiag_lowest_host(const std::vector<double>& alpha, const std::vector<double>& beta, double* eig, std::vector<double>& vec) {
    const int k = (int)alpha.size();
    auto count = [&](double x) {
        int cnt = 0;
        double d = 1.0;
        for (int i = 0; i < k; ++i) {
            d = (alpha[i] - x) - (i ? beta[i - 1] * beta[i - 1] / d : 0.0);
            if (d == 0.0) d = 1e-300;
            if (d < 0.0) ++cnt;
        }
        return cnt;
    };
    double lo = alpha[0], hi = alpha[0];
    for (int i = 0; i < k; ++i) {
        const double r = (i ? fabs(beta[i - 1]) : 0.0) + (i + 1 < k ? fabs(beta[i]) : 0.0);
        lo = fmin(lo, alpha[i] - r);
        hi = fmax(hi, alpha[i] + r);
    }
    const double scale = fmax(fabs(lo), fabs(hi)) + 1e-300;
    hi += 1e-12 * scale;
    for (int it = 0; it < 200 && hi - lo > 4e-16 * scale; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (count(mid) >= 1) hi = mid;
        else lo = mid;
    }
    const double lam = 0.5 * (lo + hi);
    *eig = lam;
    vec.assign(k, 1.0);
    if (k == 1) return;
    const double mu = lam - 1e-10 * scale;
    std::vector<double> d(k), l(k), z(k);
    d[0] = alpha[0] - mu;
    for (int i = 1; i < k; ++i) {
        l[i] = beta[i - 1] / d[i - 1];
        d[i] = (alpha[i] - mu) - l[i] * beta[i - 1];
        if (d[i] == 0.0) d[i] = 1e-300;
    }
    for (int i = 0; i < k; ++i) vec[i] = (i & 1) ? -0.7 : 1.0;
    for (int iter = 0; iter < 4; ++iter) {
        z[0] = vec[0];
        for (int i = 1; i < k; ++i) z[i] = vec[i] - l[i] * z[i - 1];
        z[k - 1] /= d[k - 1];
        for (int i = k - 2; i >= 0; --i) z[i] = z[i] / d[i] - l[i + 1] * z[i + 1];
        double nn = 0.0;
        for (int i = 0; i < k; ++i) nn += z[i] * z[i];
        nn = 1.0 / sqrt(nn);
        for (int i = 0; i < k; ++i) vec[i] = z[i] * nn;
    }
    if (vec[0] < 0.0)
        for (int i = 0; i < k; ++i) vec[i] = -vec[i];
}
cplx hdot(const cplx* a, const cplx* b, int64_t n) {
    cplx s = 0.0;
    for (int64_t e = 0; e < n; ++e) s += std::conj(a[e]) * b[e];
    return s;
}
// w -= sum_r rows[r] <rows[r], w>, twice; returns the sum of <rows[pick], w> over both passes
double hproject(const std::vector<const cplx*>& rows, cplx* w, int64_t n, int pick) {
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
}  // namespace

int Backend::lanczos_orth(const htn_gemm_launch* stages, int n_stages, int x_slot, int y_slot, void* Vv, int64_t n, int kd, double tol,
                          int max_restart, int zero_y, htn_exchange2_fn exchange, void* user, const void* Qv, int nf, double* eig,
                          int* n_matvec, double* residual, double* matvec_ms) {
    if (kd < 2 || nf < 0) return set_error("lanczos_orth: krylovdim >= 2 and n_frozen >= 0 required");
    cplx* Vd = (cplx*)Vv;
    const size_t bytes = sizeof(cplx) * (size_t)n;
    std::vector<cplx> Q((size_t)nf * n), B((size_t)(kd + 1) * n), x((size_t)n);
    if (nf && download(Q.data(), Qv, bytes * nf)) return 1;
    if (download(B.data(), Vd, bytes)) return 1;
    auto matvec = [&](const cplx* v, cplx* w) -> int {        // through device rows kd (x) and kd + 1 (y) of the caller's V
        cplx *xd = Vd + (int64_t)kd * n, *yd = Vd + (int64_t)(kd + 1) * n;
        if (upload(xd, v, bytes)) return 1;
        if (zero_y && zero(yd, bytes)) return 1;
        for (int s = 0; s < n_stages; ++s) {
            const void* bufs[HTN_MAX_BUFS];
            for (int b = 0; b < HTN_MAX_BUFS; ++b) bufs[b] = stages[s].bufs[b];
            bufs[x_slot] = xd;
            bufs[y_slot] = yd;
            if (stages[s].n_tiles > 0 && grouped_gemm(bufs, stages[s].tiles, stages[s].n_tiles, stages[s].segs)) return 1;
        }
        if (exchange && exchange(yd, n, user)) return set_error("lanczos_orth: the exchange hook reported a failure");
        return download(w, yd, bytes);
    };
    auto normalise = [&](cplx* v) {
        const double nn = hdot(v, v, n).real();
        const double s = nn > 0.0 ? 1.0 / sqrt(nn) : 0.0;
        for (int64_t e = 0; e < n; ++e) v[e] *= s;
        return nn;
    };
    std::vector<const cplx*> qrows;
    for (int r = 0; r < nf; ++r) qrows.push_back(Q.data() + (int64_t)r * n);
    hproject(qrows, B.data(), n, -1);
    if (!(normalise(B.data()) > 0.0)) return set_error("lanczos_orth: the start vector lies in the span of the frozen rows");
    int nmv = 0;
    double theta = 0.0, res = 0.0, beta = 0.0, amax = 0.0;
    std::vector<double> y;
    for (int restart = 0; restart <= max_restart; ++restart) {
        std::vector<double> alphas, betas;
        for (int j = 0; j < kd; ++j) {
            cplx* w = B.data() + (int64_t)(j + 1) * n;
            if (matvec(B.data() + (int64_t)j * n, w)) return 1;
            ++nmv;
            std::vector<const cplx*> rows = qrows;
            for (int r = 0; r <= j; ++r) rows.push_back(B.data() + (int64_t)r * n);
            const double alpha = hproject(rows, w, n, nf + j);
            beta = sqrt(hdot(w, w, n).real());
            if (!(alpha == alpha) || !(beta == beta)) return set_error("lanczos_orth: NaN in the tridiagonal coefficients");
            alphas.push_back(alpha);
            tridiag_lowest_host(alphas, betas, &theta, y);
            res = fabs(beta * y.back());
            amax = std::max(amax, std::max(fabs(alpha), beta));
            if (res < tol || beta < 1e-14 * std::max(amax, 1e-300) || j == kd - 1) break;
            betas.push_back(beta);
            const double inv = 1.0 / beta;
            for (int64_t e = 0; e < n; ++e) w[e] *= inv;
        }
        const int k = (int)y.size();
        std::fill(x.begin(), x.end(), cplx(0.0, 0.0));
        for (int r = 0; r < k; ++r)
            for (int64_t e = 0; e < n; ++e) x[e] += y[r] * B[(size_t)r * n + e];
        hproject(qrows, x.data(), n, -1);
        normalise(x.data());
        memcpy((void*)B.data(), x.data(), bytes);
        if (res < tol || beta < 1e-14 * std::max(amax, 1e-300)) break;
    }
    if (upload(Vd, B.data(), bytes) || sync()) return 1;
    *eig = theta;
    *n_matvec = nmv;
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
    cplx* Vd = (cplx*)Vv;
    const size_t bytes = sizeof(cplx) * (size_t)n;
    std::vector<cplx> B((size_t)(kd + 1) * n), x((size_t)n);
    if (download(B.data(), Vd, bytes)) return 1;
    auto matvec = [&](const cplx* v, cplx* w) -> int {        // through device rows kd (x) and kd + 1 (y) of the caller's V
        cplx *xd = Vd + (int64_t)kd * n, *yd = Vd + (int64_t)(kd + 1) * n;
        if (upload(xd, v, bytes)) return 1;
        if (zero_y && zero(yd, bytes)) return 1;
        for (int s = 0; s < n_stages; ++s) {
            const void* bufs[HTN_MAX_BUFS];
            for (int b = 0; b < HTN_MAX_BUFS; ++b) bufs[b] = stages[s].bufs[b];
            bufs[x_slot] = xd;
            bufs[y_slot] = yd;
            if (stages[s].n_tiles > 0 && grouped_gemm(bufs, stages[s].tiles, stages[s].n_tiles, stages[s].segs)) return 1;
        }
        if (exchange && exchange(yd, n, user)) return set_error("krylov_expm: the exchange hook reported a failure");
        return download(w, yd, bytes);
    };
    {
        const double nn = hdot(B.data(), B.data(), n).real();
        if (!(nn > 0.0)) return set_error("krylov_expm: the start vector is zero or not finite");
        const double sc = 1.0 / sqrt(nn);
        for (int64_t e = 0; e < n; ++e) B[(size_t)e] *= sc;
    }
    htn_expm::Expm ex;
    ex.dt_re = dt_re, ex.dt_im = dt_im, ex.tol = tol;
    int nmv = 0;
    for (int restart = 0;; ++restart) {
        ex.begin_cycle();
        for (int j = 0; j < kd; ++j) {
            cplx* w = B.data() + (int64_t)(j + 1) * n;
            if (matvec(B.data() + (int64_t)j * n, w)) return 1;
            ++nmv;
            std::vector<const cplx*> rows;
            for (int r = 0; r <= j; ++r) rows.push_back(B.data() + (int64_t)r * n);
            const double alpha = hproject(rows, w, n, j);
            const double beta = sqrt(hdot(w, w, n).real());
            if (!(alpha == alpha) || !(beta == beta)) return set_error("krylov_expm: NaN in the tridiagonal coefficients");
            bool bad = false;
            const bool stop = ex.step(alpha, beta, kd, &bad);
            if (bad) return set_error("krylov_expm: the QL iteration of the tridiagonal matrix did not converge");
            if (stop) break;
            const double inv = 1.0 / beta;
            for (int64_t e = 0; e < n; ++e) w[e] *= inv;
        }
        if (!ex.converged && restart >= max_restart)
            return set_error("krylov_expm: not converged after %d restart(s) of krylovdim %d: fraction %.3e of dt remains (estimate %.3e, tol %.3e)",
                             std::max(max_restart, 0), kd, ex.remaining, ex.est, tol);
        if (!ex.finish()) return set_error("krylov_expm: no fraction of the step down to 2^-60 meets the tolerance");
        const int m = (int)ex.c.size();
        std::fill(x.begin(), x.end(), cplx(0.0, 0.0));
        for (int r = 0; r < m; ++r)
            for (int64_t e = 0; e < n; ++e) x[(size_t)e] += ex.c[(size_t)r] * B[(size_t)r * n + e];
        memcpy((void*)B.data(), x.data(), bytes);
        if (ex.remaining == 0.0) break;
    }
    if (upload(Vd, B.data(), bytes) || sync()) return 1;
    *growth = ex.growth;
    *alpha0 = ex.alpha0;
    *n_matvec = nmv;
    *err = ex.err_total;
    if (matvec_ms) *matvec_ms = 0.0;
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

// Handles are reference counted: an htn_mps keeps its context and its MPO alive, so destroying the handles in any order
// (garbage-collected host languages do exactly that) is safe; the last release frees the object.
struct htn_ctx {
    std::atomic<int> refs{1};
    std::unique_ptr<Backend> be;
    int rank = 0, world = 1;
    bool shard = false;              // zero y + reduce after every matvec (world > 1, or forced for tests)
    htn_exchange2_fn exch = nullptr;
    void* exch_user = nullptr;
};
struct htn_mpo {
    std::atomic<int> refs{1};
    htn_ctx* ctx;
    Mpo mpo;
};
static void ctx_release(htn_ctx* c) {
    if (c && --c->refs == 0) delete c;
}
static void mpo_release(htn_mpo* m) {
    if (m && --m->refs == 0) {
        htn_ctx* c = m->ctx;
        delete m;
        ctx_release(c);
    }
}

namespace {

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct DBuf {
    Backend* be;
    void* p;
    size_t bytes;
    DBuf(Backend* b, size_t n) : be(b), p(nullptr), bytes(n) { p = be->alloc(std::max<size_t>(n, 16)); }
    ~DBuf() {
        if (p) be->release(p);
    }
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
};
typedef std::shared_ptr<DBuf> DBufP;
// device buffer of host data (copy items, descriptors, column indices, scale factors, small matrices)
template <class T>
DBufP upload_vec(Backend* be, const std::vector<T>& v) {
    auto b = std::make_shared<DBuf>(be, sizeof(T) * std::max<size_t>(v.size(), 1));
    if (!b->p) return nullptr;
    if (!v.empty() && be->upload(b->p, v.data(), sizeof(T) * v.size())) return nullptr;
    return b;
}
struct DView {                     // complex128 window of a device buffer
    DBufP base;
    int64_t off = 0;
    cplx* ptr() const { return base ? (cplx*)base->p + off : nullptr; }
};

// plain rows x cols copy, op N: no gather, no scaling (callers set what differs)
htn_copy_item copy_item(int64_t dst_off, int32_t ldd, int64_t src_off, int32_t lds, int32_t rows, int32_t cols) {
    htn_copy_item it;
    memset(&it, 0, sizeof(it));
    it.dst_off = dst_off, it.src_off = src_off, it.idx_off = -1, it.scl_off = -1;
    it.rows = rows, it.cols = cols, it.ldd = ldd, it.lds = lds, it.op = HTN_OP_N, it.scale_dim = -1;
    return it;
}

// host wall time of the stages of one update; with `profile` every lap ends in a stream sync (GPU-inclusive times)
struct StageClock {
    Backend* be;
    bool profile;
    double t0, last;
    double plan = 0.0, lanczos = 0.0, svd = -1.0, env = 0.0;      // svd < 0: what the other stages leave of the total
    StageClock(Backend* b, bool p) : be(b), profile(p), t0(now()), last(t0) {}
    double lap() {
        if (profile) be->sync();
        const double t = now(), d = t - last;
        last = t;
        return d;
    }
};

struct DevTasks {
    DBufP mem;
    const htn_tile* tiles = nullptr;
    const htn_seg* segs = nullptr;
    int32_t ntiles = 0, nsegs = 0;
    int32_t ws_slots = 0;          // split-K workspace slabs the list needs (balance_tiles)
    int64_t flops = 0;
};

struct ApplyC {
    DevTasks dz, dy;
    bool has_z = false;
    int64_t zsize = 0, flops = 0;
    int32_t ntiles = 0, nsegs = 0;
};
template <class Lay>
struct TwoStageC {                 // compiled two-stage contraction (EnvPlan / OvlPlan): stage 1 -> BUF_Z, stage 2 -> BUF_Y
    std::shared_ptr<const Lay> lay;        // layout of the result (not set: the caller names it -- projector rows)
    DevTasks d1, d2;
    int64_t zsize = 0, flops = 0;
};
typedef TwoStageC<EnvLayout> EnvC;
typedef TwoStageC<OvlLayout> OvlC;
struct SvdC {
    SvdPlan sp;
    DBufP stage, desc;
    // sector-sharded SVD (world > 1): the blocks this rank owns (LPT over ~ m n^2), as their own staging / descriptor lists
    std::vector<htn_svd_block> own_desc;
    DBufP own_stage, own_desc_dev;
    int n_own = 0;
};
struct FinC {
    SiteLayoutP layA, layB;
    DBufP items;                   // iso_g | cen_g | iso_v copy items
    const htn_copy_item *ig = nullptr, *cg = nullptr, *iv = nullptr;
    int n_ig = 0, n_cg = 0, n_iv = 0;
    DevTasks cen;
    bool has_cen = false;
};

struct Spectrum {
    std::vector<Sec> secs;
    std::vector<std::vector<double>> vals;
};
struct RelayC {                    // copy items that re-lay a site tensor from one layout kind to another (or copy it)
    DBufP items;
    int n = 0;
};
struct Gauge1C {                   // compiled gauge move of a one-site update: QR / LQ descriptors + absorption into the neighbour
    std::vector<htn_qr_block> desc;
    DBufP desc_dev;
    int64_t rsize = 0;
    DevTasks absorb;
};
struct MeetC {                     // the items that pair the left and the right half of a correlator on one bond (htn_block_trdots_z)
    std::vector<htn_trdot_item> items;
    DBufP items_dev;
};
struct OrthState {                 // one attached state phi: overlap environments <psi|phi> per bond, carried along the sweep
    htn_mps* phi = nullptr;
    std::vector<OvlLayoutP> Llay, Rlay;
    std::vector<DView> Lbuf, Rbuf;
};
struct Solve {                     // the eigenproblem of one update (compiled apply, vector length) and what the solver returned
    std::shared_ptr<ApplyC> ap;
    int64_t n = 0;
    double E = 0.0, res = 0.0, mv_ms = 0.0;
    int nmv = 0;
    double growth = 1.0;           // evolving updates: |x| / |x0| of the exponential
};
struct BondWork {                  // what flows between the steps of one two-site update (htn_mps::update_bond)
    ThetaLayoutP tl;
    Solve sol;
    // device buffers: all live until the update returns and go back to the pool in reverse order of declaration
    DView V, z, Qb;                // Krylov basis (row 0: theta, then the optimised tensor); Z stage of the apply; projector rows
    std::shared_ptr<SvdC> sc;
    DView G, Vj;
    DBufP S, idx;                  // s_elems singular values | per-block sweep counts (int32); kept columns, block after block
    size_t s_elems = 0;
    std::vector<double> s_host;    // host copy of S
    int jac_sweeps = 0;
    std::vector<int> lens, qd, counts;     // per block: values, quantum dimension, kept values
    std::vector<std::vector<int>> order;   // per block: its columns by descending value
    std::vector<double> vals;              // all values, block after block, each block descending
    double nrm = 0.0, tw = 0.0;
    BondP mid;
    double tA = 0.0, tB = 0.0, tC = 0.0, tD = 0.0;      // HTN_DEBUG_HOST_TIMERS: after the SVD call, download, truncation, finalise plan
};

}  // namespace

struct htn_mps {
    std::atomic<int> refs{1};      // htn_mps_destroy drops one reference (htn_idmrg_window hands out extra ones)
    htn_ctx* ctx;
    htn_mpo* mpo_handle = nullptr;
    Backend* be;
    const Mpo* mpo;
    int L;
    std::vector<BondP> bonds;
    std::vector<SiteLayoutP> site_lay;
    std::vector<DView> site_buf;
    std::vector<EnvLayoutP> Llay, Rlay;
    std::vector<DView> Lbuf, Rbuf;
    std::unordered_map<std::string, std::shared_ptr<const void>> cache;
    int64_t hits = 0, misses = 0;
    double energy = 0.0;
    std::map<int, Spectrum> spectra;
    std::map<int, std::pair<std::pair<int, double>, double>> cut_hint;      // bond -> ((chi, cutoff), smallest kept value)
    std::map<int, int> sweeps_hint;     // bond -> outer Jacobi sweeps its large blocks needed last time (htn_svd_opts.sweeps_hint)
    std::vector<int32_t> idx_host;
    std::vector<OrthState> orth;        // htn_mps_set_orthogonal: the sweep stays in the orthogonal complement of these states
    int orth_dropped = 0;               // projector vectors dropped as numerically dependent in the last bond update
    int centre = 0;                     // site that carries the centre (htn_mps_create: 0; every update moves it)

    template <class T, class F>
    std::shared_ptr<T> cached(const std::string& key, F build) {
        auto it = cache.find(key);
        if (it != cache.end()) {
            ++hits;
            return std::const_pointer_cast<T>(std::static_pointer_cast<const T>(it->second));
        }
        if (cache.size() > 20000) cache.clear();
        ++misses;
        std::shared_ptr<T> v = build();
        if (v) cache[key] = v;
        return v;
    }
    static std::string ikey(const char* tag, int i) {
        std::string k(tag);
        k.append((const char*)&i, sizeof(i));
        return k;
    }
    DBufP dalloc(size_t bytes) {
        auto b = std::make_shared<DBuf>(be, bytes);
        return b->p ? b : nullptr;
    }
    DView zalloc(int64_t n, bool zero) {
        DView v;
        v.base = dalloc(sizeof(cplx) * (size_t)std::max<int64_t>(n, 1));
        if (v.base && zero) be->zero(v.base->p, sizeof(cplx) * (size_t)std::max<int64_t>(n, 1));
        return v;
    }
    DView ws;                      // split-K workspace of the grouped GEMM: [tickets | slabs], grown on demand
    int64_t ws_slots = -1;
    int ensure_ws(int slots) {
        if (slots <= ws_slots) return 0;
        const int64_t want = std::max<int64_t>(2 * (int64_t)slots, 256);
        ws = zalloc(HTN_WS_ELEMS(want), false);
        if (!ws.base) return set_error("device allocation of the split-K workspace failed");
        if (be->zero(ws.ptr(), sizeof(cplx) * HTN_WS_TICKET_ELEMS)) return 1;      // tickets start at zero; the kernel resets them
        ws_slots = want;
        return 0;
    }
    int upload_tasks(const Tasks& t_in, DevTasks& d) {
        Tasks balanced;
        const Tasks* tp = &t_in;
        d.ws_slots = 0;
        if (be->kind() == HTN_BACKEND_HIP && t_in.ntiles > 0) {        // (the CPU baseline runs tiles as they are)
            balanced = t_in;
            balanced.tiles.resize((size_t)t_in.ntiles);
            d.ws_slots = balance_tiles(balanced, 256);
            tp = &balanced;
        }
        const Tasks& t = *tp;
        const size_t tb = (sizeof(htn_tile) * t.tiles.size() + 63) / 64 * 64, sb = sizeof(htn_seg) * t.segs.size();
        d.mem = dalloc(tb + sb);
        if (!d.mem) return set_error("device allocation of a task list failed");
        if (be->upload(d.mem->p, t.tiles.data(), sizeof(htn_tile) * t.tiles.size())) return 1;
        if (be->upload((char*)d.mem->p + tb, t.segs.data(), sb)) return 1;
        d.tiles = (const htn_tile*)d.mem->p;
        d.segs = (const htn_seg*)((char*)d.mem->p + tb);
        d.ntiles = t.ntiles;
        d.nsegs = t.nsegs;
        d.flops = t.flops;
        return 0;
    }
    // (htn_plan_apply_dump shows the lists BEFORE balancing: those are what the Python statement of the planner emits)
    SiteLayoutP site_layout(char kind, BondP bl, BondP br) {
        return cached<const SiteLayout>(std::string("slay") + kind + bl->key + "|" + br->key,
                                        [&] { return build_site_layout(mpo->sym, kind, bl, br); });
    }
    ThetaLayoutP theta_layout(BondP bl, BondP br) {
        return cached<const ThetaLayout>(std::string("tl") + bl->key + "|" + br->key,
                                         [&] { return build_theta_layout(mpo->sym, bl, br); });
    }
    int gemm(const DevTasks& d, std::initializer_list<std::pair<int, const void*>> bufs) {
        if (d.ntiles == 0) return 0;
        if (ensure_ws(d.ws_slots)) return 1;
        const void* table[HTN_MAX_BUFS] = {nullptr};
        for (auto& kv : bufs) table[kv.first] = kv.second;
        table[HTN_BUF_WS] = ws.ptr();
        return be->grouped_gemm(table, d.tiles, d.ntiles, d.segs);
    }

    // compiled two-stage plan: upload t1 and t2, record zsize (and the flops)
    template <class C, class P>
    std::shared_ptr<C> compile2(std::shared_ptr<C> e, const P& p) {
        if (upload_tasks(p.t1, e->d1) || upload_tasks(p.t2, e->d2)) return nullptr;
        e->zsize = p.zsize;
        e->flops = p.t1.flops + p.t2.flops;
        return e;
    }
    int env_step(char side, int i);
    int left_env(int i) { return env_step('L', i); }
    int right_env(int i) { return env_step('R', i); }
    // overlap transfers with `ket` as the ket state (this = bra): in -> out across site i
    int ovl_step(char side, const htn_mps* ket, int i, const OvlLayoutP& inl, const DView& in, OvlLayoutP* outl, DView* out);
    int ovl_boundary(const htn_mps* ket, int b, OvlLayoutP* outl, DView* out);
    int ovl_project(const OrthState& o, int i, const ThetaLayout& tl, cplx* dst);
    int orth_attach(htn_mps* const* others, int n);
    void orth_detach();
    // H_eff applies (two-site: make_apply, one-site: make_apply1)
    std::shared_ptr<ApplyC> compile_apply(ApplyPlan& p, bool deal_y);
    std::shared_ptr<ApplyC> make_apply(int i, const ThetaLayout& tl);
    std::shared_ptr<ApplyC> make_apply1(int i, const SiteLayout& lay);
    int apply_stages(const ApplyC& ap, const DView& L, const DView& R, const DView& z, htn_gemm_launch* stages);
    int apply_once(const ApplyC& ap, const DView& L, const DView& R, int64_t n, const void* x_host, void* y_host, bool exchange);
    int theta_into(int i, const ThetaLayout& tl, cplx* dst);
    // two-site update: update_bond runs these once each, in this order
    int bond_solve(int i, bool optimise, const htn_sweep_opts& o, StageClock& clk, BondWork& w, const cplx* evolve_dt = nullptr);
    std::shared_ptr<SvdC> make_svd(int i, const ThetaLayout& tl, bool right);
    int bond_svd(int i, bool right, const htn_sweep_opts& o, BondWork& w);
    int bond_truncate(int i, const htn_sweep_opts& o, BondWork& w);
    int bond_finalise(int i, bool right, BondWork& w);
    int bond_advance(int i, bool right);
    void bond_spectrum(int i, const BondWork& w);
    void fill_stats(htn_bond_stats* st, int bond, int direction, const Solve& sol, int64_t env_elems, int jacobi_sweeps,
                    int64_t svd_flops, double trunc_weight, const StageClock& clk);
    int update_bond(int i, int direction, bool right, bool optimise, const htn_sweep_opts& o, htn_bond_stats* st,
                    const cplx* evolve_dt = nullptr, double* log_growth = nullptr);
    int sweep(const htn_sweep_opts& o, htn_bond_stats* st, double* E);
    // time evolution (htn_bond_evolve / htn_site_evolve / htn_tdvp2_sweep / htn_mps_set_mpo)
    int evolve_checks(const htn_sweep_opts& o, const char* who) const;
    int evolve_site(int i, cplx dt, const htn_sweep_opts& o, htn_bond_stats* st, double* log_growth);
    int tdvp2_sweep(cplx dt, const htn_sweep_opts& o, htn_bond_stats* st, double* E, double* log_norm);
    int set_mpo(htn_mpo* m);
    // one-site DMRG (htn_site_update / htn_dmrg1_sweep)
    int relay(const SiteLayout& from, const cplx* src, const SiteLayout& to, cplx* dst);
    int update_site(int i, int direction, bool optimise, const htn_sweep_opts& o, htn_bond_stats* st);
    int sweep1(const htn_sweep_opts& o, htn_bond_stats* st, double* E);
    // two-point correlation functions (htn_mps_correlator)
    int correlator(const htn_corr_channel& ch, cplx* out_host, double* norm_host);
};

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
    if (!c) return 1;
    DView z = zalloc(c->zsize, false), out = zalloc(c->lay->size, false);
    if (!z.base || !out.base) return set_error("device allocation failed (%s environment)", left ? "left" : "right");
    if (gemm(c->d1, {{left ? BUF_L : BUF_R, ebuf[from].ptr()}, {BUF_S1, site_buf[i].ptr()}, {BUF_Z, z.ptr()}})) return 1;
    if (gemm(c->d2, {{BUF_S1, site_buf[i].ptr()}, {BUF_Z, z.ptr()}, {BUF_Y, out.ptr()}})) return 1;
    elay[to] = c->lay;
    ebuf[to] = out;
    return 0;
}

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
int htn_mps::bond_solve(int i, bool optimise, const htn_sweep_opts& o, StageClock& clk, BondWork& w, const cplx* evolve_dt) {
    w.tl = theta_layout(bonds[i], bonds[i + 2]);
    const ThetaLayout& tl = *w.tl;
    Solve& s = w.sol;
    const int64_t n = s.n = tl.size;
    const int kd = o.krylovdim;
    if (n <= 0) return set_error("htn_bond_update: empty two-site tensor on bond %d", i);
    w.V = zalloc((int64_t)(kd + 2) * n, false);
    if (!w.V.base) return set_error("device allocation of the Krylov basis failed (%lld elements)", (long long)((kd + 2) * n));
    if (theta_into(i, tl, w.V.ptr())) return 1;                // theta -> V[0] (the Lanczos driver normalises it)
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
    if (evolve_dt) {            // (evolving update: theta <- exp(-i dt H_eff) theta; E = <theta|H_eff|theta> before the step)
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
                         const cplx* evolve_dt, double* log_growth) {
    if (i < 0 || i + 1 >= L) return set_error("htn_bond_update: bond index %d out of range", i);
    StageClock clk(be, o.profile);
    BondWork w;
    if (bond_solve(i, optimise, o, clk, w, evolve_dt)) return 1;          // (laps clk.plan and clk.lanczos)
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
    energy = w.sol.E;
    centre = right ? i + 1 : i;
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

static int site1_checks(const htn_mps* m, int i, const char* who) {
    if (i < 0 || i >= m->L) return set_error("%s: site %d out of range", who, i);
    if (m->centre != i) return set_error("%s: the centre is on site %d, not on site %d", who, m->centre, i);
    if (!m->orth.empty()) return set_error("%s: one-site updates of a state with attached orthogonal states are not supported", who);
    if (m->ctx->world > 1 || m->ctx->shard || m->be->has_comm())
        return set_error("%s: one-site updates on a context with a communicator are not supported", who);
    if (!m->Llay[i] || !m->Rlay[i + 1] || m->Llay[i]->bond->key != m->bonds[i]->key || m->Rlay[i + 1]->bond->key != m->bonds[i + 1]->key)
        return set_error("%s: the environments of site %d were built on other bond tables: run a two-site sweep first", who, i);
    return 0;
}

int htn_mps::update_site(int i, int direction, bool optimise, const htn_sweep_opts& o, htn_bond_stats* st) {
    if (site1_checks(this, i, "htn_site_update")) return 1;
    if (direction < -1 || direction > 1) return set_error("htn_site_update: direction %d (must be -1, 0 or +1)", direction);
    if ((direction > 0 && i + 1 >= L) || (direction < 0 && i == 0))
        return set_error("htn_site_update: site %d has no neighbour in direction %d", i, direction);
    StageClock clk(be, o.profile);
    const SiteLayoutP cur = site_lay[i];
    const SiteLayoutP lay = direction == 0 ? cur : site_layout(direction > 0 ? 'L' : 'R', bonds[i], bonds[i + 1]);
    Solve s;
    const int64_t n = s.n = lay->size;
    if (n <= 0) return set_error("htn_site_update: empty site tensor on site %d", i);
    for (const auto& M : lay->mats)      // a full-rank gauge move needs the long side along the orthonormal direction
        if (direction != 0 && (lay->kind == 'L' ? M.rows < M.cols : M.cols < M.rows))
            return set_error("htn_site_update: sector (%d, %d) of site %d is a %d x %d block, its bond is wider than the rest of the "
                             "site supports: run a two-site sweep first", M.c.N, M.c.j, i, M.rows, M.cols);
    if (direction != 0 && site_lay[i + direction]->kind != (direction > 0 ? 'R' : 'L'))
        return set_error("htn_site_update: site %d is not in %s layout", i + direction, direction > 0 ? "right" : "left");
    const int kd = o.krylovdim;
    DView V = zalloc((int64_t)(kd + 2) * n, false);
    if (!V.base) return set_error("device allocation of the Krylov basis failed (%lld elements)", (long long)((kd + 2) * n));
    if (relay(*cur, site_buf[i].ptr(), *lay, V.ptr())) return 1;
    s.ap = make_apply1(i, *lay);
    if (!s.ap) return 1;
    DView z = zalloc(s.ap->zsize, false);
    if (!z.base) return set_error("device allocation failed (one-site apply)");
    htn_gemm_launch stages[2];
    const int ns = apply_stages(*s.ap, Lbuf[i], Rbuf[i + 1], z, stages);
    if (ns < 0) return 1;
    clk.plan = clk.lap();
    if (be->lanczos(stages, ns, BUF_X, BUF_Y, V.ptr(), n, kd, optimise ? o.lanczos_tol : 1e300, o.maxrestart, 0, nullptr, ctx, &s.E, &s.nmv,
                    &s.res, be->timing ? &s.mv_ms : nullptr))
        return 1;
    clk.lanczos = clk.lap();
    // ---- the optimised centre, then the gauge move ----
    DView out = zalloc(n, false);
    if (!out.base) return set_error("device allocation failed (site tensor)");
    if (relay(*lay, V.ptr(), *lay, out.ptr())) return 1;
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
    Solve s;
    const int64_t n = s.n = lay->size;
    if (n <= 0) return set_error("htn_site_evolve: empty site tensor on site %d", i);
    const int kd = o.krylovdim;
    DView V = zalloc((int64_t)(kd + 2) * n, false);
    if (!V.base) return set_error("device allocation of the Krylov basis failed (%lld elements)", (long long)((kd + 2) * n));
    if (relay(*lay, site_buf[i].ptr(), *lay, V.ptr())) return 1;
    s.ap = make_apply1(i, *lay);
    if (!s.ap) return 1;
    DView z = zalloc(s.ap->zsize, false);
    if (!z.base) return set_error("device allocation failed (one-site apply)");
    htn_gemm_launch stages[2];
    const int ns = apply_stages(*s.ap, Lbuf[i], Rbuf[i + 1], z, stages);
    if (ns < 0) return 1;
    clk.plan = clk.lap();
    if (be->krylov_expm(stages, ns, BUF_X, BUF_Y, V.ptr(), n, kd, dt.real(), dt.imag(), o.lanczos_tol, o.maxrestart, 0, nullptr, ctx, &s.growth,
                        &s.E, &s.nmv, &s.res, be->timing ? &s.mv_ms : nullptr))
        return 1;
    clk.lanczos = clk.lap();
    DView out = zalloc(n, false);
    if (!out.base) return set_error("device allocation failed (site tensor)");
    if (relay(*lay, V.ptr(), *lay, out.ptr())) return 1;
    site_buf[i] = out;
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

// the quench: another Hamiltonian under the same state.  Everything that was planned or contracted with the old MPO goes (the
// plan cache, the environments); the boundaries and the right environments are rebuilt as mps_finish builds them.
static int mps_finish(htn_mps* e, const void* left_env_host, const void* right_env_host, const DView* left_dev, const DView* right_dev);
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

// ---- construction of an htn_mps: shared by htn_mps_create and the IDMRG2 driver ------------------------------------
static htn_mps* mps_new(htn_ctx* ctx, const htn_mpo* mpo) {
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
struct MpsGuard {              // drops a half-built htn_mps (and the references it took) on an error return
    htn_mps* p;
    ~MpsGuard() {
        if (p) htn_mps_destroy(p);
    }
};
static int mps_load_bonds(htn_mps* e, const int32_t* bond_ptr, const htn_sector* sectors) {
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
static int mps_load_sites(htn_mps* e, const int32_t* sub_ptr, const htn_subblock* subs, const int64_t* data_ptr, const void* data_host) {
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
static int mps_finish(htn_mps* e, const void* left_env_host, const void* right_env_host, const DView* left_dev, const DView* right_dev) {
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

static void idmrg_free(htn_idmrg* d) {
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

// =====================================================================================================================
// C ABI
// =====================================================================================================================
extern "C" {

const char* htn_last_error(void) { return err_buf(); }
int htn_abi_version(void) { return HTN_ABI_VERSION; }

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
    if (m->mpo.sites.front().left.size() != 1 || m->mpo.sites.back().right.size() != 1) {
        // a window inside a larger system (iDMRG) has full-width boundary bonds: allowed, the boundary environments
        // then must be supplied to htn_mps_create
    }
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

static htn_sweep_opts norm_opts(const htn_sweep_opts* o) {
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

int htn_bond_update(htn_mps* mps, int32_t i, int32_t direction, int32_t placement, int32_t optimise, const htn_sweep_opts* opts,
                    htn_bond_stats* stats) {
    if (mps->be->activate()) return 1;
    return mps->update_bond(i, direction, placement == 0, optimise != 0, norm_opts(opts), stats);
}
int htn_dmrg2_sweep(htn_mps* mps, const htn_sweep_opts* opts, htn_bond_stats* stats, double* energy) {
    if (mps->be->activate()) return 1;
    return mps->sweep(norm_opts(opts), stats, energy);
}

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
int htn_mps_set_mpo(htn_mps* mps, const htn_mpo* mpo) {
    if (!mps || !mpo) return set_error("htn_mps_set_mpo: bad arguments");
    if (mps->be->activate()) return 1;
    return mps->set_mpo(const_cast<htn_mpo*>(mpo));
}
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

int htn_mps_set_orthogonal(htn_mps* mps, const htn_mps* const* others, int32_t n) {
    if (!mps || n < 0 || (n > 0 && !others)) return set_error("htn_mps_set_orthogonal: bad arguments");
    if (n > 8) return set_error("htn_mps_set_orthogonal: at most 8 attached states (%d given)", n);
    if (mps->be->activate()) return 1;
    if (n == 0) {
        mps->orth_detach();
        return 0;
    }
    if (mps->ctx->world > 1) return set_error("htn_mps_set_orthogonal: not available on a context with a communicator");
    std::vector<htn_mps*> list;
    for (int k = 0; k < n; ++k) {
        htn_mps* o = const_cast<htn_mps*>(others[k]);
        if (!o || o == mps) return set_error("htn_mps_set_orthogonal: state %d is NULL or the state itself", k);
        if (o->ctx != mps->ctx) return set_error("htn_mps_set_orthogonal: state %d lives in a different context", k);
        if (o->L != mps->L) return set_error("htn_mps_set_orthogonal: state %d has %d sites, this state %d", k, o->L, mps->L);
        const Sym &a = mps->mpo->sym, &b = o->mpo->sym;
        bool same = a.kind == b.kind && a.n_site == b.n_site;
        for (int q = 0; same && q < a.n_site; ++q) same = a.site[q] == b.site[q];
        if (!same) return set_error("htn_mps_set_orthogonal: state %d has a different symmetry", k);
        if (o->bonds[0]->key != mps->bonds[0]->key || o->bonds[o->L]->key != mps->bonds[mps->L]->key)
            return set_error("htn_mps_set_orthogonal: state %d is in a different total sector", k);
        if (mps->bonds[0]->dim_full(a) != 1 || mps->bonds[mps->L]->secs.size() != 1 || mps->bonds[mps->L]->dims[0] != 1)
            return set_error("htn_mps_set_orthogonal: the end bonds must be single sectors of dimension 1 (a finite chain)");
        list.push_back(o);
    }
    return mps->orth_attach(list.data(), n);
}
int32_t htn_mps_orthogonal_count(const htn_mps* mps, int32_t* dropped_host) {
    if (dropped_host) *dropped_host = mps->orth_dropped;
    return (int32_t)mps->orth.size();
}
int htn_mps_overlap(htn_mps* a, const htn_mps* b, double* out_host) {
    if (!a || !b || !out_host) return set_error("htn_mps_overlap: bad arguments");
    if (a->ctx != b->ctx) return set_error("htn_mps_overlap: the states live in different contexts");
    if (a->L != b->L) return set_error("htn_mps_overlap: %d and %d sites", a->L, b->L);
    if (a->be->activate()) return 1;
    out_host[0] = out_host[1] = 0.0;
    if (a->bonds[0]->key != b->bonds[0]->key || a->bonds[a->L]->key != b->bonds[b->L]->key) return 0;      // different total sectors
    OvlLayoutP lay;
    DView buf;
    if (a->ovl_boundary(b, 0, &lay, &buf)) return 1;
    for (int i = 0; i < a->L; ++i) {
        OvlLayoutP nl;
        DView nb;
        if (a->ovl_step('L', b, i, lay, buf, &nl, &nb)) return 1;
        lay = nl;
        buf = nb;
    }
    if (lay->size != 1) return set_error("htn_mps_overlap: the right end bonds are not one sector of dimension 1");
    cplx v;
    if (a->be->download(&v, buf.ptr(), sizeof(v))) return 1;
    out_host[0] = v.real();
    out_host[1] = v.imag();
    return 0;
}

int htn_mps_correlator(htn_mps* mps, const htn_corr_channel* ch, void* out_host, double* norm_host) {
    if (!mps || !ch || !out_host) return set_error("htn_mps_correlator: bad arguments");
    if (mps->be->activate()) return 1;
    return mps->correlator(*ch, (cplx*)out_host, norm_host);
}

int64_t htn_mps_theta_size(htn_mps* mps, int32_t i) {
    if (i < 0 || i + 1 >= mps->L) return -1;
    return mps->theta_layout(mps->bonds[i], mps->bonds[i + 2])->size;
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
int htn_heff2_apply(htn_mps* mps, int32_t i, const void* x_host, void* y_host) {
    if (i < 0 || i + 1 >= mps->L) return set_error("htn_heff2_apply: bond out of range");
    if (mps->be->activate()) return 1;
    ThetaLayoutP tl = mps->theta_layout(mps->bonds[i], mps->bonds[i + 2]);
    auto ap = mps->make_apply(i, *tl);
    if (!ap) return 1;
    return mps->apply_once(*ap, mps->Lbuf[i], mps->Rbuf[i + 2], tl->size, x_host, y_host, mps->ctx->shard);
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
int32_t htn_mps_env_bond(const htn_mps* mps, int32_t side, int32_t b, htn_sector* out) {
    if (b < 0 || b > mps->L) return -1;
    const EnvLayoutP& l = side == 0 ? mps->Llay[b] : mps->Rlay[b];
    if (!l) return -1;
    const Bond& B = *l->bond;
    if (out)
        for (size_t k = 0; k < B.secs.size(); ++k) out[k] = {B.secs[k].N, B.secs[k].j, B.dims[k]};
    return (int32_t)B.secs.size();
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

int htn_idmrg_create(htn_ctx* ctx, const htn_mpo* mpo, const htn_idmrg_opts* opts, htn_idmrg** out) {
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
void htn_idmrg_destroy(htn_idmrg* d) { idmrg_free(d); }
int32_t htn_idmrg_boundary(const htn_idmrg* d, int32_t side, htn_sector* out) {
    if (!d || side < 0 || side > 1) return -1;
    const Bond& B = side ? *d->bR : *d->bL;
    if (out)
        for (size_t k = 0; k < B.secs.size(); ++k) out[k] = {B.secs[k].N, B.secs[k].j, B.dims[k]};
    return (int32_t)B.secs.size();
}
int htn_idmrg_step(htn_idmrg* d, const int32_t* bond_ptr, const htn_sector* sectors, const int32_t* sub_ptr, const htn_subblock* subs,
                   const int64_t* data_ptr, const void* data_host, htn_idmrg_stats* stats) {
    if (!d) return set_error("htn_idmrg_step: NULL handle");
    if (d->failed) return set_error("htn_idmrg_step: an earlier step failed; the driver cannot continue");
    if (d->finished) return set_error("htn_idmrg_step: the growth has finished (converged or maxiter)");
    if (d->be->activate()) return 1;
    return d->run_step(bond_ptr, sectors, sub_ptr, subs, data_ptr, data_host, stats);
}
int htn_idmrg_window(htn_idmrg* d, htn_mps** out) {
    if (!d || !out) return set_error("htn_idmrg_window: NULL argument");
    if (!d->win) return set_error("htn_idmrg_window: no step has run yet");
    ++d->win->refs;
    *out = d->win;
    return 0;
}

}  // extern "C"
