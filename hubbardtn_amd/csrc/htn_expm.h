// Host side of the Krylov exponential x = exp(-i dt H) x0 (htn_krylov_expm_z and htn::Backend::krylov_expm): what is done with
// the tridiagonal coefficients (alpha_j, beta_j) of an orthonormal Lanczos basis.  Plain C++, header only: the device driver
// (htn_krylov.hip) and the host statement of the method (htn_backend_host.cpp) take the SAME decisions from the same numbers.
//
//   after step m:   T_m = tridiag(alpha_0..alpha_{m-1}; beta_0..beta_{m-2}) is diagonalised completely (implicit QL, m <= 31),
//                   c = exp(-i dt T_m) e_1,   est = beta_m |dt| |c_m|   (Saad's a-posteriori estimate, SIAM J. Numer. Anal. 29, 1992)
//   stop when est < tol, when beta_m < 1e-14 x (largest |alpha| or beta seen: an invariant subspace, the result is exact),
//   or at m = krylovdim.  Not converged there: the fraction s of the remaining time is halved until
//   beta_m |s dt| |c_m(s dt)| < tol s (same T: host work only), that partial step is applied and the basis is rebuilt from its
//   result for the remaining time.
#pragma once
#include <math.h>

#include <complex>
#include <vector>

namespace htn_expm {

typedef std::complex<double> cplx;

// eigenvalues d[0..n) and eigenvectors Z (column major, Z[i + k n] = component i of vector k) of the real symmetric tridiagonal
// matrix with diagonal d and sub-diagonal e[0..n-1) by the implicit QL iteration with Wilkinson shifts.  -> false: no convergence
inline bool tridiag_eig(int n, std::vector<double>& d, std::vector<double> e, std::vector<double>& Z) {
    Z.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) Z[(size_t)i + (size_t)i * n] = 1.0;
    e.resize((size_t)n, 0.0);
    e[(size_t)n - 1] = 0.0;
    for (int l = 0; l < n; ++l) {
        for (int iter = 0;; ++iter) {
            int m = l;
            for (; m < n - 1; ++m) {
                const double dd = fabs(d[m]) + fabs(d[m + 1]);
                if (fabs(e[m]) <= 2.3e-16 * dd) break;
            }
            if (m == l) break;
            if (iter == 80) return false;
            double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
            double r = hypot(g, 1.0);
            g = d[m] - d[l] + e[l] / (g + copysign(r, g));
            double s = 1.0, c = 1.0, p = 0.0;
            int i = m - 1;
            for (; i >= l; --i) {
                double f = s * e[i];
                const double b = c * e[i];
                e[i + 1] = r = hypot(f, g);
                if (r == 0.0) {
                    d[i + 1] -= p;
                    e[m] = 0.0;
                    break;
                }
                s = f / r;
                c = g / r;
                g = d[i + 1] - p;
                r = (d[i] - g) * s + 2.0 * c * b;
                d[i + 1] = g + (p = s * r);
                g = c * r - b;
                for (int k = 0; k < n; ++k) {
                    f = Z[(size_t)k + (size_t)(i + 1) * n];
                    Z[(size_t)k + (size_t)(i + 1) * n] = s * Z[(size_t)k + (size_t)i * n] + c * f;
                    Z[(size_t)k + (size_t)i * n] = c * Z[(size_t)k + (size_t)i * n] - s * f;
                }
            }
            if (r == 0.0 && i >= l) continue;
            d[l] -= p;
            e[l] = g;
            e[m] = 0.0;
        }
    }
    return true;
}

// The decisions of one solve.  Per restart cycle: begin_cycle(); step(alpha, beta) after every Lanczos step until it returns true;
// then finish(): the coefficients of the step that is applied (c, |c|), the fraction of the remaining time it covers.
struct Expm {
    double dt_re = 0.0, dt_im = 0.0, tol = 0.0;
    double remaining = 1.0;        // fraction of dt still to be applied
    double growth = 1.0;           // |x| / |x0| so far
    double alpha0 = 0.0, est = 0.0, amax = 0.0;
    double err_total = 0.0;        // sum of the estimates of the steps applied
    bool have_alpha0 = false, converged = false;
    std::vector<double> alphas, betas, lam, Z;
    std::vector<cplx> c;
    double beta_m = 0.0;

    void begin_cycle() {
        alphas.clear();
        betas.clear();
        converged = false;
    }
    // c = exp(-i (f dt) T_m) e_1 from the eigen-decomposition at hand
    void coefficients(double f) {
        const int m = (int)alphas.size();
        c.assign((size_t)m, cplx(0.0, 0.0));
        for (int k = 0; k < m; ++k) {
            const double ph = -f * dt_re * lam[k], gr = f * dt_im * lam[k];      // -i (dr + i di) lam = di lam - i dr lam
            const cplx w = exp(gr) * cplx(cos(ph), sin(ph)) * Z[(size_t)k * m];
            for (int i = 0; i < m; ++i) c[i] += Z[(size_t)i + (size_t)k * m] * w;
        }
    }
    double estimate(double f) const { return beta_m * f * hypot(dt_re, dt_im) * std::abs(c.back()); }
    // -> true: the cycle ends here (converged, invariant subspace, or m = krylovdim); < 0 through `bad`: the QL iteration failed
    bool step(double alpha, double beta, int krylovdim, bool* bad) {
        if (!have_alpha0) alpha0 = alpha, have_alpha0 = true;
        alphas.push_back(alpha);
        beta_m = beta;
        amax = fmax(amax, fmax(fabs(alpha), beta));
        const int m = (int)alphas.size();
        lam = alphas;
        *bad = !tridiag_eig(m, lam, betas, Z);
        if (*bad) return true;
        coefficients(remaining);
        est = estimate(remaining);
        const bool invariant = beta < 1e-14 * fmax(amax, 1e-300);
        if (invariant) est = 0.0;
        converged = est < tol * remaining || invariant || hypot(dt_re, dt_im) == 0.0;
        if (converged || m == krylovdim) return true;
        betas.push_back(beta);
        return false;
    }
    // the step to apply at the end of a cycle: all of the remaining time if converged, else the largest halved fraction that
    // meets the tolerance.  -> false: no fraction down to 2^-60 does
    bool finish() {
        double s = 1.0;
        if (!converged) {
            for (int h = 0;; ++h) {
                if (h == 60) return false;
                s *= 0.5;
                coefficients(s * remaining);
                est = estimate(s * remaining);
                if (est < tol * s * remaining) break;
            }
        }
        err_total += est;
        double nn = 0.0;
        for (const cplx& v : c) nn += std::norm(v);
        nn = sqrt(nn);
        growth *= nn;
        for (cplx& v : c) v /= nn;
        remaining = converged ? 0.0 : remaining * (1.0 - s);
        return true;
    }
};

}  // namespace htn_expm
