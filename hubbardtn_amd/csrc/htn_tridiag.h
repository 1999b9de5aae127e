// Lowest eigenpair of the Lanczos tridiagonal matrix, on the host: ONE statement for the device driver (htn_krylov.hip) and the
// host statement of the projected solve (htn_backend_host.cpp), so that both stop at the same step from the same coefficients.
#pragma once
#include <math.h>

#include <vector>

namespace htn {

// number of eigenvalues < x of the symmetric tridiagonal (a, b): sign changes of the Sturm sequence
inline int sturm_count(const std::vector<double>& a, const std::vector<double>& b, double x) {
    int cnt = 0;
    double d = 1.0;
    const int k = (int)a.size();
    for (int i = 0; i < k; ++i) {
        const double off = i ? b[i - 1] * b[i - 1] : 0.0;
        d = (a[i] - x) - (i ? off / d : 0.0);
        if (d == 0.0) d = 1e-300;
        if (d < 0.0) ++cnt;
    }
    return cnt;
}

// lowest eigenpair of the symmetric tridiagonal (alpha, beta): bisection on the Sturm sequence for the eigenvalue, then inverse
// iteration with a shift just below it (T - mu I is positive definite, so the LDL^T tridiagonal solve needs no pivoting).
// O(k) per step: microseconds for k <= 64.
inline void tridiag_lowest(const std::vector<double>& alpha, const std::vector<double>& beta, double* eig, std::vector<double>& vec) {
    const int k = (int)alpha.size();
    double lo = alpha[0], hi = alpha[0];
    for (int i = 0; i < k; ++i) {
        const double r = (i ? fabs(beta[i - 1]) : 0.0) + (i + 1 < k ? fabs(beta[i]) : 0.0);
        lo = fmin(lo, alpha[i] - r);
        hi = fmax(hi, alpha[i] + r);
    }
    const double scale = fmax(fabs(lo), fabs(hi)) + 1e-300;
    hi = hi + 1e-12 * scale;
    for (int it = 0; it < 200 && hi - lo > 4e-16 * scale; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (sturm_count(alpha, beta, mid) >= 1) hi = mid;
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
    for (int i = 0; i < k; ++i) vec[i] = (i & 1) ? -0.7 : 1.0;   // not orthogonal to the lowest vector in practice
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

}  // namespace htn
