// Host side of the shifted linear solve (z - H) x = b (htn_krylov_solve_z and htn::Backend::krylov_solve): what is done with the
// tridiagonal coefficients (alpha_j, beta_j) of an orthonormal Lanczos basis.  Plain C++, header only: the device driver
// (htn_krylov.hip) and the host statement of the method (htn_backend_host.cpp) take the SAME decisions from the same numbers.
//
// H is Hermitian, so K(z - H, r) = K(H, r): the basis is the one of the eigen-solver and of the exponential.
//   after step m:   minimise | beta_0 e_1 - (z I~ - T~_{m+1,m}) y | over y by Givens rotations on the (m + 1) x m complex
//                   tridiagonal matrix, one new column and one new rotation per step; the residual norm is the modulus of the
//                   last entry of the rotated right-hand side -- no matvec, no back-substitution until the cycle ends
//   stop when |r| <= tol |b|, when beta_m < 1e-14 x (largest |alpha| or beta seen: an invariant subspace, the solve is exact),
//   or at m = krylovdim.  Not converged there: x <- x + V_m y and the basis is rebuilt from r = V_{m+1} rho,
//   rho = beta_0 e_1 - (z I~ - T~) y.  For Im z != 0 the field of values of z - H lies on the line Im = Im z, away from 0, and the
//   restarted minimal residual converges (Elman); for real z it may stagnate, and the driver then reports what remains.
#pragma once
#include <math.h>

#include <complex>
#include <vector>

namespace htn_resolvent {

typedef std::complex<double> cplx;

struct Resolvent {
    cplx z = 0.0;
    double tol = 0.0;
    double bnorm = 0.0;            // |b| of the original right-hand side: the scale of the stopping rule
    double beta0 = 0.0;            // |r| at the start of the cycle
    double amax = 0.0;
    double resid = 0.0;            // |r| / |b| after the last step
    bool converged = false;
    std::vector<double> alphas, betas;         // betas[j] = T~[j + 1][j], one per step taken
    std::vector<cplx> R;                       // rotated columns: R[3 j + d] = entry (j - 2 + d, j), d = 0..2
    std::vector<cplx> gc;                      // rotations: c_j
    std::vector<double> gs;                    //            s_j (real: the sub-diagonal is)
    std::vector<cplx> g;                       // rotated right-hand side, m + 1 entries
    std::vector<cplx> y, rho;                  // finish(): the coefficients of the update and of the next start vector

    void begin_cycle(double r_norm) {
        beta0 = r_norm;
        alphas.clear(), betas.clear(), R.clear(), gc.clear(), gs.clear();
        g.assign(1, cplx(r_norm, 0.0));
        resid = bnorm > 0.0 ? r_norm / bnorm : 0.0;
        converged = r_norm <= tol * bnorm;
    }
    // -> true: the cycle ends here (converged, invariant subspace, or m = krylovdim)
    bool step(double alpha, double beta, int krylovdim) {
        const int j = (int)alphas.size();
        alphas.push_back(alpha);
        betas.push_back(beta);
        amax = fmax(amax, fmax(fabs(alpha), beta));
        // column j of z I~ - T~: rows j - 1, j, j + 1; the rotations j - 2 and j - 1 reach it
        cplx up2 = 0.0, up1 = j > 0 ? cplx(-betas[(size_t)j - 1], 0.0) : cplx(0.0), d = z - alpha;
        if (j > 1) {               // rotation j - 2 on rows (j - 2, j - 1): the column has 0 in row j - 2
            up2 = gs[(size_t)j - 2] * up1;
            up1 = gc[(size_t)j - 2] * up1;
        }
        if (j > 0) {               // rotation j - 1 on rows (j - 1, j)
            const cplx a = up1, b = d;
            up1 = std::conj(gc[(size_t)j - 1]) * a + gs[(size_t)j - 1] * b;
            d = -gs[(size_t)j - 1] * a + gc[(size_t)j - 1] * b;
        }
        const double r = hypot(std::abs(d), beta);
        cplx c(1.0, 0.0);
        double s = 0.0;
        if (r > 0.0) c = d / r, s = -beta / r;
        R.push_back(up2), R.push_back(up1), R.push_back(cplx(r, 0.0));
        gc.push_back(c), gs.push_back(s);
        const cplx gj = g[(size_t)j];
        g[(size_t)j] = std::conj(c) * gj;
        g.push_back(-s * gj);
        const bool invariant = beta < 1e-14 * fmax(amax, 1e-300);
        resid = invariant ? 0.0 : std::abs(g.back()) / bnorm;
        converged = resid <= tol || invariant;
        return converged || j + 1 == krylovdim;
    }
    // y by back-substitution, rho = beta_0 e_1 - (z I~ - T~) y taken from the matrix itself; -> |y|_2
    double finish() {
        const int m = (int)alphas.size();
        y.assign((size_t)m, cplx(0.0));
        for (int i = m - 1; i >= 0; --i) {
            cplx t = g[(size_t)i];
            if (i + 1 < m) t -= R[3 * ((size_t)i + 1) + 1] * y[(size_t)i + 1];
            if (i + 2 < m) t -= R[3 * ((size_t)i + 2)] * y[(size_t)i + 2];
            const cplx rii = R[3 * (size_t)i + 2];
            y[(size_t)i] = std::abs(rii) > 0.0 ? t / rii : cplx(0.0);
        }
        rho.assign((size_t)m + 1, cplx(0.0));
        if (m + 1 > 0) rho[0] = beta0;
        for (int j = 0; j < m; ++j) {
            if (j > 0) rho[(size_t)j - 1] += betas[(size_t)j - 1] * y[(size_t)j];
            rho[(size_t)j] -= (z - alphas[(size_t)j]) * y[(size_t)j];
            rho[(size_t)j + 1] += betas[(size_t)j] * y[(size_t)j];
        }
        double nn = 0.0;
        for (const cplx& v : y) nn += std::norm(v);
        return sqrt(nn);
    }
    double rho_norm() const {
        double nn = 0.0;
        for (const cplx& v : rho) nn += std::norm(v);
        return sqrt(nn);
    }
};

}  // namespace htn_resolvent
