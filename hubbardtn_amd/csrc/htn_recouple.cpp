// Fusion rules of the site multiplets (Sym) and the closed-form SU(2) recoupling coefficients of the planners: Wigner 6j / 9j
// by the Racah formula, cached, and the coef_* products that become the alpha of a task-list segment.  Host C++ (no HIP).
// NOT a translation unit of its own: #included by htn_plan.cpp (one unit, see its head); never name it on a build line.
#include "htn_core.h"

namespace htn {

// ---- symmetry ----------------------------------------------------------------------------------------------------
bool Sym::triangle(int a, int b, int c) const {
    if (!su2()) return a + b == c;
    return abs(a - b) <= c && c <= a + b && ((a + b + c) & 1) == 0;
}
void Sym::fuse(Sec sec, int s, std::vector<Sec>& out) const {
    out.clear();
    const Sec m = site[s];
    const int N = wrapN(sec.N + m.N);
    if (!su2()) {
        out.push_back({N, sec.j + m.j});
        return;
    }
    for (int jj = abs(sec.j - m.j); jj <= sec.j + m.j; jj += 2) out.push_back({N, jj});
}
void Sym::split(Sec sec, int s, std::vector<Sec>& out) const {
    out.clear();
    const Sec m = site[s];
    if (kind != HTN_SYM_SU2 && sec.N < m.N) return;
    const int N = wrapN(sec.N - m.N);
    if (!su2()) {
        out.push_back({N, sec.j - m.j});
        return;
    }
    for (int jj = abs(sec.j - m.j); jj <= sec.j + m.j; jj += 2) out.push_back({N, jj});
}

// ---- Wigner symbols (Racah formula; validated against brute-force CG contraction, tests/test_wigner.py) ---------
static double fact(int n) {
    static double tab[171];
    static std::once_flag once;
    std::call_once(once, [] {
        tab[0] = 1.0;
        for (int i = 1; i <= 170; ++i) tab[i] = tab[i - 1] * i;
    });
    return tab[n];
}
static inline bool tri(int a, int b, int c) { return abs(a - b) <= c && c <= a + b && ((a + b + c) & 1) == 0; }
static double delta(int a, int b, int c) {
    return fact((a + b - c) / 2) * fact((a - b + c) / 2) * fact((-a + b + c) / 2) / fact((a + b + c) / 2 + 1);
}
static std::mutex g_wig_mu;
static std::unordered_map<uint64_t, double> g_6j, g_9j, g_cl, g_cr;
static inline uint64_t pack(std::initializer_list<int> v) {
    uint64_t h = 0;
    for (int x : v) h = (h << 7) | (uint64_t)(x & 127);
    return h;
}
double wigner6j(int j1, int j2, int j3, int j4, int j5, int j6) {
    if (!(tri(j1, j2, j3) && tri(j1, j5, j6) && tri(j4, j2, j6) && tri(j4, j5, j3))) return 0.0;
    const uint64_t key = pack({j1, j2, j3, j4, j5, j6});
    {
        std::lock_guard<std::mutex> lk(g_wig_mu);
        auto it = g_6j.find(key);
        if (it != g_6j.end()) return it->second;
    }
    const double pref = sqrt(delta(j1, j2, j3) * delta(j1, j5, j6) * delta(j4, j2, j6) * delta(j4, j5, j3));
    const int a1 = (j1 + j2 + j3) / 2, a2 = (j1 + j5 + j6) / 2, a3 = (j4 + j2 + j6) / 2, a4 = (j4 + j5 + j3) / 2;
    const int b1 = (j1 + j2 + j4 + j5) / 2, b2 = (j2 + j3 + j5 + j6) / 2, b3 = (j3 + j1 + j6 + j4) / 2;
    double s = 0.0;
    for (int t = std::max(std::max(a1, a2), std::max(a3, a4)); t <= std::min(b1, std::min(b2, b3)); ++t)
        s += ((t & 1) ? -1.0 : 1.0) * fact(t + 1) /
             (fact(t - a1) * fact(t - a2) * fact(t - a3) * fact(t - a4) * fact(b1 - t) * fact(b2 - t) * fact(b3 - t));
    const double r = pref * s;
    std::lock_guard<std::mutex> lk(g_wig_mu);
    g_6j[key] = r;
    return r;
}
double wigner9j(int j1, int j2, int j3, int j4, int j5, int j6, int j7, int j8, int j9) {
    if (!(tri(j1, j2, j3) && tri(j4, j5, j6) && tri(j7, j8, j9) && tri(j1, j4, j7) && tri(j2, j5, j8) && tri(j3, j6, j9)))
        return 0.0;
    const uint64_t key = pack({j1, j2, j3, j4, j5, j6, j7, j8, j9});
    {
        std::lock_guard<std::mutex> lk(g_wig_mu);
        auto it = g_9j.find(key);
        if (it != g_9j.end()) return it->second;
    }
    const int lo = std::max(std::max(abs(j1 - j9), abs(j4 - j8)), abs(j2 - j6));
    const int hi = std::min(std::min(j1 + j9, j4 + j8), j2 + j6);
    double s = 0.0;
    for (int x = lo; x <= hi; x += 2)
        s += ((x & 1) ? -1.0 : 1.0) * (x + 1) * wigner6j(j1, j4, j7, j8, j9, x) * wigner6j(j2, j5, j8, j4, x, j6) *
             wigner6j(j3, j6, j9, x, j1, j2);
    std::lock_guard<std::mutex> lk(g_wig_mu);
    g_9j[key] = s;
    return s;
}
// L'[a',w',a] += coef * A[b',s',a']^+ L[b',w,b] W[w,s',s,w'] A[b,s,a]
double coef_left(int jbp, int k, int jb, int jsp, int js, int kop, int jap, int kp, int ja) {
    return sqrt((double)((jbp + 1) * (jsp + 1) * (ja + 1) * (kp + 1))) * wigner9j(jb, k, jbp, js, kop, jsp, ja, kp, jap);
}
// R[c',w,c] += coef * conj(B[c',s',b']) W[w,s',s,w'] R[b',w',b] B[c,s,b]
double coef_right(int jcp, int k, int jc, int jsp, int js, int kop, int jbp, int kp, int jb) {
    return wigner9j(jc, k, jcp, js, kop, jsp, jb, kp, jbp) * sqrt((double)((kp + 1) * (jsp + 1))) * (jc + 1) * (jbp + 1) /
           sqrt((double)((jb + 1) * (jcp + 1)));
}
// y[a',s1',c',s2',b'] += coef * L[a',w,a] theta[a,s1,c,s2,b] R[b',w',b]^T
double coef_apply(int ja, int jap, int k, int js1, int js1p, int kop1, int km, int jc, int jcp, int js2, int js2p,
                  int kop2, int kp, int jb, int jbp) {
    return coef_left(jap, k, ja, js1p, js1, kop1, jcp, km, jc) * coef_left(jcp, km, jc, js2p, js2, kop2, jbp, kp, jb) *
           (jbp + 1) / (jb + 1);
}

}  // namespace htn
