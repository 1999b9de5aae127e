// Jacobi SVD, piece of htn_svd.hip: one-sided rotations of column pairs, the sweep loops, SplitCols / DenseCols, padded fast path
#pragma once

// ----------------------------------------------------------------------------------------------
// batched one-sided (Hestenes) Jacobi SVD, one 16-wave workgroup per coupled-sector block
// ----------------------------------------------------------------------------------------------
// Round-robin (circle) ordering: n-1 rounds of n/2 disjoint column pairs per sweep, rounds separated by
// a workgroup barrier.  The critical path is (#sweeps) x (n-1) rounds x (latency of one round), so the
// kernel is built to make a round short:
//   * a pair is rotated by a GROUP of GS = 16 / 32 / 64 lanes chosen from the column length
//     (m <= 128 / 256 / 512): 1024 / GS pairs rotate concurrently, i.e. one pass per round up to n = 128,
//     and both columns stay in registers between the dot products and the rotation;
//   * the matrix lives in LDS when it fits the dynamic LDS window (round latency ~ LDS instead of L2),
//     otherwise in global memory (L2 resident: a few hundred KB);
//   * sweeps stop early through the quadratic convergence of cyclic Jacobi: a sweep whose largest squared
//     cosine, seen BEFORE the rotations, is below 0.1 tol leaves less than tol^2 behind, so neither the
//     textbook's final "checking" sweep nor the sweep before it is run -- unless the sweep rotated by large angles
//     (columns of nearly equal norm: clustered singular values), where the cosines carry over at first order.
#define JAC_THREADS 1024
#define JAC_MAXEL 8           // column elements per lane kept in registers: m <= GS * JAC_MAXEL

template <int GS>
__device__ __forceinline__ double group_sum(double v) {      // all-reduce inside aligned groups of GS lanes
    v = row_sum16(v);
    if (GS == 16) return v;
    // row sums as wave-uniform scalars (v_readlane) instead of ds_bpermute butterflies; same summation order
    const double a = lane_bcast<0>(v) + lane_bcast<16>(v);
    const double b = lane_bcast<32>(v) + lane_bcast<48>(v);
    if (GS == 32) return (threadIdx.x & 32) ? b : a;
    return a + b;
}

template <int GS>
__device__ __forceinline__ double jacobi_pair(double2* ga, double2* gb, double2* __restrict__ va,
                                              double2* __restrict__ vb, int m, int n, int sub, double tol,
                                              bool accumulate, double zero2, double& t2max) {
    double2 a[JAC_MAXEL], b[JAC_MAXEL];
    double aa = 0.0, bb = 0.0, gr = 0.0, gi = 0.0;
#pragma unroll
    for (int e = 0; e < JAC_MAXEL; ++e) {
        const int i = sub + GS * e;
        if (i < m) {
            a[e] = ga[i];
            b[e] = gb[i];
            aa += a[e].x * a[e].x + a[e].y * a[e].y;
            bb += b[e].x * b[e].x + b[e].y * b[e].y;
            gr += a[e].x * b[e].x + a[e].y * b[e].y;      // conj(a) * b
            gi += a[e].x * b[e].y - a[e].y * b[e].x;
        }
    }
    aa = group_sum<GS>(aa);
    bb = group_sum<GS>(bb);
    gr = group_sum<GS>(gr);
    gi = group_sum<GS>(gi);
    // a column below 1e-15 |G|_F is numerically zero (surplus columns of a wide or rank-deficient block):
    // its direction is rounding noise and must not keep the sweep loop alive
    if (aa <= zero2 || bb <= zero2) return 0.0;
    const double g2 = gr * gr + gi * gi;
    const double ab = aa * bb;
    const double ratio2 = g2 * fast_rcp(ab);          // (|a.b| / (|a||b|))^2
    if (g2 == 0.0 || g2 <= tol * tol * ab) return ratio2;
    // rotation diagonalising [[aa, gamma], [conj gamma, bb]]:  t = sign(h) 2g / (|h| + sqrt(h^2 + 4 g^2)), h = bb - aa
    const double ig = fast_rsq(g2);
    const double g = g2 * ig;
    const double h = bb - aa;
    const double w2 = fma(h, h, 4.0 * g2);
    const double w = w2 * fast_rsq(w2);
    double t = 2.0 * g * fast_rcp(fabs(h) + w);
    t = h >= 0.0 ? t : -t;
    t2max = fmax(t2max, t * t);                       // largest tan^2 of the sweep's rotations, see jacobi_last_sweep
    const double c = fast_rsq(fma(t, t, 1.0));
    const double s = c * t;
    // b~ = exp(-i phi) b with exp(i phi) = gamma / |gamma|;  a' = c a - s b~ ; b' = s a + c b~
    const double pr = gr * ig, pi = -gi * ig;   // exp(-i phi)
#pragma unroll
    for (int e = 0; e < JAC_MAXEL; ++e) {
        const int i = sub + GS * e;
        if (i < m) {
            const double2 bt = make_double2(pr * b[e].x - pi * b[e].y, pr * b[e].y + pi * b[e].x);
            ga[i] = make_double2(c * a[e].x - s * bt.x, c * a[e].y - s * bt.y);
            gb[i] = make_double2(s * a[e].x + c * bt.x, s * a[e].y + c * bt.y);
        }
    }
    if (accumulate)
        for (int i = sub; i < n; i += GS) {
            const double2 x = va[i], y = vb[i];
            const double2 yt = make_double2(pr * y.x - pi * y.y, pr * y.y + pi * y.x);
            va[i] = make_double2(c * x.x - s * yt.x, c * x.y - s * yt.y);
            vb[i] = make_double2(s * x.x + c * yt.x, s * x.y + c * yt.y);
        }
    return ratio2;
}

// Was this sweep the last?  mx: the largest SQUARED cosine it saw before its rotations, t2: the largest tan^2 it rotated by.
// By the quadratic convergence of cyclic Jacobi a sweep leaves about C mx^2 behind (C = 0.005 .. 0.2 measured on
// Schmidt-type spectra), so one that saw nothing above 0.1 tol has left < tol^2: no checking sweep afterwards.  That
// argument needs SMALL rotation angles.  A rotation by tan t turns the cosines its two columns have with every other
// column into each other at first order, t^2 mx squared: inside a cluster of singular values (s_i = 1 + i 1e-13: squared
// cosines of 1e-24, angles of order one) the sweep leaves what it saw, and the column norms miss the singular values by
// as much.  So the shortcut also asks for t2 mx <= tol^2; mx <= tol^2 alone means that nothing was rotated at all.
__device__ __forceinline__ bool jacobi_last_sweep(double mx, double t2, double tol) {
    const double tol2 = tol * tol;
    return mx <= tol2 || (mx <= 0.1 * tol && t2 * mx <= tol2);
}

template <int GS>
__device__ __forceinline__ int jacobi_sweeps(double2* g, double2* __restrict__ v, int m, int n, int max_sweeps,
                                             double tol, double* s_ratio, int tid, bool accumulate, double zero2) {
    const int grp = tid / GS, sub = tid % GS;
    const int ngroups = JAC_THREADS / GS;
    const int np = n + (n & 1);      // padded to even; index np-1 == n is a bye when n is odd
    int sweeps = 0;
    bool done = (n < 2);
    while (!done && sweeps < max_sweeps) {
        if (tid == 0) s_ratio[0] = s_ratio[1] = 0.0;
        __syncthreads();
        double ratio = 0.0, t2 = 0.0;
        for (int r = 0; r < np - 1; ++r) {
            for (int p = grp; p < np / 2; p += ngroups) {
                int i, j;
                if (p == 0) {
                    i = np - 1;
                    j = r;
                } else {
                    i = (r + p) % (np - 1);
                    j = (r + np - 1 - p) % (np - 1);
                }
                if (i < n && j < n) {
                    const int lo = i < j ? i : j, hi = i < j ? j : i;
                    const double rr = jacobi_pair<GS>(g + (int64_t)lo * m, g + (int64_t)hi * m, v + (int64_t)lo * n,
                                                      v + (int64_t)hi * n, m, n, sub, tol, accumulate, zero2, t2);
                    ratio = rr > ratio ? rr : ratio;
                }
            }
            __syncthreads();
        }
        // workgroup max of the non-negative ratio: doubles order like their bit patterns
        if (sub == 0 && ratio > 0.0) atomicMax((unsigned long long*)s_ratio, (unsigned long long)__double_as_longlong(ratio));
        if (sub == 0 && t2 > 0.0) atomicMax((unsigned long long*)(s_ratio + 1), (unsigned long long)__double_as_longlong(t2));
        __syncthreads();
        const double mx = s_ratio[0];  // max over the sweep of the SQUARED cosine between column pairs
        ++sweeps;
        done = jacobi_last_sweep(mx, s_ratio[1], tol);
        __syncthreads();
    }
    return done ? sweeps : -sweeps;
}

// column storage split between LDS (first nl columns) and global memory (the rest): blocks slightly larger
// than the LDS window keep most of their columns at LDS latency.  Generic (flat) pointers.
struct SplitCols {
    double2* lds;
    double2* glob;
    int nl, mp;
    __device__ __forceinline__ double2* col(int j) const {
        return j < nl ? lds + (int64_t)j * mp : glob + (int64_t)(j - nl) * mp;
    }
};

// ---- padded fast path (QR-preconditioned blocks) -----------------------------------------------------
// Columns are stored with leading dimension GS * E (zero padded), so every lane owns exactly E elements
// of each column: no per-element predication, all loads issued back to back, and the LDS / global address
// space is known at compile time (ds_* / global_* instead of flat_*).
template <int GS, int E, typename P>
__device__ __forceinline__ double jacobi_pair_pad(P ga, P gb, int sub, double tol2, double zero2, double& t2max) {
    double2 a[E], b[E];
    double aa = 0.0, bb = 0.0, gr = 0.0, gi = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        a[e] = ga[sub + GS * e];
        b[e] = gb[sub + GS * e];
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        aa = fma(a[e].x, a[e].x, fma(a[e].y, a[e].y, aa));
        bb = fma(b[e].x, b[e].x, fma(b[e].y, b[e].y, bb));
        gr = fma(a[e].x, b[e].x, fma(a[e].y, b[e].y, gr));      // conj(a) * b
        gi = fma(a[e].x, b[e].y, fma(-a[e].y, b[e].x, gi));
    }
    aa = group_sum<GS>(aa);
    bb = group_sum<GS>(bb);
    gr = group_sum<GS>(gr);
    gi = group_sum<GS>(gi);
    if (aa <= zero2 || bb <= zero2) return 0.0;
    const double g2 = gr * gr + gi * gi;
    const double ab = aa * bb;
    const double ratio2 = g2 * fast_rcp(ab);
    if (g2 == 0.0 || g2 <= tol2 * ab) return ratio2;
    const double ig = fast_rsq(g2);
    const double g = g2 * ig;
    const double h = bb - aa;
    const double w2 = fma(h, h, 4.0 * g2);
    const double w = w2 * fast_rsq(w2);
    double t = 2.0 * g * fast_rcp(fabs(h) + w);
    t = h >= 0.0 ? t : -t;
    t2max = fmax(t2max, t * t);                       // largest tan^2 of the sweep's rotations, see jacobi_last_sweep
    const double c = fast_rsq(fma(t, t, 1.0));
    const double s = c * t;
    // a' = c a - sig b ; b' = conj(sig)... written with sig = s exp(-i phi), tau = c exp(-i phi):
    //   a' = c a - sig b,  b' = s a + tau b
    const double sr = s * gr * ig, si = -s * gi * ig;
    const double tr = c * gr * ig, ti = -c * gi * ig;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        double2 na, nb;
        na.x = fma(c, a[e].x, fma(-sr, b[e].x, si * b[e].y));
        na.y = fma(c, a[e].y, fma(-sr, b[e].y, -si * b[e].x));
        nb.x = fma(s, a[e].x, fma(tr, b[e].x, -ti * b[e].y));
        nb.y = fma(s, a[e].y, fma(tr, b[e].y, ti * b[e].x));
        ga[sub + GS * e] = na;
        gb[sub + GS * e] = nb;
    }
    return ratio2;
}

template <int GS, int E, typename C>
__device__ __forceinline__ int jacobi_sweeps_pad(C cols, int n, int max_sweeps, double tol, double* s_ratio, int tid,
                                                 double zero2) {
    const int grp = tid / GS, sub = tid % GS;
    constexpr int ngroups = JAC_THREADS / GS;
    const int np = n + (n & 1);      // padded to even; index np-1 == n is a bye when n is odd
    const int md = np - 1;
    const double tol2 = tol * tol;
    int sweeps = 0;
    bool done = (n < 2);
    while (!done && sweeps < max_sweeps) {
        if (tid == 0) s_ratio[0] = s_ratio[1] = 0.0;
        __syncthreads();
        double ratio = 0.0, t2 = 0.0;
        for (int r = 0; r < md; ++r) {
            for (int p = grp; p < np / 2; p += ngroups) {
                int i, j;
                if (p == 0) {
                    i = np - 1;
                    j = r;
                } else {
                    i = r + p;
                    i = i >= md ? i - md : i;
                    j = r + md - p;
                    j = j >= md ? j - md : j;
                }
                if (i < n && j < n) {
                    const int lo = i < j ? i : j, hi = i < j ? j : i;
                    const double rr = jacobi_pair_pad<GS, E>(cols.col(lo), cols.col(hi), sub, tol2, zero2, t2);
                    ratio = rr > ratio ? rr : ratio;
                }
            }
            __syncthreads();
        }
        if (sub == 0 && ratio > 0.0) atomicMax((unsigned long long*)s_ratio, (unsigned long long)__double_as_longlong(ratio));
        if (sub == 0 && t2 > 0.0) atomicMax((unsigned long long*)(s_ratio + 1), (unsigned long long)__double_as_longlong(t2));
        __syncthreads();
        const double mx = s_ratio[0];  // max over the sweep of the SQUARED cosine between column pairs
        ++sweeps;
        done = jacobi_last_sweep(mx, s_ratio[1], tol);
        __syncthreads();
    }
    return done ? sweeps : -sweeps;
}

// all columns in one array of known address space (LDS when P is an LDS pointer after inlining)
template <typename P>
struct DenseCols {
    P base;
    int mp;
    __device__ __forceinline__ P col(int j) const { return base + j * mp; }
};

template <int GS, typename C>
__device__ __forceinline__ int jacobi_dispatch_e(C g, int E, int n, int max_sweeps, double tol, double* s_ratio, int tid,
                                                 double zero2) {
    switch (E) {
        case 1: return jacobi_sweeps_pad<GS, 1>(g, n, max_sweeps, tol, s_ratio, tid, zero2);
        case 2: return jacobi_sweeps_pad<GS, 2>(g, n, max_sweeps, tol, s_ratio, tid, zero2);
        case 3: return jacobi_sweeps_pad<GS, 3>(g, n, max_sweeps, tol, s_ratio, tid, zero2);
        case 4: return jacobi_sweeps_pad<GS, 4>(g, n, max_sweeps, tol, s_ratio, tid, zero2);
        case 5: return jacobi_sweeps_pad<GS, 5>(g, n, max_sweeps, tol, s_ratio, tid, zero2);
        case 6: return jacobi_sweeps_pad<GS, 6>(g, n, max_sweeps, tol, s_ratio, tid, zero2);
        case 7: return jacobi_sweeps_pad<GS, 7>(g, n, max_sweeps, tol, s_ratio, tid, zero2);
        default: return jacobi_sweeps_pad<GS, 8>(g, n, max_sweeps, tol, s_ratio, tid, zero2);
    }
}
