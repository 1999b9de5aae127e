// Jacobi SVD, piece of htn_svd.hip: pair visits (k_jacobi_pairs_gram), k_jacobi_check / k_jacobi_finish, the tall path
#pragma once

// ---- large blocks: block one-sided Jacobi over several CUs ---------------------------------------------
// A block whose R^H does not fit one CU's LDS is VALU-bound on that CU (all n/2 pairs of a round on 16
// waves).  Here the columns are cut into panels of w = 8; one WORKGROUP handles one PAIR of panels (a "visit"),
// the panel pairs of one tournament round run on different CUs, and rounds are separated by kernel boundaries
// (the only cross-CU synchronisation used: no in-kernel grid barriers).  Per block and outer sweep the visits leave two
// numbers, the largest squared cosine they saw and the largest tan^2 they rotated by; k_jacobi_check decides from them
// with jacobi_last_sweep (htn_svd_cols.h), the one statement of the stopping rule, and the host reads one count per sweep.
#define JAC_PANEL 8
struct JacPairItem {
    int32_t blk, ci, ni, cj, nj, pad[3];
};

// ---- panel-pair visit on the Gram matrix ---------------------------------------------------------------
// Rotating the 2 w = 16 columns of mp rows directly costs, per round, a chain of LDS reads, dots over the
// columns, a lane reduction, the rotation and the write back -- about 1.7 us, almost all of it latency (the
// first version of this path did that, 37 us per visit).  Here only ONE pass touches the long columns:
//   (1) G = P^H P  (16 x 16, Hermitian) on v_mfma_f64_16x16x4_f64, the row range split over the 4 waves;
//   (2) one cyclic sweep of two-sided Jacobi on G, 8 disjoint rotations per round, accumulating U (16 x 16);
//       one thread per matrix element, no reductions, two workgroup barriers per round;
//   (3) P <- P U on the MFMA pipe, written straight back to global.
// In exact arithmetic this is one-sided Jacobi on the columns (a one-sided rotation of two columns IS the
// two-sided rotation of their Gram matrix).  In floating point G is re-formed from the columns at every visit, so rounding in
// (2) only perturbs the rotation angles, never the orthogonality test: the stopping criterion is evaluated on
// the exact Gram of the visit.  The pivot 2 x 2 block is updated with Rutishauser's formulas
// (a' = a - t|g|, b' = b + t|g|, 0 off-diagonal), which keep the small diagonal entries of a graded Gram
// matrix relatively accurate (Demmel & Veselic 1992); the remaining entries use the plain bilinear update.
// partner of LDS column slot x in round r.  mode 0 (cross visit, 8 rounds): slot p of panel A meets slot
// 8 + (p + r) % 8 of panel B -- every A-B pair exactly once.  mode 1 (intra visit, 7 rounds): round-robin
// tournament inside each group of 8 slots.
__device__ __forceinline__ int jg_partner(int x, int r, int mode) {
    if (mode == 0) return x < 8 ? 8 + ((x + r) & 7) : ((x - r) & 7);
    const int g = x & 8, k = x & 7;
    if (k == 7) return g + r;
    if (k == r) return g + 7;
    int y = 2 * r - k + 7;
    y = y >= 14 ? y - 14 : (y >= 7 ? y - 7 : y);
    return g + y;
}

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ double2 cmulc(double2 ac, double2 b) {      // conj(ac) * b
    return make_double2(fma(ac.x, b.x, ac.y * b.y), fma(ac.x, b.y, -ac.y * b.x));
}


// rotation that annihilates the (lo, hi) entry g of a 2 x 2 Hermitian pivot [[aa, g], [conj g, bb]]: c = cos, cq = cos *
// tan / |g|, dq = tan * |g|, t2 = tan^2; identity (returns false, t2 = 0) for dead slots, numerically zero columns and pairs
// already orthogonal to tol.  No branches: cos from cos(2 theta) = |h| / w runs in parallel with the reciprocal that gives q.
__device__ __forceinline__ bool jg_rotation(double aa, double bb, double2 g, bool live, double z2, double tol2,
                                            double& c, double& cq, double& dq, double& t2) {
    const double g2 = fma(g.x, g.x, g.y * g.y);
    const bool on = live && aa > z2 && bb > z2 && g2 > 0.0 && g2 > tol2 * aa * bb;
    const double h = on ? bb - aa : 0.0, g2s = on ? g2 : 1.0, ah = fabs(h);
    const double w2 = fma(h, h, 4.0 * g2s);
    const double iw = fast_rsq(w2);
    double q = 2.0 * fast_rcp(fma(w2, iw, ah));
    q = h >= 0.0 ? q : -q;
    const double c2 = fma(0.5 * ah, iw, 0.5);
    const double cc = c2 * fast_rsq(c2);
    c = on ? cc : 1.0;
    cq = on ? cc * q : 0.0;
    dq = on ? q * g2s : 0.0;
    t2 = on ? q * q * g2s : 0.0;
    return on;
}

#define JG_LD 17
#define JG_PS 9            // doubles per lane of the Gram partials (8 used): odd stride, no 16-way bank conflict
#define JG_GU_ELEMS (4 * 64 * JG_PS / 2)        // complex128 elements of the G/U region (>= 4 * 16 * JG_LD; the partials alias it)
// slot q (0..15) of a visit (0..7: first panel, 8..15: second): does it hold a column, and which one (-1 for dead slots)
__device__ __forceinline__ bool jg_slot_live(const JacPairItem& it, int q) { return q < 8 ? q < it.ni : q - 8 < it.nj; }
__device__ __forceinline__ int jg_slot_col(const JacPairItem& it, int q) {
    return q < 8 ? (q < it.ni ? it.ci + q : -1) : (q - 8 < it.nj ? it.cj + (q - 8) : -1);
}

// ---- the 16 x 16 Gram-visit core, shared by k_jacobi_pairs_gram (4 waves) and k_jacobi_tall_visit (TALL_WAVES) --------------
// Every wave has left its MFMA accumulators g1 + g2 (registers 0..3) and mm (4..7) at part + (wave * 64 + lane) * JG_PS.
// Element (ei, ej) of the Gram matrix, the wave partials summed in a fixed order: deterministic.
template <int NW>
__device__ __forceinline__ double2 jg_gram_element(const double* part, int ei, int ej) {
    // accumulator element (row = l4 + 4 reg, col = l15): G[i][j] sits in lane j + 16 (i & 3), reg i >> 2
    const double* pa = part + (ej + 16 * (ei & 3)) * JG_PS + (ei >> 2);
    const double* pb = part + (ei + 16 * (ej & 3)) * JG_PS + 4 + (ej >> 2);
    double gr = 0.0, mij = 0.0, mji = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        gr += pa[w * 64 * JG_PS];
        mij += pa[w * 64 * JG_PS + 4];
        mji += pb[w * 64 * JG_PS];
    }
    return make_double2(gr, mij - mji);
}

// GU = G[2][16][17], U[2][16][17]: G <- the Gram matrix, U <- identity.  MIRROR: threads 256.. mirror 0..255 (same element,
// same arithmetic) and never write G / U.
template <bool MIRROR>
__device__ __forceinline__ void jg_gram_store(double2* GU, double2 g, int ei, int ej) {
    if (!MIRROR || threadIdx.x < 256) {
        GU[ei * JG_LD + ej] = g;
        GU[2 * 16 * JG_LD + ei * JG_LD + ej] = make_double2(ei == ej ? 1.0 : 0.0, 0.0);
    }
}

// convergence measure of a visit: max squared cosine over its column pairs (exact Gram), as bits, through s_rbits (zeroed
// before the last barrier).  True: nothing to rotate in this visit (uniform), the measure has been handed to ratio_bits
// (the block's first word: [2 blk] squared cosine, [2 blk + 1] tan^2, see jg_visit_report).
__device__ __forceinline__ bool jg_visit_converged(const double2* GU, const JacPairItem& it, int mode, int ei, int ej, double z2,
                                                   double tol2, unsigned long long* s_rbits,
                                                   unsigned long long* ratio_bits, unsigned long long& first_bits) {
    {
        double ratio = 0.0;
        const bool vi = jg_slot_live(it, ei), vj = jg_slot_live(it, ej);
        if (vi && vj && ei < ej && (mode ? (ei >> 3) == (ej >> 3) : (ei < 8 && ej >= 8))) {
            const double dii = GU[ei * JG_LD + ei].x, djj = GU[ej * JG_LD + ej].x;
            const double2 g = GU[ei * JG_LD + ej];
            if (dii > z2 && djj > z2) ratio = fma(g.x, g.x, g.y * g.y) * fast_rcp(dii * djj);
        }
        const unsigned long long key = wave_max_u64((unsigned long long)__double_as_longlong(ratio));
        if ((threadIdx.x & 63) == 0 && key) atomicMax(s_rbits, key);
    }
    __syncthreads();
    first_bits = *s_rbits;
    if (__longlong_as_double((long long)first_bits) > tol2) return false;
    if (threadIdx.x == 0 && first_bits) atomicMax(ratio_bits, first_bits);
    return true;
}

// what a visit that rotated leaves for k_jacobi_check: the squared cosine it saw first and the largest tan^2 it rotated by,
// integer maxima on the bit patterns (non-negative doubles order like their bits): the order of the visits does not matter
__device__ __forceinline__ void jg_visit_report(unsigned long long* ratio_bits, int blk, unsigned long long first_bits, double t2max) {
    const unsigned long long key = wave_max_u64((unsigned long long)__double_as_longlong(t2max));
    if ((threadIdx.x & 63) == 0 && threadIdx.x < 256 && key) atomicMax(&ratio_bits[2 * blk + 1], key);
    if (threadIdx.x == 0) atomicMax(&ratio_bits[2 * blk], first_bits);
}

// `inner` cyclic sweeps of two-sided Jacobi on G, U <- U J; returns the buffer (0 / 1) that holds the final G and U.
// t2max <- the largest tan^2 among the rotations of this thread's row pairs (every pair of a round is some row's).
// One thread per element (i, j).  It needs the rotation of i's pair (row operation) and of j's pair (column
// operation) and computes both itself from the pivot entries -- 256-fold redundant arithmetic, but the
// round is then a single chain [12 LDS reads -> two interleaved rotations -> update -> write] with ONE
// barrier (G and U are double buffered), instead of [8 lanes rotate] barrier [256 lanes apply] barrier.
template <bool MIRROR>
__device__ __forceinline__ int jg_rounds(double2* GU, const JacPairItem& it, int mode, int inner, int ei, int ej, double z2,
                                         double tol2, double& t2max) {
    const int nrounds = mode ? 7 : 8;
    unsigned livemask = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) livemask |= (unsigned)jg_slot_live(it, q) << q;
    int cur = 0;
    for (int sw = 0; sw < inner; ++sw) {
        for (int r = 0; r < nrounds; ++r) {
            const double2* Gc = GU + cur * 16 * JG_LD;
            const double2* Uc = GU + (2 + cur) * 16 * JG_LD;
            double2* Gn = GU + (cur ^ 1) * 16 * JG_LD;
            double2* Un = GU + (2 + (cur ^ 1)) * 16 * JG_LD;
            const int ib = jg_partner(ei, r, mode), jb = jg_partner(ej, r, mode);
            const int ilo = ei < ib ? ei : ib, ihi = ei < ib ? ib : ei;
            const int jlo = ej < jb ? ej : jb, jhi = ej < jb ? jb : ej;
            const double iaa = Gc[ilo * JG_LD + ilo].x, ibb = Gc[ihi * JG_LD + ihi].x;
            const double2 ig = Gc[ilo * JG_LD + ihi];                  // conj(a_lo) . a_hi
            const double jaa = Gc[jlo * JG_LD + jlo].x, jbb = Gc[jhi * JG_LD + jhi].x;
            const double2 jg = Gc[jlo * JG_LD + jhi];
            const double2 gij = Gc[ei * JG_LD + ej], gijb = Gc[ei * JG_LD + jb];
            const double2 gibj = Gc[ib * JG_LD + ej], gibjb = Gc[ib * JG_LD + jb];
            const double2 uij = Uc[ei * JG_LD + ej], uijb = Uc[ei * JG_LD + jb];
            // J = [[c, c q g], [-c q conj(g), c]] on (lo, hi), q = tan / |g|: real diagonal, no phase division.
            // Both rotations are computed branch-free (jg_rotation) so that their two dependent chains interleave.
            double ci, cqi, dqi, cj, cqj, dqj, t2i, t2j;
            const bool oni = jg_rotation(iaa, ibb, ig, ((livemask >> ilo) & (livemask >> ihi) & 1u) != 0, z2, tol2, ci, cqi, dqi, t2i);
            jg_rotation(jaa, jbb, jg, ((livemask >> jlo) & (livemask >> jhi) & 1u) != 0, z2, tol2, cj, cqj, dqj, t2j);
            t2max = fmax(t2max, t2i);
            // column j of J: J[j][j] = c, J[jb][j] = -cq conj(g) if j is the lower index, +cq g if the upper
            const double2 jpj = ej == jlo ? make_double2(-cqj * jg.x, cqj * jg.y) : make_double2(cqj * jg.x, cqj * jg.y);
            const double2 ipi = ei == ilo ? make_double2(-cqi * ig.x, cqi * ig.y) : make_double2(cqi * ig.x, cqi * ig.y);
            double2 t2 = cmul(gijb, jpj);
            const double2 Tij = make_double2(fma(cj, gij.x, t2.x), fma(cj, gij.y, t2.y));
            t2 = cmul(gibjb, jpj);
            const double2 Tibj = make_double2(fma(cj, gibj.x, t2.x), fma(cj, gibj.y, t2.y));
            t2 = cmulc(ipi, Tibj);
            double2 gn = make_double2(fma(ci, Tij.x, t2.x), fma(ci, Tij.y, t2.y));
            {               // pivot block by Rutishauser's formulas: a' = a - t|g|, b' = b + t|g|, off-diagonal 0
                const double dg = ei == ilo ? iaa - dqi : ibb + dqi;
                const bool pd = oni && ej == ei, po = oni && ej == ib;
                gn.x = pd ? dg : (po ? 0.0 : gn.x);
                gn.y = (pd || po) ? 0.0 : gn.y;
            }
            t2 = cmul(uijb, jpj);
            if (!MIRROR || threadIdx.x < 256) {
                Gn[ei * JG_LD + ej] = gn;
                Un[ei * JG_LD + ej] = make_double2(fma(cj, uij.x, t2.x), fma(cj, uij.y, t2.y));
            }
            __syncthreads();
            cur ^= 1;
        }
    }
    return cur;
}

// A operand of the transposed product D[b][i] = sum_a U[a][b] P[i][a] (step (3) of k_jacobi_pairs_gram, tall_apply):
// U[4 kk + l4][l15] as real part, imaginary part and its negative
__device__ __forceinline__ void jg_load_u(const double2* Uc, int l15, int l4, double (&ur)[4], double (&ui)[4], double (&nui)[4]) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const double2 u = Uc[(4 * kk + l4) * JG_LD + l15];
        ur[kk] = u.x;
        ui[kk] = u.y;
        nui[kk] = -u.y;
    }
}

__global__ __launch_bounds__(256) void k_jacobi_pairs_gram(double2* __restrict__ Vj,
                                                           const htn_svd_block* __restrict__ desc,
                                                           const int* __restrict__ large_ids,
                                                           const JacPairItem* __restrict__ items,
                                                           const double* __restrict__ zero2,
                                                           unsigned long long* __restrict__ ratio_bits,
                                                           const int* __restrict__ done, double tol, int inner) {
    extern __shared__ double2 g_lds[];
    __shared__ unsigned long long s_rbits;
    const JacPairItem it = items[blockIdx.x];
    if (done[it.blk]) return;
    const htn_svd_block D = desc[large_ids[it.blk]];
    const int m = D.m, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int gsx = m <= 16 * JAC_MAXEL ? 16 : (m <= 32 * JAC_MAXEL ? 32 : 64);
    const int mp = gsx * ((m + gsx - 1) / gsx);
    const int ldp = mp + 1;
    double2* __restrict__ X = Vj + D.v_off;
    const int mode = it.pad[0];
    double2* P = g_lds;                              // [16][ldp]
    double2* GU = g_lds + 16 * ldp;                  // G[2][16][17], U[2][16][17]; the Gram partials alias it
    const double z2 = zero2[it.blk];
    const double tol2 = tol * tol;
    if (tid == 0) s_rbits = 0ull;
    // ---- (0) columns -> LDS: 16 lanes per column, 256 contiguous bytes per request ----
    {
        const int c = tid >> 4, r = tid & 15;
        const int col = jg_slot_col(it, c);
        const bool live = col >= 0;
        const double2* __restrict__ src = X + (int64_t)(live ? col : 0) * mp;
        double2* dst = P + c * ldp;
        const int ne = mp >> 4;
        for (int e0 = 0; e0 < ne; e0 += 16) {          // 16 requests in flight per lane: one round trip up to 256 rows
            double2 v[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = r + 16 * (e0 + e);
                v[e] = (live && e0 + e < ne) ? src[row] : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (e0 + e < ne) dst[r + 16 * (e0 + e)] = v[e];
        }
    }
    __syncthreads();
    // ---- (1) Gram: lane (l15, l4) feeds P[4 ks + l4][l15] as A and as B operand ----
    {
        d4 g1 = {0.0, 0.0, 0.0, 0.0}, g2 = {0.0, 0.0, 0.0, 0.0}, mm = {0.0, 0.0, 0.0, 0.0};
        const double2* pc = P + l15 * ldp + l4;
        const int nit = mp >> 4;                     // k-steps of this wave: ks = wave + 4 it
        // operands of four steps are fetched together, the next four are in flight during the 12 MFMAs
        double2 nx[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) nx[u] = u < nit ? pc[4 * (wave + 4 * u)] : make_double2(0.0, 0.0);
        for (int it0 = 0; it0 < nit; it0 += 4) {
            double2 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = nx[u];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (it0 + 4 + u < nit) nx[u] = pc[4 * (wave + 4 * (it0 + 4 + u))];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (it0 + u < nit) {                 // wave-uniform
                    g1 = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u].x, v[u].x, g1, 0, 0, 0);
                    g2 = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u].y, v[u].y, g2, 0, 0, 0);
                    mm = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u].x, v[u].y, mm, 0, 0, 0);      // M[a][b] = sum re_a im_b
                }
            }
        }
        double* part = (double*)GU + (wave * 64 + lane) * JG_PS;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            part[r] = g1[r] + g2[r];
            part[4 + r] = mm[r];
        }
    }
    __syncthreads();
    const int ei = tid >> 4, ej = tid & 15;
    const double2 gij = jg_gram_element<4>((const double*)GU, ei, ej);
    __syncthreads();                                // partials consumed; the region becomes G / U
    jg_gram_store<false>(GU, gij, ei, ej);
    __syncthreads();
    unsigned long long first_bits;
    if (jg_visit_converged(GU, it, mode, ei, ej, z2, tol2, &s_rbits, &ratio_bits[2 * it.blk], first_bits)) return;
    // ---- (2) two-sided Jacobi on G, U <- U J ----
    double t2max = 0.0;
    const int cur = jg_rounds<false>(GU, it, mode, inner, ei, ej, z2, tol2, t2max);
    // ---- (3) P <- P U, transposed product so that a lane's 16 neighbours write 256 contiguous bytes:
    //      D[b][i] = sum_a U[a][b] P[i][a]:  A operand U[4 kk + l4][l15], B operand P[i0 + l15][4 kk + l4] ----
    {
        const double2* Uc = GU + (2 + cur) * 16 * JG_LD;
        double ur[4], ui[4], nui[4];
        jg_load_u(Uc, l15, l4, ur, ui, nui);
        int colg[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) colg[r] = jg_slot_col(it, l4 + 4 * r);
        const int nrt = mp >> 4;
        const double2* pb = P + l4 * ldp + l15;
        double2 pn[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) pn[kk] = wave < nrt ? pb[4 * kk * ldp + wave * 16] : make_double2(0.0, 0.0);
        for (int rt = wave; rt < nrt; rt += 4) {
            const int i0 = rt * 16;
            double2 p[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) p[kk] = pn[kk];
            if (rt + 4 < nrt) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) pn[kk] = pb[4 * kk * ldp + i0 + 64];
            }
            d4 ar = {0.0, 0.0, 0.0, 0.0}, ai = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                ar = __builtin_amdgcn_mfma_f64_16x16x4f64(ur[kk], p[kk].x, ar, 0, 0, 0);
                ai = __builtin_amdgcn_mfma_f64_16x16x4f64(ur[kk], p[kk].y, ai, 0, 0, 0);
                ar = __builtin_amdgcn_mfma_f64_16x16x4f64(nui[kk], p[kk].y, ar, 0, 0, 0);
                ai = __builtin_amdgcn_mfma_f64_16x16x4f64(ui[kk], p[kk].x, ai, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (colg[r] >= 0) X[(int64_t)colg[r] * mp + i0 + l15] = make_double2(ar[r], ai[r]);
        }
    }
    jg_visit_report(ratio_bits, it.blk, first_bits, t2max);
}

// after every outer sweep: convergence bookkeeping of the large blocks ON THE DEVICE (one thread per block), so
// the host never has to answer before the next sweep can start.  active_out is host-pinned: the host reads it
// one sweep late (the next sweep is already enqueued; if everything had converged its visits return at once).
// ratio_bits: two words per block, the sweep's largest squared cosine and largest tan^2 (jg_visit_report); both are zeroed
// here for the next sweep.
__global__ void k_jacobi_check(unsigned long long* __restrict__ ratio_bits, int* __restrict__ done,
                               int* __restrict__ sweeps, int nl, double tol, int* __restrict__ active_out) {
    __shared__ int s_active;
    if (threadIdx.x == 0) s_active = 0;
    __syncthreads();
    for (int li = threadIdx.x; li < nl; li += blockDim.x) {
        if (!done[li]) {
            const double mx = __longlong_as_double((long long)ratio_bits[2 * li]);
            const double t2 = __longlong_as_double((long long)ratio_bits[2 * li + 1]);
            sweeps[li] += 1;
            if (jacobi_last_sweep(mx, t2, tol)) done[li] = 1;
            else atomicAdd(&s_active, 1);
        }
        ratio_bits[2 * li] = ratio_bits[2 * li + 1] = 0ull;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *active_out = s_active;
        __threadfence_system();
    }
}

__global__ __launch_bounds__(JAC_THREADS) void k_jacobi_finish(double2* __restrict__ G, const double2* __restrict__ Vj,
                                                               double* __restrict__ S,
                                                               const htn_svd_block* __restrict__ desc,
                                                               const int* __restrict__ large_ids,
                                                               const int* __restrict__ perm,
                                                               const int* __restrict__ sweeps,
                                                               const int* __restrict__ done, int* __restrict__ info) {
    const int b = large_ids[blockIdx.x];
    const htn_svd_block D = desc[b];
    const int m = D.m, n = D.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gsx = m <= 16 * JAC_MAXEL ? 16 : (m <= 32 * JAC_MAXEL ? 32 : 64);
    const int mp = gsx * ((m + gsx - 1) / gsx);
    const double2* __restrict__ X = Vj + D.v_off;
    double2* __restrict__ g = G + D.g_off;
    const int* __restrict__ pc = perm + blockIdx.x * 64 * JAC_MAXEL;
    for (int j = wave; j < n; j += JAC_THREADS / 64) {
        double sn = 0.0;
        for (int i = lane; i < m; i += 64) {
            const double2 x = X[(int64_t)j * mp + i];
            sn += x.x * x.x + x.y * x.y;
            g[(int64_t)j * m + pc[i]] = x;          // undo the pivoting: row k of X is row perm[k] of the result
        }
        sn = wave_sum(sn);
        if (lane == 0) S[D.s_off + j] = sqrt(sn);
    }
    if (tid == 0) info[b] = done[blockIdx.x] ? sweeps[blockIdx.x] : -sweeps[blockIdx.x];
}

// ---- tall blocks: pair-visit block Jacobi with the columns streamed from global memory ------------------------------
// A plain (non-QRCP) block whose columns are longer than 512 rows fits neither the registers of the one-workgroup kernel
// nor the LDS panel of k_jacobi_pairs_gram.  It runs the same tournament as the pair-visit path (one launch per round,
// one workgroup per panel pair, the launch boundary the only ordering between workgroups, no workgroup ever waits for
// another), but a visit never holds its 16 columns: (a) the 16 x 16 Gram is accumulated on v_mfma_f64_16x16x4_f64 over
// row chunks read straight from global memory, every wave a contiguous row range, the wave partials summed in a fixed
// order; (b) the inner two-sided Jacobi and the convergence measure are those of k_jacobi_pairs_gram (the jg_* functions
// above); (c) U is applied chunk by chunk to the columns of X and, when accumulating,
// to the same columns of J (n x n, ld n).  No QR preconditioning: expect more outer sweeps than the QRCP path.
#define TALL_THREADS 512
#define TALL_WAVES (TALL_THREADS / 64)
#define TALL_DEPTH 8              // loads in flight per lane: k-steps of the Gram, 16-row tiles (x 4 columns) of the apply
#define TALL_PARTS 32             // workgroups per block of the |X|_F^2 / identity-J pass

// A[:, cols] <- A[:, cols] U for a rows x n matrix with leading dimension ld (U: 16 x 16 in LDS, ld JG_LD).
// Same transposed MFMA product as step (3) of k_jacobi_pairs_gram, B operand read from global memory: a wave owns
// 16-row tiles rt = wave + TALL_WAVES t, so no two waves touch the same rows.
__device__ __forceinline__ void tall_apply(double2* A, int64_t ld, int rows, const double2* Uc, const JacPairItem& it,
                                           int wave, int l15, int l4) {
    double ur[4], ui[4], nui[4];
    jg_load_u(Uc, l15, l4, ur, ui, nui);
    int colk[4], colg[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        colk[kk] = jg_slot_col(it, 4 * kk + l4);     // B operand: column slot 4 kk + l4
        colg[kk] = jg_slot_col(it, l4 + 4 * kk);     // output row r of the accumulator: column slot l4 + 4 r
    }
    const int nrt = (rows + 15) >> 4;
    for (int rt0 = wave; rt0 < nrt; rt0 += TALL_WAVES * (TALL_DEPTH / 4)) {
        double2 p[TALL_DEPTH / 4][4];
#pragma unroll
        for (int t = 0; t < TALL_DEPTH / 4; ++t) {
            const int row = (rt0 + t * TALL_WAVES) * 16 + l15;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                p[t][kk] = (colk[kk] >= 0 && row < rows) ? A[(int64_t)colk[kk] * ld + row] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int t = 0; t < TALL_DEPTH / 4; ++t) {
            const int row = (rt0 + t * TALL_WAVES) * 16 + l15;
            d4 ar = {0.0, 0.0, 0.0, 0.0}, ai = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                ar = __builtin_amdgcn_mfma_f64_16x16x4f64(ur[kk], p[t][kk].x, ar, 0, 0, 0);
                ai = __builtin_amdgcn_mfma_f64_16x16x4f64(ur[kk], p[t][kk].y, ai, 0, 0, 0);
                ar = __builtin_amdgcn_mfma_f64_16x16x4f64(nui[kk], p[t][kk].y, ar, 0, 0, 0);
                ai = __builtin_amdgcn_mfma_f64_16x16x4f64(ui[kk], p[t][kk].x, ai, 0, 0, 0);
            }
            if (row < rows) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (colg[r] >= 0) A[(int64_t)colg[r] * ld + row] = make_double2(ar[r], ai[r]);
            }
        }
    }
}

__global__ __launch_bounds__(TALL_THREADS) void k_jacobi_tall_visit(double2* __restrict__ G, double2* __restrict__ Vj,
                                                                    const htn_svd_block* __restrict__ desc,
                                                                    const int* __restrict__ tall_ids,
                                                                    const JacPairItem* __restrict__ items,
                                                                    const double* __restrict__ zero2,
                                                                    unsigned long long* __restrict__ ratio_bits,
                                                                    const int* __restrict__ done, double tol) {
    __shared__ double s_part[TALL_WAVES * 64 * JG_PS];      // Gram partials of every wave
    __shared__ double2 GU[4 * 16 * JG_LD];                   // G[2][16][17], U[2][16][17]
    __shared__ unsigned long long s_rbits;
    const JacPairItem it = items[blockIdx.x];
    if (done[it.blk]) return;
    const htn_svd_block D = desc[tall_ids[it.blk]];
    const int m = D.m, n = D.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    double2* X = G + D.g_off;
    const int mode = it.pad[0];
    const double z2 = zero2[it.blk];
    const double tol2 = tol * tol;
    if (tid == 0) s_rbits = 0ull;
    // ---- (a) Gram: lane (l15, l4) feeds row 4 ks + l4 of column slot l15 as A and as B operand; wave w sums the
    //      k-steps [w per, (w + 1) per) in ascending order ----
    {
        d4 g1 = {0.0, 0.0, 0.0, 0.0}, g2 = {0.0, 0.0, 0.0, 0.0}, mm = {0.0, 0.0, 0.0, 0.0};
        const int col = jg_slot_col(it, l15);
        const double2* src = X + (int64_t)(col >= 0 ? col : 0) * m;
        const int nks = (m + 3) >> 2, per = (nks + TALL_WAVES - 1) / TALL_WAVES;
        const int ks0 = wave * per, ks1 = min(nks, ks0 + per);
        for (int ks = ks0; ks < ks1; ks += TALL_DEPTH) {
            double2 v[TALL_DEPTH];
#pragma unroll
            for (int u = 0; u < TALL_DEPTH; ++u) {
                const int row = 4 * (ks + u) + l4;
                v[u] = (col >= 0 && ks + u < ks1 && row < m) ? src[row] : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int u = 0; u < TALL_DEPTH; ++u) {
                if (ks + u < ks1) {                  // wave-uniform
                    g1 = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u].x, v[u].x, g1, 0, 0, 0);
                    g2 = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u].y, v[u].y, g2, 0, 0, 0);
                    mm = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u].x, v[u].y, mm, 0, 0, 0);      // M[a][b] = sum re_a im_b
                }
            }
        }
        double* part = s_part + (wave * 64 + lane) * JG_PS;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            part[r] = g1[r] + g2[r];
            part[4 + r] = mm[r];
        }
    }
    __syncthreads();
    // threads 256.. mirror 0..255 (same element, same arithmetic) and never write G / U
    const int ei = (tid >> 4) & 15, ej = tid & 15;
    jg_gram_store<true>(GU, jg_gram_element<TALL_WAVES>(s_part, ei, ej), ei, ej);
    __syncthreads();
    unsigned long long first_bits;
    if (jg_visit_converged(GU, it, mode, ei, ej, z2, tol2, &s_rbits, &ratio_bits[2 * it.blk], first_bits)) return;
    // ---- (b) two-sided Jacobi on G, U <- U J: one cyclic sweep ----
    double t2max = 0.0;
    const int cur = jg_rounds<true>(GU, it, mode, 1, ei, ej, z2, tol2, t2max);
    // ---- (c) X[:, pair] <- X[:, pair] U, and J[:, pair] <- J[:, pair] U when accumulating ----
    const double2* Uf = GU + (2 + cur) * 16 * JG_LD;
    tall_apply(X, m, m, Uf, it, wave, l15, l4);
    if (D.flags & HTN_SVD_ACCUMULATE) tall_apply(Vj + D.v_off, n, n, Uf, it, wave, l15, l4);
    jg_visit_report(ratio_bits, it.blk, first_bits, t2max);
}

// |X|_F^2 of every tall block in TALL_PARTS column stripes (fixed-order sums: bit-reproducible), J = identity when
// accumulating; grid (n_tall, TALL_PARTS), 256 threads
__global__ __launch_bounds__(256) void k_jacobi_tall_init(double2* __restrict__ G, double2* __restrict__ Vj,
                                                          const htn_svd_block* __restrict__ desc,
                                                          const int* __restrict__ tall_ids, double* __restrict__ part) {
    __shared__ double s_w[4];
    const htn_svd_block D = desc[tall_ids[blockIdx.x]];
    const int m = D.m, n = D.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double2* __restrict__ X = G + D.g_off;
    double f = 0.0;
    for (int j = blockIdx.y; j < n; j += TALL_PARTS)
        for (int i = tid; i < m; i += 256) {
            const double2 x = X[(int64_t)j * m + i];
            f += x.x * x.x + x.y * x.y;
        }
    if (D.flags & HTN_SVD_ACCUMULATE) {
        double2* __restrict__ J = Vj + D.v_off;
        for (int j = blockIdx.y; j < n; j += TALL_PARTS)
            for (int i = tid; i < n; i += 256) J[(int64_t)j * n + i] = make_double2(i == j ? 1.0 : 0.0, 0.0);
    }
    f = wave_sum(f);
    if (lane == 0) s_w[wave] = f;
    __syncthreads();
    if (tid == 0) part[blockIdx.x * TALL_PARTS + blockIdx.y] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// "numerically zero" threshold of every tall block: 1e-30 |X|_F^2, as in k_jacobi_svd
__global__ void k_jacobi_tall_zero(const double* __restrict__ part, double* __restrict__ zero2, int nt) {
    for (int li = threadIdx.x; li < nt; li += blockDim.x) {
        double t = 0.0;
        for (int q = 0; q < TALL_PARTS; ++q) t += part[li * TALL_PARTS + q];
        zero2[li] = 1e-30 * t;
    }
}

// S = column norms, info = sweep count (< 0: not converged); grid (ceil(max n / 4), n_tall), one column per wave
__global__ __launch_bounds__(256) void k_jacobi_tall_finish(const double2* __restrict__ G, double* __restrict__ S,
                                                            const htn_svd_block* __restrict__ desc,
                                                            const int* __restrict__ tall_ids,
                                                            const int* __restrict__ sweeps, const int* __restrict__ done,
                                                            int* __restrict__ info) {
    const int b = tall_ids[blockIdx.y];
    const htn_svd_block D = desc[b];
    const int m = D.m, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x * 4 + wave;
    if (j < D.n) {
        const double2* __restrict__ x = G + D.g_off + (int64_t)j * m;
        double sn = 0.0;
        for (int i = lane; i < m; i += 64) sn += x[i].x * x[i].x + x[i].y * x[i].y;
        sn = wave_sum(sn);
        if (lane == 0) S[D.s_off + j] = sqrt(sn);
    }
    if (blockIdx.x == 0 && tid == 0) info[b] = done[blockIdx.y] ? sweeps[blockIdx.y] : -sweeps[blockIdx.y];
}
