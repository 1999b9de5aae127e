// Batched null-space projection (htn_block_nullproj_z): per item R <- (1 - Q Q^H) R (side 0, Q m x k with orthonormal
// columns) or R <- R (1 - Q^H Q) (side 1, Q k x n with orthonormal rows), applied twice; per result the squared norm of the
// coefficients the first pass removed and the squared norm of what is left.  The projected residuals of the two-site energy
// variance (htn_mps::variance in htn_variance.cpp).
//
// Side 1 is side 0 of the conjugate-transposed views (R^H <- (1 - Q^H Q) R^H), so one body serves both: it works on the LOGICAL
// matrices R (M x N) and Q (M x K) and reaches memory through accessors that conjugate and swap the indices for side 1.
// Work unit = (item, 16 logical columns of R) = one workgroup of four waves; units touch disjoint columns, no unit waits for
// another.  Q is taken in rounds of 64 logical columns:
//   (1) every wave forms, over its quarter of the M rows, its share of W = Q_round^H R_chunk (64 x 16): four 16 x 16 pieces on
//       v_mfma_f64_16x16x4_f64 (the pattern of k_qr_blocks' projection, htn_qr.hip), each lane feeding two consecutive rows per
//       step; the four shares go to LDS and are added in wave order, |W|^2 is collected there in the first pass;
//   (2) every wave updates 16-row tiles of the chunk, R_tile -= Q_tile W, with the same instruction, W read from LDS.
// Rounds follow one another on the updated chunk (block Gram-Schmidt); Q and the chunk are read through the L2, the chunk is
// written in place.  The barrier after (2) makes the chunk visible to the waves of the workgroup (one CU, one L1).  The norm of
// the chunk is taken in a last pass over it.  Every sum has a fixed order (MFMA accumulation in loop order, wave shares in wave
// order, wave_sum's tree, the four wave sums in wave order), stage 2 adds units and items in order: repeated calls give the same bits.
#include <algorithm>

#include "htn_common.h"

namespace {

constexpr int NP_THREADS = 256;
constexpr int NP_NW = NP_THREADS / 64;       // waves
constexpr int NP_CH = 4;                      // 16-column pieces of Q per round
constexpr int NP_KR = 16 * NP_CH;             // logical columns of Q per round
constexpr int NP_WELEMS = NP_KR * 16;         // one share of W
static_assert(sizeof(htn_nullproj_item) == 64, "htn_nullproj_item is a 64-byte record");
static_assert(NP_NW == 4, "the wave shares are added as (0 + 1) + (2 + 3)");

__device__ __forceinline__ int np_units(int m, int n, int side) { return HTN_NULLPROJ_UNITS(m, n, side); }

template <bool TR, class P>
struct NpMat {           // logical matrix: the view itself (TR = false) or its conjugate transpose
    P* a;
    int64_t ld;
    __device__ __forceinline__ double2 ld_(int i, int j) const {
        if (!TR) return a[(int64_t)j * ld + i];
        double2 x = a[(int64_t)i * ld + j];
        x.y = -x.y;
        return x;
    }
};
template <bool TR>
__device__ __forceinline__ void np_st(const NpMat<TR, double2>& v, int i, int j, double2 x) {
    if (!TR) v.a[(int64_t)j * v.ld + i] = x;
    else v.a[(int64_t)i * v.ld + j] = make_double2(x.x, -x.y);
}

// one unit: logical R (M x N), Q (M x K), columns c0 .. c0 + nc of R.  -> this thread's shares of |W|^2 (first pass) and |R|^2
template <bool TR>
__device__ __forceinline__ void np_unit(const NpMat<TR, double2> R, const NpMat<TR, const double2> Q, int M, int K, int c0, int nc,
                                        double2* Wp, double& w2, double& r2) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int mq = (M + 8 * NP_NW - 1) / (8 * NP_NW) * 8;            // rows of one wave's quarter, a multiple of the 8-row step
    const int r0 = wave * mq, r1 = min(M, r0 + mq);
    const bool pcol = l15 < nc;
    for (int pass = 0; pass < 2; ++pass)
        for (int g0 = 0; g0 < K; g0 += NP_KR) {
            const int kr = min(NP_KR, K - g0), nch = (kr + 15) >> 4;
            // ---- (1) this wave's share of W = Q_round^H R_chunk over the rows r0 .. r1 ----
            d4 cr[NP_CH], ci[NP_CH];
#pragma unroll
            for (int c = 0; c < NP_CH; ++c) cr[c] = ci[c] = d4{0.0, 0.0, 0.0, 0.0};
            for (int base = r0; base < r1; base += 8) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int i = base + 2 * l4 + e;
                    const bool row = i < r1;
                    const double2 b = row && pcol ? R.ld_(i, c0 + l15) : make_double2(0.0, 0.0);
#pragma unroll
                    for (int c = 0; c < NP_CH; ++c)
                        if (c < nch) {                                // (wave-uniform)
                            const int t = 16 * c + l15;
                            const double2 q = row && t < kr ? Q.ld_(i, g0 + t) : make_double2(0.0, 0.0);
                            cr[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(q.x, b.x, cr[c], 0, 0, 0);
                            ci[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(q.x, b.y, ci[c], 0, 0, 0);
                            cr[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(q.y, b.y, cr[c], 0, 0, 0);
                            ci[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(-q.y, b.x, ci[c], 0, 0, 0);
                        }
                }
            }
#pragma unroll
            for (int c = 0; c < NP_CH; ++c)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    Wp[wave * NP_WELEMS + (16 * c + l4 + 4 * reg) * 16 + l15] = make_double2(cr[c][reg], ci[c][reg]);
            __syncthreads();
            // the shares in wave order; W stays in share 0 (every element is read and written by one thread)
            for (int e = tid; e < NP_WELEMS; e += NP_THREADS) {
                const double2 a0 = Wp[e], a1 = Wp[NP_WELEMS + e], a2 = Wp[2 * NP_WELEMS + e], a3 = Wp[3 * NP_WELEMS + e];
                const double2 s = make_double2((a0.x + a1.x) + (a2.x + a3.x), (a0.y + a1.y) + (a2.y + a3.y));
                Wp[e] = s;
                if (pass == 0) w2 += s.x * s.x + s.y * s.y;
            }
            __syncthreads();
            // ---- (2) R_chunk -= Q_round W, 16-row tiles dealt to the waves ----
            const int kq = nch << 2;                                  // K steps of 4 over the pieces that were formed
            for (int rt = wave; rt < ((M + 15) >> 4); rt += NP_NW) {
                const int i0 = 16 * rt, ia = i0 + l15;
                d4 dr = {0.0, 0.0, 0.0, 0.0}, di = {0.0, 0.0, 0.0, 0.0};
                for (int kk = 0; kk < kq; ++kk) {
                    const int k = 4 * kk + l4;
                    const double2 qa = ia < M && k < kr ? Q.ld_(ia, g0 + k) : make_double2(0.0, 0.0);
                    const double2 wv = Wp[k * 16 + l15];
                    dr = __builtin_amdgcn_mfma_f64_16x16x4f64(qa.x, wv.x, dr, 0, 0, 0);
                    di = __builtin_amdgcn_mfma_f64_16x16x4f64(qa.x, wv.y, di, 0, 0, 0);
                    dr = __builtin_amdgcn_mfma_f64_16x16x4f64(-qa.y, wv.y, dr, 0, 0, 0);
                    di = __builtin_amdgcn_mfma_f64_16x16x4f64(qa.y, wv.x, di, 0, 0, 0);
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int i = i0 + l4 + 4 * reg;
                    if (i < M && pcol) {
                        const double2 o = R.ld_(i, c0 + l15);
                        np_st<TR>(R, i, c0 + l15, make_double2(o.x - dr[reg], o.y - di[reg]));
                    }
                }
            }
            __syncthreads();                                          // the chunk as the next round reads it; W is free again
        }
    // ---- |R_chunk|^2 as it stands now (k = 0: as it came) ----
    const int64_t ne = (int64_t)M * nc;
    for (int64_t e = tid; e < ne; e += NP_THREADS) {
        const int i = TR ? (int)(e / nc) : (int)(e % M), p = TR ? (int)(e % nc) : (int)(e / M);      // along the view's columns
        const double2 x = R.ld_(i, c0 + p);
        r2 += x.x * x.x + x.y * x.y;
    }
}

// stage 1: one workgroup per unit; partial[2 u], partial[2 u + 1] = the unit's |W|^2 and |R|^2
__global__ __launch_bounds__(NP_THREADS) void k_nullproj_units(double2* Rb, const double2* Qb, const htn_nullproj_item* __restrict__ items,
                                                               int n_items, double* __restrict__ partial) {
    __shared__ double2 Wp[NP_NW * NP_WELEMS];
    __shared__ double red[2 * NP_NW];
    // the item of this unit: the units are numbered item after item
    int q = 0, first = 0;
    for (; q < n_items; ++q) {
        const int nu = np_units(items[q].m, items[q].n, items[q].side);
        if ((int)blockIdx.x < first + nu) break;
        first += nu;
    }
    if (q >= n_items) return;                                        // (uniform; the host sized the launch from the same list)
    const htn_nullproj_item it = items[q];
    const int c0 = 16 * ((int)blockIdx.x - first);
    double w2 = 0.0, r2 = 0.0;
    if (it.side == 0)
        np_unit<false>(NpMat<false, double2>{Rb + it.r_off, it.ldr}, NpMat<false, const double2>{Qb + it.q_off, it.ldq}, it.m, it.k, c0,
                       min(16, it.n - c0), Wp, w2, r2);
    else
        np_unit<true>(NpMat<true, double2>{Rb + it.r_off, it.ldr}, NpMat<true, const double2>{Qb + it.q_off, it.ldq}, it.n, it.k, c0,
                      min(16, it.m - c0), Wp, w2, r2);
    w2 = wave_sum(w2);
    r2 = wave_sum(r2);
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) red[tid >> 6] = w2, red[NP_NW + (tid >> 6)] = r2;
    __syncthreads();
    if (tid == 0) {
        partial[2 * (int64_t)blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        partial[2 * (int64_t)blockIdx.x + 1] = (red[4] + red[5]) + (red[6] + red[7]);
    }
}

// stage 2: one workgroup per result: per item the units in unit order, the items in list order
__global__ __launch_bounds__(NP_THREADS) void k_nullproj_reduce(const htn_nullproj_item* __restrict__ items, int n_items,
                                                                const double* __restrict__ partial, double* __restrict__ out) {
    __shared__ int cnt[NP_THREADS], hit[NP_THREADS];
    __shared__ double vw[NP_THREADS], vr[NP_THREADS];
    const int o = blockIdx.x, tid = threadIdx.x;
    double sw = 0.0, sr = 0.0;               // (thread 0) the result so far
    int64_t first = 0;                       // number of the first unit of the current chunk of items (every thread keeps it)
    for (int q0 = 0; q0 < n_items; q0 += NP_THREADS) {
        const int q = q0 + tid, nq = min(NP_THREADS, n_items - q0);
        int nu = 0, mine = 0;
        if (q < n_items) {
            nu = np_units(items[q].m, items[q].n, items[q].side);
            mine = items[q].out == o;
        }
        cnt[tid] = nu;
        __syncthreads();
        int64_t u0 = first, all = 0;         // first unit of this thread's item: the counts before it
        for (int k = 0; k < nq; ++k) {
            if (k < tid) u0 += cnt[k];
            all += cnt[k];
        }
        first += all;
        double w = 0.0, r = 0.0;
        if (mine)
            for (int u = 0; u < nu; ++u) w += partial[2 * (u0 + u)], r += partial[2 * (u0 + u) + 1];
        vw[tid] = w, vr[tid] = r, hit[tid] = mine;
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < nq; ++k)
                if (hit[k]) sw += vw[k], sr += vr[k];
        __syncthreads();
    }
    if (tid == 0) out[2 * o] = sw, out[2 * o + 1] = sr;
}

}  // namespace

extern "C" int htn_block_nullproj_z(void* R, const void* Q, const htn_nullproj_item* items, const htn_nullproj_item* items_host,
                                    int32_t n_items, double* out, int32_t n_out, void* scratch, void* stream) {
    if (n_items < 0 || n_out < 0) return fail_msg("htn_block_nullproj_z: negative count");
    if (n_out == 0) return 0;
    if (!out || (n_items > 0 && (!items || !items_host))) return fail_msg("htn_block_nullproj_z: NULL argument (the host copy of the items is required)");
    int64_t units = 0;
    bool any_q = false;
    for (int q = 0; q < n_items; ++q) {
        const htn_nullproj_item& it = items_host[q];
        const bool bad = it.m < 0 || it.n < 0 || it.k < 0 || (it.side != 0 && it.side != 1) || it.out < 0 || it.out >= n_out || it.r_off < 0 ||
                         (it.m > 0 && it.n > 0 && (it.ldr < it.m || (it.k > 0 && (it.q_off < 0 || it.ldq < (it.side ? it.k : it.m)))));
        if (bad) {
            snprintf(htn_err_buf(), 512, "htn_block_nullproj_z: item %d: m = %d, n = %d, k = %d, ldr = %d, ldq = %d, side = %d, out = %d of %d", q,
                     it.m, it.n, it.k, it.ldr, it.ldq, it.side, it.out, n_out);
            return 1;
        }
        units += HTN_NULLPROJ_UNITS(it.m, it.n, it.side);
        any_q = any_q || (it.m > 0 && it.n > 0 && it.k > 0);
    }
    if (units > INT32_MAX / 2) return fail_msg("htn_block_nullproj_z: too many work units");
    if (units > 0 && (!R || !scratch || (any_q && !Q))) return fail_msg("htn_block_nullproj_z: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    if (units > 0) {
        hipLaunchKernelGGL(k_nullproj_units, dim3((unsigned)units), dim3(NP_THREADS), 0, st, (double2*)R, (const double2*)Q, items, n_items,
                           (double*)scratch);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_nullproj_reduce, dim3(n_out), dim3(NP_THREADS), 0, st, items, n_items, (const double*)scratch, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
