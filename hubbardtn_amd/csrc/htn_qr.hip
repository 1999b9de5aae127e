// Batched unpivoted QR / LQ that forms the orthonormal factor (htn_qr_blocks_z): the gauge move of a one-site DMRG update.
//
// One workgroup (8 waves) per block, grid = number of blocks, no workgroup ever waits for another; nothing but the block
// itself and its R buffer is touched in global memory (no scratch).  Left-looking over panels of w columns held in LDS
// (w = 16 while the panel fits, halved for longer columns):
//   (a) the panel is projected against the finished columns Q: W = Q^H A_p, A_p -= Q W, both on v_mfma_f64_16x16x4_f64.
//       Q is read back through the L2 in groups of 128 columns: one wave per 16-column chunk forms its 16 x w piece of W over
//       all rows (no cross-wave sum), the pieces meet in LDS, then every wave updates 16-row tiles of the panel.  The
//       projection is repeated when some panel column lost more than half of its squared norm in the first one (the
//       Daniel-Gragg-Kaufman-Stewart criterion with eta = 1 / sqrt 2: otherwise one projection already leaves the column
//       orthogonal to Q to a small multiple of rounding) -- "twice is enough"; and once more, without touching R, after (b)
//       when a column shrank to less than half inside the panel, which magnifies what rounding left of Q in it;
//   (b) inside the panel classical Gram-Schmidt, always twice: every thread owns the rows tid, tid + 512, ... of all panel
//       columns, so only the sums cross threads;
//   (c) R collects the coefficients of (a) and (b); the panel goes back in place.
// A column whose remainder is below 1e-13 of its norm gets an exact zero on the diagonal of R and is replaced by the unit
// vector of the row with the least weight in the columns so far, orthogonalised like any other column (a slow, rare path).
// Every sum has a fixed order (lane sums by DPP + v_readlane, the eight wave partials in a fixed tree, MFMA accumulation in
// loop order): two runs give the same bits.  Barriers inside the panel loops order LDS traffic only.
#include <mutex>

#include "htn_common.h"

namespace {

constexpr int QR_NT = HTN_QR_CHUNK;             // threads of a workgroup = rows covered by one pass of the row-owning loops
constexpr int QR_NW = QR_NT / 64;               // waves
constexpr int QR_GROUP = QR_NW * 16;            // finished columns projected per round: one 16-column chunk per wave
constexpr int QR_PANEL_ELEMS = 7680;            // LDS panel, complex128 elements (120 KiB)
constexpr int QR_RED_STRIDE = 34;
constexpr size_t QR_LDS_BYTES = (size_t)(QR_PANEL_ELEMS + QR_GROUP * 16) * sizeof(double2) + (2 * QR_NW * QR_RED_STRIDE + 16) * sizeof(double);
static_assert(QR_NW == 8, "the wave tree of wg_reduce is written for eight waves");
static_assert(QR_LDS_BYTES <= 163840, "LDS of one CU");
static_assert(((HTN_QR_MAX_M + 15) & ~15) + 1 <= QR_PANEL_ELEMS, "a one-column panel must fit");

// workgroup barrier that orders LDS traffic only (__syncthreads() also drains the vector-memory queue)
__device__ __forceinline__ void qr_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

struct QrView {          // the logical m x n matrix M that is factorised: the view itself, or its conjugate transpose
    double2* a;
    int64_t ld;
    bool tr;
};
__device__ __forceinline__ double2 qr_ld(const QrView& v, int i, int j) {
    if (!v.tr) return v.a[(int64_t)j * v.ld + i];
    double2 x = v.a[(int64_t)i * v.ld + j];
    x.y = -x.y;
    return x;
}
__device__ __forceinline__ void qr_st(const QrView& v, int i, int j, double2 x) {
    if (!v.tr) v.a[(int64_t)j * v.ld + i] = x;
    else v.a[(int64_t)i * v.ld + j] = make_double2(x.x, -x.y);
}
struct QrR {             // R (n x n upper) of M; for the LQ case L = R^H is what is stored
    double2* r;
    int64_t ldr;
    bool tr;
};
__device__ __forceinline__ double2* qr_rptr(const QrR& R, int row, int col) {
    return R.tr ? R.r + (int64_t)row * R.ldr + col : R.r + (int64_t)col * R.ldr + row;
}
__device__ __forceinline__ void qr_rset(const QrR& R, int row, int col, double re, double im) {
    *qr_rptr(R, row, col) = make_double2(re, R.tr ? -im : im);
}
__device__ __forceinline__ void qr_radd(const QrR& R, int row, int col, double re, double im) {
    double2* p = qr_rptr(R, row, col);
    const double2 o = *p;
    *p = make_double2(o.x + re, o.y + (R.tr ? -im : im));
}

// sums of NV values over the workgroup, every thread gets them: lanes by wave_sum, the eight waves in a fixed tree.  `red`
// is double buffered, so one LDS barrier per call is enough (a wave can be at most one call ahead of the slowest one).
template <int NV>
__device__ __forceinline__ void wg_reduce(double (&v)[NV], double* red, int& buf, int wave, int lane) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        v[k] = wave_sum(v[k]);
        __builtin_amdgcn_sched_barrier(0);      // one lane sum at a time: interleaving all of them spills the scalar registers
    }
    double* r = red + buf * (QR_NW * QR_RED_STRIDE);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) r[wave * QR_RED_STRIDE + k] = v[k];
    }
    qr_lds_barrier();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        v[k] = ((r[0 * QR_RED_STRIDE + k] + r[1 * QR_RED_STRIDE + k]) + (r[2 * QR_RED_STRIDE + k] + r[3 * QR_RED_STRIDE + k])) +
               ((r[4 * QR_RED_STRIDE + k] + r[5 * QR_RED_STRIDE + k]) + (r[6 * QR_RED_STRIDE + k] + r[7 * QR_RED_STRIDE + k]));
        if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // four sums in flight, not all NV: 8 NV loaded doubles would spill
    }
    buf ^= 1;
}

__global__ __launch_bounds__(QR_NT) void k_qr_blocks(double2* A, double2* Rb, const htn_qr_block* __restrict__ desc) {
    extern __shared__ double2 qr_lds[];
    const htn_qr_block D = desc[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int m = D.m, n = D.n;
    const int mp16 = (m + 15) & ~15, mp = mp16 + 1;          // odd column stride: the 16 columns of a row fall into 16 banks groups
    int w = HTN_QR_PANEL;
    while (w > 1 && w * mp > QR_PANEL_ELEMS) w >>= 1;
    double2* P = qr_lds;                                      // [w][mp] panel
    double2* Wb = qr_lds + QR_PANEL_ELEMS;                    // [QR_GROUP][16] coefficients of one round
    double* red = (double*)(Wb + QR_GROUP * 16);
    double* s_cn = red + 2 * QR_NW * QR_RED_STRIDE;           // [16] squared norms of the panel's original columns
    int rbuf = 0;
    const QrView M{A + D.offset, D.ld, D.trans != 0};
    const QrR R{Rb + D.r_offset, D.ldr, D.trans != 0};

    for (int e = tid; e < n * n; e += QR_NT) {               // the triangle below the diagonal is never written again
        const int r = e % n, c = e / n;
        if (r > c) qr_rset(R, r, c, 0.0, 0.0);
    }

    for (int j0 = 0; j0 < n; j0 += w) {
        const int wp = min(w, n - j0);
        // ---- panel -> LDS; squared norms of the original columns ----
        for (int c = 0; c < wp; ++c) {
            double cn[1] = {0.0};
            for (int i = tid; i < mp; i += QR_NT) {
                const double2 x = i < m ? qr_ld(M, i, j0 + c) : make_double2(0.0, 0.0);
                P[c * mp + i] = x;
                cn[0] += x.x * x.x + x.y * x.y;
            }
            wg_reduce<1>(cn, red, rbuf, wave, lane);
            if (tid == 0) s_cn[c] = cn[0];                    // (read only behind later barriers)
        }
        // ---- (a) projection against the finished columns: mode 0 writes the coefficients to R, 1 adds them, 2 leaves R alone ----
        auto project = [&](int mode) {
            for (int g0 = 0; g0 < j0; g0 += QR_GROUP) {
                const int c0 = g0 + 16 * wave;
                if (c0 < j0) {                                // wave-uniform: this wave's chunk of finished columns
                    d4 cr = {0.0, 0.0, 0.0, 0.0}, ci = {0.0, 0.0, 0.0, 0.0};
                    const int col = c0 + l15, colc = min(col, n - 1);
                    const bool live = col < j0, pcol = l15 < wp;
                    for (int ks = 0; ks < (mp16 >> 2); ++ks) {
                        const int i = 4 * ks + l4;
                        double2 q = qr_ld(M, min(i, m - 1), colc);
                        if (!live) q = make_double2(0.0, 0.0);
                        const double2 b = pcol ? P[l15 * mp + i] : make_double2(0.0, 0.0);      // rows >= m of the panel are zero
                        cr = __builtin_amdgcn_mfma_f64_16x16x4f64(q.x, b.x, cr, 0, 0, 0);
                        ci = __builtin_amdgcn_mfma_f64_16x16x4f64(q.x, b.y, ci, 0, 0, 0);
                        cr = __builtin_amdgcn_mfma_f64_16x16x4f64(q.y, b.y, cr, 0, 0, 0);
                        ci = __builtin_amdgcn_mfma_f64_16x16x4f64(-q.y, b.x, ci, 0, 0, 0);
                    }
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int t = l4 + 4 * reg;
                        Wb[(16 * wave + t) * 16 + l15] = make_double2(cr[reg], ci[reg]);
                        if (c0 + t < j0 && pcol) {
                            if (mode == 0) qr_rset(R, c0 + t, j0 + l15, cr[reg], ci[reg]);
                            else if (mode == 1) qr_radd(R, c0 + t, j0 + l15, cr[reg], ci[reg]);
                        }
                    }
                }
                qr_lds_barrier();
                const int kq = (min(QR_GROUP, j0 - g0) + 15) >> 4 << 2;        // K steps of 4 over the chunks that were formed
                for (int rt = wave; rt < (mp16 >> 4); rt += QR_NW) {
                    const int i0 = 16 * rt, ir = min(i0 + l15, m - 1);
                    d4 dr = {0.0, 0.0, 0.0, 0.0}, di = {0.0, 0.0, 0.0, 0.0};
                    for (int kk = 0; kk < kq; ++kk) {
                        const int k = 4 * kk + l4;
                        const double2 qa = qr_ld(M, ir, min(g0 + k, n - 1));      // columns >= j0 meet zero rows of W
                        const double2 wv = Wb[k * 16 + l15];
                        dr = __builtin_amdgcn_mfma_f64_16x16x4f64(qa.x, wv.x, dr, 0, 0, 0);
                        di = __builtin_amdgcn_mfma_f64_16x16x4f64(qa.x, wv.y, di, 0, 0, 0);
                        dr = __builtin_amdgcn_mfma_f64_16x16x4f64(-qa.y, wv.y, dr, 0, 0, 0);
                        di = __builtin_amdgcn_mfma_f64_16x16x4f64(qa.y, wv.x, di, 0, 0, 0);
                    }
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int i = i0 + l4 + 4 * reg;
                        if (i < m && l15 < wp) {
                            const double2 o = P[l15 * mp + i];
                            P[l15 * mp + i] = make_double2(o.x - dr[reg], o.y - di[reg]);
                        }
                    }
                }
                qr_lds_barrier();
            }
        };
        if (j0 > 0) {
            project(0);
            bool again = false;                               // second projection only when a column lost half of its squared norm
            for (int c = 0; c < wp; ++c) {
                double nn[1] = {0.0};
                for (int i = tid; i < m; i += QR_NT) {
                    const double2 x = P[c * mp + i];
                    nn[0] += x.x * x.x + x.y * x.y;
                }
                wg_reduce<1>(nn, red, rbuf, wave, lane);
                again = again || !(nn[0] >= 0.5 * s_cn[c]);
            }
            if (again) project(1);
        }
        bool cleanup = false;
        // ---- (b) Gram-Schmidt inside the panel, twice; every thread works on its own rows ----
        for (int c = 0; c < wp; ++c) {
            double pre = 0.0;                                 // squared norm of the column when it enters the panel step
            for (int pass = 0; pass < 2 && c > 0; ++pass) {
                double acc[32];
#pragma unroll
                for (int k = 0; k < 32; ++k) acc[k] = 0.0;
                for (int i = tid; i < m; i += QR_NT) {
                    const double2 x = P[c * mp + i];
                    acc[15] += x.x * x.x + x.y * x.y;         // (slot 15 is free: at most 15 columns precede c)
#pragma unroll
                    for (int k = 0; k < 15; ++k)
                        if (k < c) {
                            const double2 q = P[k * mp + i];
                            acc[k] += q.x * x.x + q.y * x.y;
                            acc[16 + k] += q.x * x.y - q.y * x.x;
                        }
                }
                wg_reduce<32>(acc, red, rbuf, wave, lane);
                if (pass == 0) pre = acc[15];
                for (int i = tid; i < m; i += QR_NT) {
                    double2 x = P[c * mp + i];
#pragma unroll
                    for (int k = 0; k < 15; ++k)
                        if (k < c) {
                            const double2 q = P[k * mp + i];
                            x.x -= acc[k] * q.x - acc[16 + k] * q.y;
                            x.y -= acc[k] * q.y + acc[16 + k] * q.x;
                        }
                    P[c * mp + i] = x;
                }
#pragma unroll
                for (int k = 0; k < 15; ++k)                  // thread k keeps row j0 + k of R for this column
                    if (k < c && tid == k) {
                        if (pass == 0) qr_rset(R, j0 + k, j0 + c, acc[k], acc[16 + k]);
                        else qr_radd(R, j0 + k, j0 + c, acc[k], acc[16 + k]);
                    }
            }
            double nr[1] = {0.0};
            for (int i = tid; i < m; i += QR_NT) {
                const double2 x = P[c * mp + i];
                nr[0] += x.x * x.x + x.y * x.y;
            }
            wg_reduce<1>(nr, red, rbuf, wave, lane);
            const double cn = s_cn[c];
            double diag = 0.0;
            if (nr[0] > 1e-26 * cn && nr[0] > 0.0) {
                // what rounding left of the finished columns in this one grows relative to it as it shrinks inside the panel
                cleanup = cleanup || (c > 0 && nr[0] < 0.25 * pre);
                diag = sqrt(nr[0]);
                const double inv = 1.0 / diag;
                for (int i = tid; i < m; i += QR_NT) {
                    const double2 x = P[c * mp + i];
                    P[c * mp + i] = make_double2(x.x * inv, x.y * inv);
                }
            } else {
                // dependent column: complete Q by the unit vector of the row with the least weight in the columns so far (its
                // remainder has squared norm >= (m - columns so far) / m), orthogonalised twice, one column at a time
                double best = 1e300;
                int bi = 0x7fffffff;
                for (int i = tid; i < m; i += QR_NT) {
                    double lev = 0.0;
                    for (int k = 0; k < j0; ++k) {
                        const double2 q = qr_ld(M, i, k);
                        lev += q.x * q.x + q.y * q.y;
                    }
                    for (int k = 0; k < c; ++k) {
                        const double2 q = P[k * mp + i];
                        lev += q.x * q.x + q.y * q.y;
                    }
                    if (lev < best) best = lev, bi = i;
                }
                double* sv = (double*)Wb;                     // (Wb is free between two projection rounds)
                int* si = (int*)(sv + QR_NT);
                sv[tid] = best;
                si[tid] = bi;
                qr_lds_barrier();
                int row = 0x7fffffff;
                best = 1e300;
                for (int t = 0; t < QR_NT; ++t) {
                    const double v = sv[t];
                    const int r = si[t];
                    if (v < best || (v == best && r < row)) best = v, row = r;
                }
                for (int i = tid; i < m; i += QR_NT) P[c * mp + i] = make_double2(i == row ? 1.0 : 0.0, 0.0);
                for (int pass = 0; pass < 2; ++pass)
                    for (int k = 0; k < j0 + c; ++k) {
                        double d[2] = {0.0, 0.0};
                        for (int i = tid; i < m; i += QR_NT) {
                            const double2 q = k < j0 ? qr_ld(M, i, k) : P[(k - j0) * mp + i];
                            const double2 x = P[c * mp + i];
                            d[0] += q.x * x.x + q.y * x.y;
                            d[1] += q.x * x.y - q.y * x.x;
                        }
                        wg_reduce<2>(d, red, rbuf, wave, lane);
                        for (int i = tid; i < m; i += QR_NT) {
                            const double2 q = k < j0 ? qr_ld(M, i, k) : P[(k - j0) * mp + i];
                            double2 x = P[c * mp + i];
                            x.x -= d[0] * q.x - d[1] * q.y;
                            x.y -= d[0] * q.y + d[1] * q.x;
                            P[c * mp + i] = x;
                        }
                    }
                double n2[1] = {0.0};
                for (int i = tid; i < m; i += QR_NT) {
                    const double2 x = P[c * mp + i];
                    n2[0] += x.x * x.x + x.y * x.y;
                }
                wg_reduce<1>(n2, red, rbuf, wave, lane);
                const double inv = 1.0 / sqrt(n2[0]);
                for (int i = tid; i < m; i += QR_NT) {
                    const double2 x = P[c * mp + i];
                    P[c * mp + i] = make_double2(x.x * inv, x.y * inv);
                }
            }
            if (tid == 16) qr_rset(R, j0 + c, j0 + c, diag, 0.0);
        }
        // ---- one more projection of the now orthonormal panel when a column shrank inside it.  The coefficients are of the
        // size of rounding times the shrink factor: R does not need them (their product with the column's row of R is below
        // rounding of the original column) and the panel stays orthonormal to their square ----
        if (j0 > 0 && cleanup) {
            qr_lds_barrier();
            project(2);
        }
        // ---- (c) the finished panel goes back in place; later panels read it through the L2 ----
        for (int c = 0; c < wp; ++c)
            for (int i = tid; i < m; i += QR_NT) qr_st(M, i, j0 + c, P[c * mp + i]);
        __syncthreads();
    }
}

int qr_set_kernel_attributes() {
    static std::mutex attr_mu;
    static bool attr_set[64] = {};
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(attr_mu);
    if (dev >= 0 && dev < 64 && !attr_set[dev]) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_qr_blocks, hipFuncAttributeMaxDynamicSharedMemorySize, (int)QR_LDS_BYTES));
        attr_set[dev] = true;
    }
    return 0;
}

}  // namespace

extern "C" int htn_qr_blocks_z(void* A, void* Rbuf, const htn_qr_block* desc, const htn_qr_block* desc_host, int32_t n_blocks,
                               void* stream) {
    if (n_blocks <= 0) return 0;
    if (!A || !Rbuf || !desc || !desc_host) return fail_msg("htn_qr_blocks_z: bad arguments (the host copy of the descriptors is required)");
    for (int b = 0; b < n_blocks; ++b) {
        const htn_qr_block& D = desc_host[b];
        if (D.n < 1 || D.m < D.n || D.ldr < D.n || D.ld < (D.trans ? D.n : D.m) || D.offset < 0 || D.r_offset < 0) {
            snprintf(htn_err_buf(), 512, "htn_qr_blocks_z: block %d: m = %d, n = %d, ld = %d, ldr = %d (need m >= n >= 1)", b, D.m, D.n,
                     D.ld, D.ldr);
            return 1;
        }
        if (D.m > HTN_QR_MAX_M) {
            snprintf(htn_err_buf(), 512, "htn_qr_blocks_z: block %d has %d rows, the LDS panel holds %d", b, D.m, HTN_QR_MAX_M);
            return 1;
        }
    }
    if (qr_set_kernel_attributes()) return 1;
    hipLaunchKernelGGL(k_qr_blocks, dim3(n_blocks), dim3(QR_NT), QR_LDS_BYTES, (hipStream_t)stream, (double2*)A, (double2*)Rbuf, desc);
    HIP_TRY(hipGetLastError());
    return 0;
}
