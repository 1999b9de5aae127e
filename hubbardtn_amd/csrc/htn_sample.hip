// One site of perfect sampling for a batch of samples (htn_sample_step_z; driver: htn_mps::sample in htn_sample.cpp; DESIGN.md
// section 4j).  Three launches per site, none of which waits for the host:
//   k_sample_probe   T = rho_l A per (sample, item) and the unit's partial sum of Re<A, T>
//   k_sample_choose  per sample: the partial sums added in a fixed order, the draw, log p, the scale of the next rho
//   k_sample_close   rho'_r = scale x sum coef A^H T over the items of the run the draw selects, read from choice[] on the device
// Work unit of probe and close = 64 rows x 16 columns of one output block of one sample: one workgroup of four waves, wave w owns
// the 16 x 16 tile of rows 16 w .. 16 w + 15 on v_mfma_f64_16x16x4_f64 (lane (l15, l4) feeds row / column l15 at K index l4 and
// receives rows l4 + 4 reg of column l15: the operand pattern of htn_nullproj.hip).  Operands come straight from global memory
// through the L2: the site tensor is shared by every sample of the batch, rho and T of a sample are read by the units of that
// sample alone; the left operand is read down its columns (16 lanes x 16 bytes contiguous).  LDS holds the four wave sums of a
// probe unit and the item sums of the choose stage, nothing else.  Every load and store is predicated on the extent of its view.
// Every sum has a fixed order (MFMA accumulation in loop order, wave_sum's tree, the four waves in wave order, units in unit
// order, items in list order), so a sample's numbers do not depend on the batch around it and repeated calls give the same bits.
#include <algorithm>

#include "htn_common.h"

namespace {

constexpr int SM_THREADS = 256;
static_assert(sizeof(htn_sample_item) == 64, "htn_sample_item is a 64-byte record");

__device__ __forceinline__ int sm_units(int m, int n) { return HTN_SAMPLE_UNITS(m, n); }

// the last item q with key(q) <= u (keys ascend; the host checked that key(0) = 0)
template <bool CLOSE>
__device__ __forceinline__ int sm_find(const htn_sample_item* __restrict__ items, int n_items, int u) {
    int lo = 0, hi = n_items - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int key = CLOSE ? items[mid].close_unit0 : items[mid].probe_unit0;
        if (key <= u) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// D (rows i0 .. of M, columns j0 .. of N) = op(X) Y over K, one wave: X is K x M read conjugate-transposed (CT) or M x K read as
// it stands; Y is K x N.  Accumulates into dr / di.
template <bool CT>
__device__ __forceinline__ void sm_tile(const double2* __restrict__ X, int64_t ldx, const double2* __restrict__ Y, int64_t ldy, int M, int N,
                                        int K, int i0, int j0, d4& dr, d4& di) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
    const int i = i0 + l15, j = j0 + l15;
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + l4;
        double2 a = make_double2(0.0, 0.0), b = make_double2(0.0, 0.0);
        if (k < K && i < M) {
            if (CT) {
                a = X[(int64_t)i * ldx + k];
                a.y = -a.y;
            } else
                a = X[(int64_t)k * ldx + i];
        }
        if (k < K && j < N) b = Y[(int64_t)j * ldy + k];
        dr = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, dr, 0, 0, 0);
        di = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.y, di, 0, 0, 0);
        dr = __builtin_amdgcn_mfma_f64_16x16x4f64(-a.y, b.y, dr, 0, 0, 0);
        di = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.x, di, 0, 0, 0);
    }
}

// probe: grid (units, samples)
__global__ __launch_bounds__(SM_THREADS) void k_sample_probe(const double2* __restrict__ rho, const double2* __restrict__ A, double2* __restrict__ T,
                                                             const htn_sample_item* __restrict__ items, int n_items, int64_t rho_stride,
                                                             int64_t t_stride, int n_units, double* __restrict__ partial) {
    __shared__ double red[4];
    const int u = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int q = sm_find<false>(items, n_items, u);
    const htn_sample_item it = items[q];
    const int local = u - it.probe_unit0, ct = (it.n_r + 15) >> 4;
    double dot = 0.0;
    if (local < sm_units(it.n_l, it.n_r)) {                          // (uniform; the host sized the launch from the same list)
        const int i0 = 64 * (local / ct) + 16 * wave, j0 = 16 * (local % ct);
        if (i0 < it.n_l) {                                            // (wave-uniform)
            const double2* R = rho + (int64_t)b * rho_stride + it.rho_off;
            const double2* Ab = A + it.a_off;
            double2* Tb = T + (int64_t)b * t_stride + it.t_off;
            d4 dr = {0.0, 0.0, 0.0, 0.0}, di = {0.0, 0.0, 0.0, 0.0};
            sm_tile<false>(R, it.n_l, Ab, it.lda, it.n_l, it.n_r, it.n_l, i0, j0, dr, di);
            const int j = j0 + l15;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int i = i0 + l4 + 4 * reg;
                if (i < it.n_l && j < it.n_r) {
                    Tb[(int64_t)j * it.n_l + i] = make_double2(dr[reg], di[reg]);
                    const double2 a = Ab[(int64_t)j * it.lda + i];
                    dot += a.x * dr[reg] + a.y * di[reg];
                }
            }
        }
    }
    dot = wave_sum(dot);
    if (lane == 0) red[wave] = dot;
    __syncthreads();
    if (tid == 0) partial[(int64_t)b * n_units + u] = (red[0] + red[1]) + (red[2] + red[3]);
}

// choose: one workgroup per sample
__global__ __launch_bounds__(SM_THREADS) void k_sample_choose(const htn_sample_item* __restrict__ items, int n_items, int n_site, int n_units,
                                                              const double* __restrict__ partial, const double* __restrict__ u, int measure,
                                                              int32_t* __restrict__ choice, double* __restrict__ logp, double* __restrict__ scale) {
    __shared__ double val[SM_THREADS];
    __shared__ int mult[SM_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* part = partial + (int64_t)b * n_units;
    double p[HTN_MAX_SITE] = {0.0, 0.0, 0.0, 0.0};                    // (thread 0)
    for (int q0 = 0; q0 < n_items; q0 += SM_THREADS) {
        const int q = q0 + tid, nq = min(SM_THREADS, n_items - q0);
        double v = 0.0;
        int s = 0;
        if (q < n_items) {
            const int nu = sm_units(items[q].n_l, items[q].n_r), u0 = items[q].probe_unit0;
            for (int k = 0; k < nu; ++k) v += part[u0 + k];
            v *= items[q].coef;
            s = items[q].s;
        }
        val[tid] = v, mult[tid] = s;
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < nq; ++k) {
                const double x = val[k];
                const int m = mult[k];
#pragma unroll
                for (int t = 0; t < HTN_MAX_SITE; ++t)
                    if (t == m) p[t] += x;
            }
        __syncthreads();
    }
    if (tid != 0) return;
    double total = 0.0;
#pragma unroll
    for (int t = 0; t < HTN_MAX_SITE; ++t)
        if (t < n_site) total += p[t];
    if (!measure) {
        choice[b] = -1;
        scale[b] = 1.0 / total;
        return;
    }
    const double target = u[b] * total;
    int pick = -1, last = -1;
    double cum = 0.0, pp = 0.0, pl = 0.0;
#pragma unroll
    for (int t = 0; t < HTN_MAX_SITE; ++t)
        if (t < n_site) {
            cum += p[t];
            if (p[t] > 0.0) {
                last = t, pl = p[t];
                if (pick < 0 && cum >= target) pick = t, pp = p[t];
            }
        }
    if (pick < 0) pick = last, pp = pl;                               // (rounding left the cumulative sum below u x total)
    choice[b] = pick;
    logp[b] += log(pp / total);
    scale[b] = 1.0 / pp;                                              // (a sample without any weight: inf, its rho' is NaN from here on)
}

// close: grid (units, samples)
__global__ __launch_bounds__(SM_THREADS) void k_sample_close(double2* __restrict__ rho_next, const double2* __restrict__ A, const double2* __restrict__ T,
                                                             const htn_sample_item* __restrict__ items, int n_items, int64_t rho_next_stride,
                                                             int64_t t_stride, int measure, const int32_t* __restrict__ choice,
                                                             const double* __restrict__ scale) {
    const int u = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int q = sm_find<true>(items, n_items, u);
    const htn_sample_item it = items[q];
    const int local = u - it.close_unit0, ct = (it.n_r + 15) >> 4, n = it.n_r;
    if (local >= sm_units(n, n)) return;
    const int i0 = 64 * (local / ct) + 16 * wave, j0 = 16 * (local % ct);
    if (i0 >= n) return;
    const int pick = measure ? choice[b] : -1;
    const double2* Tb = T + (int64_t)b * t_stride;
    d4 dr = {0.0, 0.0, 0.0, 0.0}, di = {0.0, 0.0, 0.0, 0.0};
    for (int r = q; r < n_items; ++r) {                               // the run of items that end in this sector
        const int64_t out_off = items[r].out_off;
        if (out_off != it.out_off) break;
        if (measure && items[r].s != pick) continue;
        const int nl = items[r].n_l;
        d4 tr = {0.0, 0.0, 0.0, 0.0}, ti = {0.0, 0.0, 0.0, 0.0};
        sm_tile<true>(A + items[r].a_off, items[r].lda, Tb + items[r].t_off, nl, n, n, nl, i0, j0, tr, ti);
        const double c = items[r].coef;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) dr[reg] += c * tr[reg], di[reg] += c * ti[reg];
    }
    const double f = scale[b];
    double2* O = rho_next + (int64_t)b * rho_next_stride + it.out_off;
    const int j = j0 + l15;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int i = i0 + l4 + 4 * reg;
        if (i < n && j < n) O[(int64_t)j * n + i] = make_double2(f * dr[reg], f * di[reg]);
    }
}

}  // namespace

extern "C" int htn_sample_step_z(void* rho_next, const void* rho, const void* A, void* T, const htn_sample_item* items,
                                 const htn_sample_item* items_host, int32_t n_items, int32_t n_site, int32_t n_samples, int64_t rho_stride,
                                 int64_t rho_next_stride, int64_t t_stride, const double* u, int32_t measure, int32_t* choice, double* logp,
                                 void* scratch, void* stream) {
    if (n_samples == 0) return 0;
    if (n_items <= 0 || n_samples < 0 || n_samples > 65535 || n_site < 1 || n_site > HTN_MAX_SITE)
        return fail_msg("htn_sample_step_z: need n_items >= 1, 1 <= n_samples <= 65535, 1 <= n_site <= HTN_MAX_SITE");
    if (!rho_next || !rho || !A || !T || !items || !items_host || !choice || !logp || !scratch || (measure && !u))
        return fail_msg("htn_sample_step_z: NULL argument (the host copy of the items is required)");
    if (rho_stride < 0 || rho_next_stride < 0 || t_stride < 0) return fail_msg("htn_sample_step_z: negative stride");
    int64_t pu = 0, cu = 0, run_units = 0;
    for (int q = 0; q < n_items; ++q) {
        const htn_sample_item& it = items_host[q];
        const bool first = q == 0 || items_host[q - 1].out_off != it.out_off;
        if (first) cu += run_units, run_units = HTN_SAMPLE_UNITS(it.n_r, it.n_r);
        const int64_t want_cu = first ? cu : cu + run_units;
        const bool bad = it.n_l < 1 || it.n_r < 1 || it.lda < it.n_l || it.s < 0 || it.s >= n_site || it.rho_off < 0 || it.a_off < 0 ||
                         it.t_off < 0 || it.out_off < 0 || it.rho_off + (int64_t)it.n_l * it.n_l > rho_stride ||
                         it.t_off + (int64_t)it.n_l * it.n_r > t_stride || it.out_off + (int64_t)it.n_r * it.n_r > rho_next_stride ||
                         (!first && it.n_r != items_host[q - 1].n_r) || it.probe_unit0 != pu || it.close_unit0 != want_cu;
        if (bad) {
            snprintf(htn_err_buf(), 512, "htn_sample_step_z: item %d: n_l = %d, n_r = %d, lda = %d, s = %d of %d, units %d / %d (expected %lld / %lld) or a view outside its stride",
                     q, it.n_l, it.n_r, it.lda, it.s, n_site, it.probe_unit0, it.close_unit0, (long long)pu, (long long)want_cu);
            return 1;
        }
        pu += HTN_SAMPLE_UNITS(it.n_l, it.n_r);
        if (pu > INT32_MAX / 2 || cu + run_units > INT32_MAX / 2) return fail_msg("htn_sample_step_z: too many work units");
    }
    cu += run_units;
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)scratch;
    double* scale = partial + pu * (int64_t)n_samples;
    hipLaunchKernelGGL(k_sample_probe, dim3((unsigned)pu, (unsigned)n_samples), dim3(SM_THREADS), 0, st, (const double2*)rho, (const double2*)A,
                       (double2*)T, items, n_items, rho_stride, t_stride, (int)pu, partial);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sample_choose, dim3((unsigned)n_samples), dim3(SM_THREADS), 0, st, items, n_items, n_site, (int)pu, (const double*)partial, u,
                       measure, choice, logp, scale);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sample_close, dim3((unsigned)cu, (unsigned)n_samples), dim3(SM_THREADS), 0, st, (double2*)rho_next, (const double2*)A,
                       (const double2*)T, items, n_items, rho_next_stride, t_stride, measure, (const int32_t*)choice, (const double*)scale);
    HIP_TRY(hipGetLastError());
    return 0;
}
