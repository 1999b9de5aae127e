// Krylov vector algebra + Lanczos driver (libhubbardtn_hip.so).
//
// Stands in for KrylovKit.eigsolve(f, x0, 1, :SR, Lanczos(krylovdim, tol, eager)) as MPSKit calls it
// on the AC2 effective Hamiltonian (reached from src/HubbardFunctions.jl:1010).
// All vectors live in HBM; per iteration the host sees only the new tridiagonal coefficients
// (alpha_j, beta_j) -- a 32-byte record in coherent pinned memory -- and solves the <= krylovdim x krylovdim tridiagonal
// eigenproblem itself.  The vector kernels are HBM / Infinity-Cache bandwidth bound for many rows (roofline "hbm") and
// launch-bound for few.
//
// Reductions are two-stage with a fixed summation order (per-block partials, then one wave sums the
// 64 partials with a butterfly), so results are bit-reproducible run to run and rank to rank.
#include <math.h>

#include <atomic>
#include <chrono>
#include <vector>

#include "htn_common.h"
#include "htn_expm.h"
#include "htn_resolvent.h"
#include "htn_tridiag.h"

#define DOT_BLOCKS HTN_DOT_BLOCKS   // partial sums per vector = slices of the vector (4 per lane of the reducing wave)
#define DOT_THREADS 256       // threads of the axpy / scale kernels
#define DOT_CHUNK 32          // vectors handled per pass over the slice of w (krylovdim + 1 <= 31 by default)

// vectors per pass are a compile-time count (all loads of an element in flight at once); rows past nvec are clamped re-reads
// of the last row, which cost real cache traffic -- so the count comes in steps of four (nvec = 17 under a 32-wide
// instantiation took 22 us where 16 rows took 15).  Threads per workgroup (TH) are a template parameter too, but only 256 is
// dispatched: 1024 threads (a slice of 667 elements at chi = 1024 in one step per thread instead of three) changed no
// kernel's duration -- the 4.5-5 us of the small-j kernels are launch + one round trip + the end-of-kernel write-back,
// whatever the thread count (measured, round 3).
#define HTN_CH_DISPATCH(nvec, per, LAUNCH)          \
    do {                                            \
        if ((nvec) <= 4) LAUNCH(4, 256);            \
        else if ((nvec) <= 8) LAUNCH(8, 256);       \
        else if ((nvec) <= 12) LAUNCH(12, 256);     \
        else if ((nvec) <= 16) LAUNCH(16, 256);     \
        else if ((nvec) <= 20) LAUNCH(20, 256);     \
        else if ((nvec) <= 24) LAUNCH(24, 256);     \
        else if ((nvec) <= 28) LAUNCH(28, 256);     \
        else LAUNCH(32, 256);                       \
    } while (0)
static inline int64_t dot_slice(int64_t n) { return (n + DOT_BLOCKS - 1) / DOT_BLOCKS; }

// FROZEN ROWS (htn_lanczos_orth_z).  The three kernels of a Lanczos step take a second base pointer: with FZ the rows of a
// pass are the nf frozen rows Q[0..nf) FOLLOWED by the Krylov rows (row i >= nf is V[i - nf]).  FZ is a template parameter, so
// the instantiations htn_lanczos_z uses (FZ = false) never look at Q / nf: their code and register counts are those of the
// two-pointer-free kernels.
template <bool FZ>
__device__ __forceinline__ const double2* lan_row(const double2* V, const double2* Q, int64_t ldv, int nf, int i) {
    if (FZ && i < nf) return Q + (int64_t)i * ldv;
    return V + (int64_t)(FZ ? i - nf : i) * ldv;
}

// sum of the DOT_BLOCKS partials of one vector by one wave, fixed order
__device__ __forceinline__ double2 reduce_partials(const double2* __restrict__ p, int lane) {
    double sr = 0.0, si = 0.0;
#pragma unroll
    for (int b = 0; b < DOT_BLOCKS / 64; ++b) {
        const double2 v = p[lane + 64 * b];
        sr += v.x;
        si += v.y;
    }
    return make_double2(wave_sum(sr), wave_sum(si));
}

// partial[i * DOT_BLOCKS + b] = sum over slice b of conj(V_i) * w.  Every lane issues all its loads back to back (latency,
// not bandwidth, bounds this kernel at |theta| ~ 10^5); the reductions are the in-wave butterfly plus one fixed-order sum over
// the four waves of a slice.  CH = vectors per pass (compile time, so the loads are unconditional and can all be in flight;
// indices past nvec are clamped and their sums discarded).
// FZ: the rows are Q[0..nf) and then V[upd0 ..] (the two row ranges of the projected first pass), nvec rows in all.
template <int CH, int TH, bool FZ>
__global__ __launch_bounds__(TH) void k_dots_partial(const double2* __restrict__ V, int64_t ldv, int nvec,
                                                      const double2* __restrict__ w, int64_t n,
                                                      double2* __restrict__ partial, const double2* __restrict__ Q, int nf,
                                                      int upd0) {
    // TH / 64 waves per slice: a wave keeps CH + 1 loads in flight per lane and the kernel is bound by the latency of that
    // one batch -- 256 waves on 256 CUs moved 4.7 TB/s; the waves' shares are summed in fixed wave order
    __shared__ double red[TH / 64][CH][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t per = (n + DOT_BLOCKS - 1) / DOT_BLOCKS;
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < n ? lo + per : n;
    for (int i0 = 0; i0 < nvec; i0 += CH) {
        double sr[CH], si[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) sr[c] = si[c] = 0.0;
        for (int64_t j = lo + threadIdx.x; j < hi; j += TH) {
            const double2 b = w[j];
            double2 a[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int i = i0 + c < nvec ? i0 + c : nvec - 1;
                a[c] = lan_row<FZ>(V, Q, ldv, nf, FZ && i >= nf ? i + upd0 : i)[j];
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                sr[c] += a[c].x * b.x + a[c].y * b.y;
                si[c] += a[c].x * b.y - a[c].y * b.x;
            }
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const double r = wave_sum(sr[c]);
            const double m = wave_sum(si[c]);
            if (lane == 0) {
                red[wave][c][0] = r;
                red[wave][c][1] = m;
            }
        }
        __syncthreads();
        if (threadIdx.x < CH && i0 + (int)threadIdx.x < nvec) {
            const int c = threadIdx.x;
            double r = 0.0, m = 0.0;
#pragma unroll
            for (int q = 0; q < TH / 64; ++q) {
                r += red[q][c][0];
                m += red[q][c][1];
            }
            partial[(int64_t)(i0 + c) * DOT_BLOCKS + blockIdx.x] = make_double2(r, m);
        }
        __syncthreads();
    }
}

static void launch_dots_partial(const double2* V, int64_t ldv, int nvec, const double2* w, int64_t n, double2* partial,
                                hipStream_t st) {
#define HTN_DP(CHV, THV)                                                                                                     \
    hipLaunchKernelGGL((k_dots_partial<CHV, THV, false>), dim3(DOT_BLOCKS), dim3(THV), 0, st, V, ldv, nvec, w, n, partial, \
                       (const double2*)nullptr, 0, 0)
    HTN_CH_DISPATCH(nvec, dot_slice(n), HTN_DP);
#undef HTN_DP
}
// rows Q[0..nf) and V[upd0 .. upd0 + nvec - nf)
static void launch_dots_partial_fz(const double2* V, int64_t ldv, int nvec, const double2* w, int64_t n, double2* partial,
                                   const double2* Q, int nf, int upd0, hipStream_t st) {
#define HTN_DP(CHV, THV)                                                                                                    \
    hipLaunchKernelGGL((k_dots_partial<CHV, THV, true>), dim3(DOT_BLOCKS), dim3(THV), 0, st, V, ldv, nvec, w, n, partial, Q, \
                       nf, upd0)
    HTN_CH_DISPATCH(nvec, dot_slice(n), HTN_DP);
#undef HTN_DP
}

// one wave per vector: out[i] = sum_b partial[i][b]
__global__ void k_dots_reduce(const double2* __restrict__ partial, int nvec, double2* __restrict__ out) {
    const int i = blockIdx.x;
    const double2 r = reduce_partials(partial + (int64_t)i * DOT_BLOCKS, threadIdx.x);
    if (threadIdx.x == 0) out[i] = r;
}

// fused: c = reduce(partial); w += sign * V c ; norm_partial[b] = |w_new slice|^2 ; block 0 writes c[c_index]
// to *c_out (a device scalar: the next matvec launch hands it to the host inside the step record).  CH = vectors per pass
// (compile time): all basis loads of an element are in flight together (the earlier version walked them eight at a time, one
// memory round trip per group of eight).
template <int CH, int TH, bool FZ>
__global__ __launch_bounds__(TH) void k_axpy_norm(double2* __restrict__ w, const double2* __restrict__ V,
                                                           int64_t ldv, int nvec,
                                                           const double2* __restrict__ partial,
                                                           double2* __restrict__ c_out, int c_index, double sign,
                                                           int64_t n, double* __restrict__ norm_partial,
                                                           const double2* __restrict__ Q, int nf) {
    __shared__ double cs[64][2];
    __shared__ double red[TH / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = wave; i < nvec; i += TH / 64) {
        const double2 r = reduce_partials(partial + (int64_t)i * DOT_BLOCKS, lane);
        if (lane == 0) {
            cs[i][0] = r.x;
            cs[i][1] = r.y;
            if (blockIdx.x == 0 && i == c_index) *c_out = r;
        }
    }
    if (tid >= nvec && tid < 64) cs[tid][0] = cs[tid][1] = 0.0;      // padding coefficients for the unrolled loop
    __syncthreads();
    const int64_t per = (n + DOT_BLOCKS - 1) / DOT_BLOCKS;
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < n ? lo + per : n;
    double nn = 0.0;
    for (int64_t j = lo + tid; j < hi; j += TH) {
        double2 v[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int i = c < nvec ? c : nvec - 1;
            v[c] = lan_row<FZ>(V, Q, ldv, nf, i)[j];
        }
        double2 x = w[j];
        double sr = 0.0, si = 0.0;
#pragma unroll
        for (int c = 0; c < CH; ++c) {                    // cs[c] = 0 beyond nvec
            sr += cs[c][0] * v[c].x - cs[c][1] * v[c].y;
            si += cs[c][0] * v[c].y + cs[c][1] * v[c].x;
        }
        x.x += sign * sr;
        x.y += sign * si;
        w[j] = x;
        nn += x.x * x.x + x.y * x.y;
    }
    nn = wave_sum(nn);
    if (lane == 0) red[wave] = nn;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < TH / 64; ++q) t += red[q];
        norm_partial[blockIdx.x] = t;
    }
}

static void launch_axpy_norm(double2* w, const double2* V, int64_t ldv, int nvec, const double2* partial, double2* c_out, int c_index,
                             double sign, int64_t n, double* norm_partial, hipStream_t st) {
#define HTN_AN(CHV, THV)                                                                                                    \
    hipLaunchKernelGGL((k_axpy_norm<CHV, THV, false>), dim3(DOT_BLOCKS), dim3(THV), 0, st, w, V, ldv, nvec, partial, c_out, \
                       c_index, sign, n, norm_partial, (const double2*)nullptr, 0)
    HTN_CH_DISPATCH(nvec, dot_slice(n), HTN_AN);
#undef HTN_AN
}
static void launch_axpy_norm_fz(double2* w, const double2* V, int64_t ldv, int nvec, const double2* partial, double2* c_out,
                                int c_index, double sign, int64_t n, double* norm_partial, const double2* Q, int nf,
                                hipStream_t st) {
#define HTN_AN(CHV, THV)                                                                                                   \
    hipLaunchKernelGGL((k_axpy_norm<CHV, THV, true>), dim3(DOT_BLOCKS), dim3(THV), 0, st, w, V, ldv, nvec, partial, c_out, \
                       c_index, sign, n, norm_partial, Q, nf)
    HTN_CH_DISPATCH(nvec, dot_slice(n), HTN_AN);
#undef HTN_AN
}

// first Gram-Schmidt update FUSED with the second pass's dots: c = reduce(partial_in); w += sign * V c; and, while the
// basis values of the element are still in registers, partial_out[i][b] = sum over slice b of conj(V_i) * w_new.
// One read of the Krylov basis instead of two (the basis is the traffic of a Lanczos step: (j+1) x |theta|).
// 256 threads = one wave per SIMD, so the CH basis values + 2 CH accumulators per thread fit the register file.
// DEFERRED NORMALISATION (norm_prev != nullptr): the newest basis row V[nvec-1] is still the raw, unnormalised vector the
// previous step's second update left behind (|raw|^2 = sum norm_prev = beta^2), and w = H raw = beta H v.  This kernel reads
// that row anyway, so it does the previous step's normalisation on the way: s = 1 / beta, the row is written back as
// v = s raw, w is taken as s w, and the dots of K2 (taken with the raw row and the raw w) become c_i = s P_i (i < nvec-1),
// c_last = s^2 P_last.  The separate scale kernel of every step is gone; its record is published by the next matvec launch.
// FZ: rows 0..nf-1 are the frozen rows (normalised, never written), upd0 >= nf, and partial_in holds the dots of the rows
// [0, nf) followed by those of [upd0, nvec): both ranges are subtracted, the Krylov rows between them are not.
template <int CH, int TH, bool FZ>
__global__ __launch_bounds__(TH) void k_axpy_dots(double2* __restrict__ w, double2* __restrict__ V,
                                                           int64_t ldv, int nvec,
                                                           const double2* __restrict__ partial_in,
                                                           double2* __restrict__ c_out, int c_index, double sign,
                                                           int64_t n, double2* __restrict__ partial_out,
                                                           const double* __restrict__ norm_prev, int upd0,
                                                           const double2* __restrict__ Q, int nf) {
    __shared__ double cs[64][2];
    __shared__ double red[TH / 64][CH][2];
    __shared__ double s_scale;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int last = nvec - 1;
    if (tid < 64) {                                   // (wave 0) scale of the deferred normalisation, same order as every norm sum
        double t = 1.0;
        if (norm_prev) {
            t = 0.0;
#pragma unroll
            for (int b = 0; b < DOT_BLOCKS / 64; ++b) t += norm_prev[tid + 64 * b];
            t = wave_sum(t);
            t = t > 0.0 ? 1.0 / sqrt(t) : 0.0;
        }
        if (tid == 0) s_scale = t;
    }
    __syncthreads();
    const double s = s_scale;
    // partial_in holds the dots of rows upd0 .. nvec-1 only (the three-term first pass: upd0 = nvec - 2); the rows below
    // take no part in this update (coefficient 0) but do in the dots taken on the way
    const int skip = FZ ? upd0 - nf : upd0;           // rows [FZ ? nf : 0, upd0) have no entry in partial_in
    for (int p = (FZ ? 0 : upd0) + wave; p < (FZ ? nvec - skip : nvec); p += TH / 64) {
        const int i = FZ && p >= nf ? p + skip : p;
        double2 r = reduce_partials(partial_in + (int64_t)(FZ ? p : i - upd0) * DOT_BLOCKS, lane);
        const bool raw_row = norm_prev && i == last;   // the row this coefficient multiplies is still unnormalised
        const double f = raw_row ? s * s : s;
        r.x *= f;
        r.y *= f;
        if (lane == 0) {
            // the update below uses the rows as stored: the raw row's coefficient carries its factor s
            cs[i][0] = raw_row ? r.x * s : r.x;
            cs[i][1] = raw_row ? r.y * s : r.y;
            if (blockIdx.x == 0 && i == c_index) *c_out = r;
        }
    }
    if ((tid >= nvec || (tid < upd0 && !(FZ && tid < nf))) && tid < 64) cs[tid][0] = cs[tid][1] = 0.0;
    __syncthreads();
    const bool fix = norm_prev != nullptr;
    double2* const vlast = V + (int64_t)(FZ ? last - nf : last) * ldv;
    const int64_t per = (n + DOT_BLOCKS - 1) / DOT_BLOCKS;
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < n ? lo + per : n;
    double ar[CH], ai[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) ar[c] = ai[c] = 0.0;
    for (int64_t j = lo + tid; j < hi; j += TH) {
        double2 v[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int i = c < nvec ? c : nvec - 1;
            v[c] = lan_row<FZ>(V, Q, ldv, nf, i)[j];
        }
        if (fix) {                                    // (uniform) the newest row goes back normalised; v[] keeps it RAW: its factor s
            const double2 vl = vlast[j];              // sits in its coefficient (above) and in its dot (below) -- no per-row select
            vlast[j] = make_double2(vl.x * s, vl.y * s);
        }
        double sr = 0.0, si = 0.0;
#pragma unroll
        for (int c = 0; c < CH; ++c) {                // cs[c] = 0 beyond nvec
            sr += cs[c][0] * v[c].x - cs[c][1] * v[c].y;
            si += cs[c][0] * v[c].y + cs[c][1] * v[c].x;
        }
        double2 x = w[j];
        x.x = fma(x.x, s, sign * sr);
        x.y = fma(x.y, s, sign * si);
        w[j] = x;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            ar[c] += v[c].x * x.x + v[c].y * x.y;     // conj(v) * w_new
            ai[c] += v[c].x * x.y - v[c].y * x.x;
        }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const double r = wave_sum(ar[c]);
        const double m = wave_sum(ai[c]);
        if (lane == 0) {
            red[wave][c][0] = r;
            red[wave][c][1] = m;
        }
    }
    __syncthreads();
    if (tid < CH && tid < nvec) {                     // fixed order over the 4 waves: deterministic
        double r = 0.0, m = 0.0;
#pragma unroll
        for (int q = 0; q < TH / 64; ++q) {
            r += red[q][tid][0];
            m += red[q][tid][1];
        }
        if (fix && tid == last) {                     // <s raw, w> = s <raw, w>
            r *= s;
            m *= s;
        }
        partial_out[(int64_t)tid * DOT_BLOCKS + blockIdx.x] = make_double2(r, m);
    }
}

static void launch_axpy_dots(double2* w, double2* V, int64_t ldv, int nvec, const double2* partial_in, double2* c_out,
                             int c_index, double sign, int64_t n, double2* partial_out, const double* norm_prev, int upd0,
                             hipStream_t st) {
#define HTN_AD(CHV, THV)                                                                                                  \
    hipLaunchKernelGGL((k_axpy_dots<CHV, THV, false>), dim3(DOT_BLOCKS), dim3(THV), 0, st, w, V, ldv, nvec, partial_in, c_out, \
                       c_index, sign, n, partial_out, norm_prev, upd0, (const double2*)nullptr, 0)
    HTN_CH_DISPATCH(nvec, dot_slice(n), HTN_AD);
#undef HTN_AD
}
static void launch_axpy_dots_fz(double2* w, double2* V, int64_t ldv, int nvec, const double2* partial_in, double2* c_out,
                                int c_index, double sign, int64_t n, double2* partial_out, const double* norm_prev, int upd0,
                                const double2* Q, int nf, hipStream_t st) {
#define HTN_AD(CHV, THV)                                                                                                 \
    hipLaunchKernelGGL((k_axpy_dots<CHV, THV, true>), dim3(DOT_BLOCKS), dim3(THV), 0, st, w, V, ldv, nvec, partial_in, c_out, \
                       c_index, sign, n, partial_out, norm_prev, upd0, Q, nf)
    HTN_CH_DISPATCH(nvec, dot_slice(n), HTN_AD);
#undef HTN_AD
}

// dst = src / sqrt(sum norm_partial); with rec_out, block 0 publishes the step record {c1[0].re, c2[0].re, |w|^2}
// (c1 / c2: device scalars written by the EARLIER kernels of the step -- same stream, hence complete and visible)
__global__ __launch_bounds__(DOT_THREADS) void k_scale_by_norm(double2* __restrict__ dst, const double2* __restrict__ src,
                                                               const double* __restrict__ norm_partial, int64_t n,
                                                               LanRecord* __restrict__ rec_out,
                                                               const double2* __restrict__ c1, const double2* __restrict__ c2,
                                                               unsigned long long serial) {
    __shared__ double s_inv;
    const int tid = threadIdx.x;
    if (tid < 64) {
        double t = 0.0;
#pragma unroll
        for (int b = 0; b < DOT_BLOCKS / 64; ++b) t += norm_partial[tid + 64 * b];
        t = wave_sum(t);
        if (tid == 0) {
            s_inv = t > 0.0 ? 1.0 / sqrt(t) : 0.0;
            if (blockIdx.x == 0 && rec_out) {
                const unsigned long long w0 = (unsigned long long)__double_as_longlong(c1[0].x);
                const unsigned long long w1 = (unsigned long long)__double_as_longlong(c2[0].x);
                const unsigned long long w2 = (unsigned long long)__double_as_longlong(t);
                ulonglong2* out = (ulonglong2*)rec_out;
                out[0] = make_ulonglong2(w0, w1);
                out[1] = make_ulonglong2(w2, lan_check(w0, w1, w2, serial));
                __threadfence_system();
            }
        }
    }
    __syncthreads();
    const double s = s_inv;
    for (int64_t j = (int64_t)blockIdx.x * DOT_THREADS + tid; j < n; j += (int64_t)gridDim.x * DOT_THREADS) {
        const double2 v = src[j];
        dst[j] = make_double2(v.x * s, v.y * s);
    }
}

// the record of a step that no further matvec launch follows (the last step of a restart cycle): one wave
__global__ __launch_bounds__(64) void k_publish_record(const double* __restrict__ norm_partial, const double2* __restrict__ c1,
                                                       const double2* __restrict__ c2, LanRecord* __restrict__ rec_out,
                                                       unsigned long long serial) {
    const int tid = threadIdx.x;
    double t = 0.0;
#pragma unroll
    for (int b = 0; b < DOT_BLOCKS / 64; ++b) t += norm_partial[tid + 64 * b];
    t = wave_sum(t);
    if (tid == 0) {
        const unsigned long long w0 = (unsigned long long)__double_as_longlong(c1[0].x);
        const unsigned long long w1 = (unsigned long long)__double_as_longlong(c2[0].x);
        const unsigned long long w2 = (unsigned long long)__double_as_longlong(t);
        ulonglong2* out = (ulonglong2*)rec_out;
        out[0] = make_ulonglong2(w0, w1);
        out[1] = make_ulonglong2(w2, lan_check(w0, w1, w2, serial));
        __threadfence_system();
    }
}

// |w|^2 partials only (start-vector normalisation)
__global__ __launch_bounds__(DOT_THREADS) void k_norm_partial(const double2* __restrict__ w, int64_t n,
                                                              double* __restrict__ norm_partial) {
    __shared__ double red[DOT_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t per = (n + DOT_BLOCKS - 1) / DOT_BLOCKS;
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < n ? lo + per : n;
    double nn = 0.0;
    for (int64_t j = lo + tid; j < hi; j += DOT_THREADS) {
        const double2 x = w[j];
        nn += x.x * x.x + x.y * x.y;
    }
    nn = wave_sum(nn);
    if ((tid & 63) == 0) red[tid >> 6] = nn;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int q = 0; q < DOT_THREADS / 64; ++q) t += red[q];
        norm_partial[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(256) void k_axpys(double2* __restrict__ w, const double2* __restrict__ V,
                                               int64_t ldv, int nvec, const double2* __restrict__ coef,
                                               double sign, int64_t n) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        double sr = 0.0, si = 0.0;
        for (int i = 0; i < nvec; ++i) {
            const double2 c = coef[i];
            const double2 v = V[(int64_t)i * ldv + j];
            sr += c.x * v.x - c.y * v.y;
            si += c.x * v.y + c.y * v.x;
        }
        double2 x = w[j];
        x.x += sign * sr;
        x.y += sign * si;
        w[j] = x;
    }
}

__global__ __launch_bounds__(256) void k_scale_inv_sqrt(double2* __restrict__ dst, const double2* __restrict__ src,
                                                        const double2* __restrict__ nrm2, int64_t n) {
    const double s = 1.0 / sqrt(nrm2[0].x);
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const double2 v = src[j];
        dst[j] = make_double2(v.x * s, v.y * s);
    }
}

// Krylov exponential (htn_krylov_expm_z): V[0] <- sum_i c_i V[i] in place, i < nvec, for an ORTHONORMAL basis and host
// coefficients already divided by |c|_2 -- the result has norm 1 without a norm pass.  The coefficients travel BY VALUE in the
// kernel arguments (32 double2 = 512 B: no staging buffer, no copy, nothing to drain before it is reused).  One launch; it
// reads nvec n 16 B and writes n 16 B.  A thread reads its element of every row (CH 16-byte loads in flight, coalesced down
// each row; rows past nvec are clamped re-reads with coefficient 0) BEFORE it writes its element of row 0, and no other
// thread touches that element: the in-place update is safe.
struct KrylovCoef {
    double2 c[DOT_CHUNK];
};
template <int CH, int TH>
__global__ __launch_bounds__(TH) void k_krylov_combine(double2* V, int64_t ldv, int nvec, int64_t n, const KrylovCoef kc) {
    for (int64_t j = (int64_t)blockIdx.x * TH + threadIdx.x; j < n; j += (int64_t)gridDim.x * TH) {
        double2 v[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int i = c < nvec ? c : nvec - 1;
            v[c] = V[(int64_t)i * ldv + j];
        }
        double sr = 0.0, si = 0.0;
#pragma unroll
        for (int c = 0; c < CH; ++c) {                    // kc.c[c] = 0 beyond nvec
            sr += kc.c[c].x * v[c].x - kc.c[c].y * v[c].y;
            si += kc.c[c].x * v[c].y + kc.c[c].y * v[c].x;
        }
        V[j] = make_double2(sr, si);
    }
}

static inline int grid_for(int64_t n) {
    int64_t b = (n + 255) / 256;
    return (int)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

static void launch_krylov_combine(double2* V, int64_t ldv, int nvec, int64_t n, const KrylovCoef& kc, hipStream_t st) {
#define HTN_KC(CHV, THV) hipLaunchKernelGGL((k_krylov_combine<CHV, THV>), dim3(grid_for(n)), dim3(THV), 0, st, V, ldv, nvec, n, kc)
    HTN_CH_DISPATCH(nvec, dot_slice(n), HTN_KC);
#undef HTN_KC
}

// Shifted solve (htn_krylov_solve_z): the two updates that end a restart cycle in ONE launch,
//   X <- (keep ? X : 0) + sum_{i < m} y_i V[i]        and, with have_rho,        V[0] <- sum_{i <= m} rho_i V[i].
// Both coefficient sets travel BY VALUE (2 x 32 double2 = 1 KiB of kernel arguments: no staging buffer, nothing to drain); the
// host pads them with zeros, so one row count (nvec = the rows read) serves both sums.  A thread reads its element of every row
// and of X (CH + 1 16-byte loads in flight, coalesced down each row; rows past nvec are clamped re-reads with coefficient 0)
// BEFORE it writes its element of X and of row 0, and no other thread touches that element: both in-place updates are safe.
// Memory bound: (nvec + 1) n 16 B read, 2 n 16 B written; without rho (a converged cycle) only X is written.
struct KrylovCoef2 {
    double2 y[DOT_CHUNK], r[DOT_CHUNK];
};
template <int CH, int TH>
__global__ __launch_bounds__(TH) void k_krylov_combine2(double2* V, int64_t ldv, int nvec, int64_t n, double2* __restrict__ X, int keep,
                                                        int have_rho, const KrylovCoef2 kc) {
    for (int64_t j = (int64_t)blockIdx.x * TH + threadIdx.x; j < n; j += (int64_t)gridDim.x * TH) {
        double2 v[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int i = c < nvec ? c : nvec - 1;
            v[c] = V[(int64_t)i * ldv + j];
        }
        double2 x = make_double2(0.0, 0.0);
        if (keep) x = X[j];
        double sr = 0.0, si = 0.0, tr = 0.0, ti = 0.0;
#pragma unroll
        for (int c = 0; c < CH; ++c) {                    // kc.y[c] = kc.r[c] = 0 beyond their counts
            sr += kc.y[c].x * v[c].x - kc.y[c].y * v[c].y;
            si += kc.y[c].x * v[c].y + kc.y[c].y * v[c].x;
            tr += kc.r[c].x * v[c].x - kc.r[c].y * v[c].y;
            ti += kc.r[c].x * v[c].y + kc.r[c].y * v[c].x;
        }
        X[j] = make_double2(x.x + sr, x.y + si);
        if (have_rho) V[j] = make_double2(tr, ti);
    }
}

static void launch_krylov_combine2(double2* V, int64_t ldv, int nvec, int64_t n, double2* X, int keep, int have_rho, const KrylovCoef2& kc,
                                   hipStream_t st) {
#define HTN_KC2(CHV, THV) \
    hipLaunchKernelGGL((k_krylov_combine2<CHV, THV>), dim3(grid_for(n)), dim3(THV), 0, st, V, ldv, nvec, n, X, keep, have_rho, kc)
    HTN_CH_DISPATCH(nvec, dot_slice(n), HTN_KC2);
#undef HTN_KC2
}

extern "C" int64_t htn_dots_scratch_elems(int32_t nvec) { return (int64_t)nvec * DOT_BLOCKS; }

extern "C" int htn_dots_z(const void* V, int64_t ldv, int32_t nvec, const void* w, int64_t n, void* out,
                          void* scratch, void* stream) {
    if (nvec <= 0) return 0;
    if (nvec > 64) return fail_msg("htn_dots_z: nvec > 64");
    launch_dots_partial((const double2*)V, ldv, nvec, (const double2*)w, n, (double2*)scratch, (hipStream_t)stream);
    hipLaunchKernelGGL(k_dots_reduce, dim3(nvec), dim3(64), 0, (hipStream_t)stream, (const double2*)scratch,
                       nvec, (double2*)out);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int htn_axpys_z(void* w, const void* V, int64_t ldv, int32_t nvec, const void* coef, double sign,
                           int64_t n, void* stream) {
    if (nvec <= 0 || n <= 0) return 0;
    hipLaunchKernelGGL(k_axpys, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (double2*)w, (const double2*)V,
                       ldv, nvec, (const double2*)coef, sign, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int htn_scale_inv_sqrt_z(void* dst, const void* src, const void* nrm2, int64_t n, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_scale_inv_sqrt, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (double2*)dst,
                       (const double2*)src, (const double2*)nrm2, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ----------------------------------------------------------------------------------------------
// host side of the Lanczos driver
// ----------------------------------------------------------------------------------------------
// (the lowest eigenpair of the tridiagonal matrix: htn_tridiag.h, shared with the host statement of the projected solve)
using htn::tridiag_lowest;

extern "C" int64_t htn_lanczos_scratch_elems(int32_t krylovdim) {
    // 2 x partial sums (krylovdim+1 vectors) + c1 + c2 + y (each krylovdim+1) + norm partials (as doubles); the y block is
    // no longer written (the Ritz coefficients travel in the kernel arguments) and keeps its place in the layout
    return 2 * (int64_t)(krylovdim + 1) * DOT_BLOCKS + 3 * (krylovdim + 1) + DOT_BLOCKS + 8;
}

// ---- per-stream resources of the driver (htn_common.h: owned by the stream's registry entry) ----------------------------
#define LAN_SLOTS 64
namespace {
struct LanRes {
    int device = -1;
    LanRecord* h_rec = nullptr;      // [LAN_SLOTS] host view  \ hipHostMallocMapped | hipHostMallocCoherent: written by the
    LanRecord* d_rec = nullptr;      //             device view / device only, read by the host only
    hipEvent_t ev_done[LAN_SLOTS], ev_mv0[LAN_SLOTS], ev_mv1[LAN_SLOTS];
    bool have_events = false;
    unsigned long long serial = 0;   // last step serial handed out; never reused within the life of the entry
    unsigned sample = 0;             // phase of the 1-in-8 matvec timing sample
    ~LanRes() {
        if (device >= 0) (void)hipSetDevice(device);
        if (h_rec) (void)hipHostFree(h_rec);
        if (have_events)
            for (int i = 0; i < LAN_SLOTS; ++i) {
                (void)hipEventDestroy(ev_done[i]);
                (void)hipEventDestroy(ev_mv0[i]);
                (void)hipEventDestroy(ev_mv1[i]);
            }
    }
};
HtnStreamRegistry<LanRes> g_lan_res;

int lan_res_get(hipStream_t st, LanRes** out) {
    return g_lan_res.get(st, out, [](LanRes& r) -> int {
        HIP_TRY(hipHostMalloc((void**)&r.h_rec, sizeof(LanRecord) * LAN_SLOTS, hipHostMallocMapped | hipHostMallocCoherent));
        memset(r.h_rec, 0, sizeof(LanRecord) * LAN_SLOTS);      // (before any device work can see the block)
        HIP_TRY(hipHostGetDevicePointer((void**)&r.d_rec, r.h_rec, 0));
        for (int i = 0; i < LAN_SLOTS; ++i) {
            HIP_TRY(hipEventCreateWithFlags(&r.ev_done[i], hipEventDisableTiming));
            HIP_TRY(hipEventCreate(&r.ev_mv0[i]));
            HIP_TRY(hipEventCreate(&r.ev_mv1[i]));
        }
        r.have_events = true;
        return 0;
    });
}
}  // namespace

void htn_krylov_release_stream(hipStream_t st) { g_lan_res.release(st); }

// ---- closing a solve at the step that is expected to converge -------------------------------------------------------------
// An OPEN step is followed by the next step before the host has seen its record (the next step's first matvec launch carries
// the record): if it converges, the step behind it ran for nothing -- the most expensive step of the solve.  A CLOSED step is
// followed by k_publish_record and nothing else until the host has its record: if it converges no launch was wasted, if it does
// not the GPU idles for one host round trip before the next step arrives.
//   HTN_LANCZOS_CLOSE (read once per process)   unset / auto: the predictor below decides, step by step
//                                               never:        every step is open but the last of a cycle
//                                               always:       every step is closed (slow: a round trip per step)
enum LanClose { LAN_CLOSE_AUTO, LAN_CLOSE_NEVER, LAN_CLOSE_ALWAYS };
static LanClose lan_close_mode() {
    static const LanClose mode = [] {
        const char* v = getenv("HTN_LANCZOS_CLOSE");
        if (v && !strcmp(v, "never")) return LAN_CLOSE_NEVER;
        if (v && !strcmp(v, "always")) return LAN_CLOSE_ALWAYS;
        return LAN_CLOSE_AUTO;
    }();
    return mode;
}
// Is the step after those whose residuals |beta y_last| are in `res` expected to converge?  Geometric extrapolation of the last
// two residuals.  A pure function of the records and tol: every rank of a multi-rank run takes the same decision, and tol = 0
// never closes.
static bool lan_expect_convergence(const std::vector<double>& res, double tol) {
    const size_t k = res.size();
    if (k < 2) return false;
    const double r0 = res[k - 2], r1 = res[k - 1];
    return r1 < r0 && r1 * (r1 / r0) < tol;
}
// process totals for HTN_DEBUG_HOST_TIMERS: closed steps that converged / that did not; convergences at an open step
static std::atomic<long long> g_lan_close_hit{0}, g_lan_close_miss{0}, g_lan_open_conv{0};

// what lanczos_run needs of a shifted solve besides the host decisions: the caller's X and what became of it
struct SolveHook {
    htn_resolvent::Resolvent rs;
    double2* X = nullptr;
    bool use_guess = false;
    double xnorm = 0.0;
};

// The driver of htn_lanczos_z (nf = 0) and htn_lanczos_orth_z (nf frozen rows Q: lowest eigenpair of P H P, P = 1 - Q Q^H).
// With frozen rows every pass of a step runs over Q followed by the Krylov rows: the first (short) pass takes the dots with
// Q AND {V[j-1], V[j]} -- H v_j has O(|H|) components along Q, not O(eps |H|) -- and the second pass is the full one it always
// was; alpha_j, the deferred normalisation, the records and the pipeline do not change.  nf = 0 enqueues exactly the kernels,
// arguments and order of the driver before frozen rows existed.
static int lanczos_run(const htn_gemm_launch* stages, int32_t n_stages, int32_t x_slot, int32_t y_slot,
                       void* Vv, int64_t n, int32_t krylovdim, double tol, int32_t max_restart,
                       void* scratch, int32_t zero_y, htn_exchange2_fn exchange, void* user,
                       double* eig_host, int32_t* n_matvec_host, double* residual_host,
                       double* matvec_ms_host, void* stream_v, const double2* Q, int nf, htn_expm::Expm* ex = nullptr,
                       SolveHook* sv = nullptr) {
    hipStream_t st = (hipStream_t)stream_v;
    const int kd = krylovdim;
    const int kt = kd + nf;                                        // rows of the widest pass + 1
    double2* V = (double2*)Vv;
    double2* partial = (double2*)scratch;
    double2* partial2 = partial + (int64_t)(kt + 1) * DOT_BLOCKS;
    double2* c1 = partial2 + (int64_t)(kt + 1) * DOT_BLOCKS;      // device scalars <v_j, w>: first / second pass
    double2* c2 = c1 + (kt + 1);
    double2* ycoef = c2 + (kt + 1);
    double* norm_partial = (double*)(ycoef + (kt + 1));

    LanRes* R = nullptr;
    if (lan_res_get(st, &R)) return 1;
    const bool event_waits = htn_debug_event_waits();
    static const bool full_first_pass = htn_env_flag("HTN_LANCZOS_FULL_FIRST_PASS");

    const LanClose close_mode = ex || sv ? LAN_CLOSE_NEVER : lan_close_mode();
    bool timed_step[LAN_SLOTS] = {false};
    bool closed[LAN_SLOTS] = {false};             // the step published its own record (k_publish_record)
    unsigned long long step_serial[LAN_SLOTS] = {0};
    // (expm with dt = 0: the identity needs alpha_0 only -- one step that publishes its own record, nothing speculative)
    const bool solo = ex && ex->dt_re == 0.0 && ex->dt_im == 0.0;
    auto matvec = [&](double2* x, double2* y, const HtnGemmPublish* pub) -> int {
        if (zero_y) HIP_TRY(hipMemsetAsync(y, 0, sizeof(double2) * n, st));
        bool published = pub == nullptr;
        for (int s = 0; s < n_stages; ++s) {
            const void* bufs[HTN_MAX_BUFS];
            for (int b = 0; b < HTN_MAX_BUFS; ++b) bufs[b] = stages[s].bufs[b];
            bufs[x_slot] = x;
            bufs[y_slot] = y;
            const bool here = !published && stages[s].n_tiles > 0;        // the first launch of the matvec carries the record
            if (htn_grouped_gemm_launch(bufs, stages[s].tiles, stages[s].n_tiles, stages[s].segs, here ? pub : nullptr, st)) return 1;
            published |= here;
        }
        if (!published)         // (a matvec without a single tile: publish by the one-wave kernel)
            hipLaunchKernelGGL(k_publish_record, dim3(1), dim3(64), 0, st, pub->norm_partial, pub->c1, pub->c2, pub->rec_out, pub->serial);
        if (exchange && exchange(y, n, user)) return fail_msg("htn_lanczos_z: the exchange hook reported a failure");
        return 0;
    };
    // One Lanczos step, fully enqueued: w = H V[j]; two Gram-Schmidt passes against V[0..j]; the result stays UNNORMALISED in
    // V[j+1] with its squared norm in norm_partial.  For j > 0 (inside a cycle) V[j] itself is still the raw vector of step
    // j - 1: its normalisation is folded into this step's first update (k_axpy_dots, norm_prev) and the record of step j - 1 is
    // published by this step's first matvec launch -- four kernels per step instead of five.  The last step of a cycle
    // publishes its own record (nothing follows it).  `first` = V[j] is already normalised (start / Ritz vector).  `carry` = this
    // step's first matvec launch publishes the record of step j - 1 (false behind a closed step: that record has been delivered).
    auto publish_step = [&](int j) -> int {
        hipLaunchKernelGGL(k_publish_record, dim3(1), dim3(64), 0, st, (const double*)norm_partial, (const double2*)(c1 + j),
                           (const double2*)(c2 + j), R->d_rec + j, step_serial[j]);
        if (event_waits) HIP_TRY(hipEventRecord(R->ev_done[j], st));
        closed[j] = true;
        return 0;
    };
    auto enqueue_step = [&](int j, bool first, bool carry) -> int {
        double2* vj = V + (int64_t)j * n;
        double2* w = V + (int64_t)(j + 1) * n;
        // HIP events around a SAMPLE of the matvec launches (every 8th): an event is a marker packet that costs ~5 us
        // of pipeline bubble on this part, three of them per step were 15 us of a ~105 us Lanczos step
        const bool timed = matvec_ms_host && (R->sample % 8) == 0;
        timed_step[j] = timed;
        closed[j] = false;
        ++R->sample;
        step_serial[j] = ++R->serial;
        HtnGemmPublish pub = {nullptr, nullptr, nullptr, nullptr, 0ull};
        if (carry) pub = {norm_partial, (const double2*)(c1 + (j - 1)), (const double2*)(c2 + (j - 1)), R->d_rec + (j - 1), step_serial[j - 1]};
        if (timed) HIP_TRY(hipEventRecord(R->ev_mv0[j], st));
        if (matvec(vj, w, carry ? &pub : nullptr)) return 1;
        if (timed) HIP_TRY(hipEventRecord(R->ev_mv1[j], st));
        if (carry && event_waits) HIP_TRY(hipEventRecord(R->ev_done[j - 1], st));
        // Orthogonalisation in three kernels and TWO passes over the basis.  First the three-term part: dots with V[j-1]
        // and V[j] only, w' = w - V[j-1] c - V[j] c (against a basis that is orthonormal to rounding every other component
        // of H v_j is O(eps |H|): <v_i, H v_j> = conj(<v_j, H v_i>) and H v_i has no component along v_j for j > i + 1);
        // the kernel that makes w' takes the dots of w' with ALL rows on the way, and the last kernel subtracts those --
        // a full classical Gram-Schmidt pass whose coefficients are O(eps |H|) and whose result is orthogonal to eps |w'|,
        // which is what the second pass of a two-pass scheme delivers.  (Until round 3 the first pass was a full one as well:
        // one more read of the whole basis per step; HTN_LANCZOS_FULL_FIRST_PASS=1 brings it back for comparison.)
        const int upd0 = full_first_pass || j < 2 ? 0 : j - 1;
        if (nf == 0) {
            launch_dots_partial(V + (int64_t)upd0 * n, n, j + 1 - upd0, w, n, partial, st);
            launch_axpy_dots(w, V, n, j + 1, partial, c1 + j, j, -1.0, n, partial2, first ? (const double*)nullptr : norm_partial, upd0, st);
            launch_axpy_norm(w, V, n, j + 1, partial2, c2 + j, j, -1.0, n, norm_partial, st);
        } else {
            launch_dots_partial_fz(V, n, nf + j + 1 - upd0, w, n, partial, Q, nf, upd0, st);
            launch_axpy_dots_fz(w, V, n, nf + j + 1, partial, c1 + j, nf + j, -1.0, n, partial2,
                                first ? (const double*)nullptr : norm_partial, nf + upd0, Q, nf, st);
            launch_axpy_norm_fz(w, V, n, nf + j + 1, partial2, c2 + j, nf + j, -1.0, n, norm_partial, Q, nf, st);
        }
        if (j == kd - 1 || solo) return publish_step(j);
        return 0;
    };
    // read slot j if it holds the record of THIS step (see LanRecord): true = accepted
    auto read_record = [&](int j, double* a1, double* a2, double* nn) -> bool {
        const volatile unsigned long long* p = R->h_rec[j].w;
        const unsigned long long w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3];
        if (w3 != lan_check(w0, w1, w2, step_serial[j])) return false;
        memcpy(a1, &w0, 8);
        memcpy(a2, &w1, 8);
        memcpy(nn, &w2, 8);
        return true;
    };
    // wait for step j's record.  Product path: poll the slot (the host wakes within the PCIe latency of the store; a
    // sleeping wait costs tens of us per step).  A stream that has drained without the record arriving means the step never
    // ran to its end (a fault): report instead of spinning forever.  HTN_DEBUG_EVENT_WAITS: wait for the step's event, after
    // which the record MUST validate.
    auto wait_step = [&](int j, double* a1, double* a2, double* nn) -> int {
        if (event_waits) {
            HIP_TRY(hipEventSynchronize(R->ev_done[j]));
            if (!read_record(j, a1, a2, nn)) return fail_msg("htn_lanczos_z: the step's event completed but its record does not validate");
            return 0;
        }
        for (unsigned spins = 1;; ++spins) {
            if (read_record(j, a1, a2, nn)) return 0;
            __builtin_ia32_pause();
            if ((spins & 0xffff) == 0) {
                const hipError_t q = hipStreamQuery(st);
                if (q == hipSuccess)
                    return read_record(j, a1, a2, nn) ? 0 : fail_msg("htn_lanczos_z: the stream drained without producing the step's record");
                if (q != hipErrorNotReady) return fail("hipStreamQuery", q);
            }
        }
    };

    // w -= Q (Q^H w), twice; the second update leaves |w|^2 in norm_partial (c_index -1: no coefficient is published)
    auto project_out = [&](double2* w) {
        for (int pass = 0; pass < 2; ++pass) {
            launch_dots_partial(Q, n, nf, w, n, partial, st);
            launch_axpy_norm(w, Q, n, nf, partial, c1, -1, -1.0, n, norm_partial, st);
        }
    };
    double mv_ms = 0.0;
    int nmv = 0, n_timed = 0;
    // (shifted solve) the squared norm in norm_partial -> host: the record of the last slot, which no step uses (krylovdim <= 31)
    auto fetch_norm2 = [&](double* out) -> int {
        const int q = LAN_SLOTS - 1;
        step_serial[q] = ++R->serial;
        hipLaunchKernelGGL(k_publish_record, dim3(1), dim3(64), 0, st, (const double*)norm_partial, (const double2*)c1, (const double2*)c2,
                           R->d_rec + q, step_serial[q]);
        if (event_waits) HIP_TRY(hipEventRecord(R->ev_done[q], st));
        double a1 = 0.0, a2 = 0.0;
        if (wait_step(q, &a1, &a2, out)) return 1;
        if (!(*out == *out)) return fail_msg("htn_krylov_solve_z: NaN in a vector norm (operator, right-hand side or start value not finite)");
        return 0;
    };
    // (shifted solve) |X| -> host, V[0] = X / |X|: the end of every solve whose norm the host does not know already
    auto normalise_x = [&]() -> int {
        double x2 = 0.0;
        hipLaunchKernelGGL(k_norm_partial, dim3(DOT_BLOCKS), dim3(DOT_THREADS), 0, st, (const double2*)sv->X, n, norm_partial);
        if (fetch_norm2(&x2)) return 1;
        hipLaunchKernelGGL(k_scale_by_norm, dim3(grid_for(n)), dim3(DOT_THREADS), 0, st, V, (const double2*)sv->X, norm_partial, n,
                           (LanRecord*)nullptr, (const double2*)nullptr, (const double2*)nullptr, 0ull);
        sv->xnorm = sqrt(x2);
        return 0;
    };
    // normalise the start vector (frozen rows: projected first)
    if (nf > 0) project_out(V);
    else
    hipLaunchKernelGGL(k_norm_partial, dim3(DOT_BLOCKS), dim3(DOT_THREADS), 0, st, V, n, norm_partial);
    if (sv) {
        // |b| is the scale of the stopping rule; with a start value the basis is built from r0 = b - z x0 + H x0 (one matvec into
        // row 1, two axpys with the coefficients in the unused y block of the scratch)
        double b2 = 0.0, r2 = 0.0;
        if (fetch_norm2(&b2)) return 1;
        if (!(b2 > 0.0)) return fail_msg("htn_krylov_solve_z: the right-hand side is zero");
        sv->rs.bnorm = sqrt(b2);
        r2 = b2;
        if (sv->use_guess) {
            const double2 h[2] = {make_double2(-sv->rs.z.real(), -sv->rs.z.imag()), make_double2(1.0, 0.0)};
            HIP_TRY(hipMemcpyAsync(ycoef, h, sizeof(h), hipMemcpyHostToDevice, st));
            HIP_TRY(htn_stream_spin(st));                    // (h is on this frame)
            if (matvec(sv->X, V + n, nullptr)) return 1;
            ++nmv;
            hipLaunchKernelGGL(k_axpys, dim3(grid_for(n)), dim3(256), 0, st, V, (const double2*)sv->X, n, 1, (const double2*)ycoef, 1.0, n);
            hipLaunchKernelGGL(k_axpys, dim3(grid_for(n)), dim3(256), 0, st, V, (const double2*)(V + n), n, 1, (const double2*)(ycoef + 1), 1.0, n);
            hipLaunchKernelGGL(k_norm_partial, dim3(DOT_BLOCKS), dim3(DOT_THREADS), 0, st, V, n, norm_partial);
            if (fetch_norm2(&r2)) return 1;
        }
        sv->rs.begin_cycle(sqrt(r2 > 0.0 ? r2 : 0.0));
        if (sv->rs.converged) {                              // the start value solves the system: x = x0
            if (!sv->use_guess) return fail_msg("htn_krylov_solve_z: tol >= 1 accepts x = 0");
            if (normalise_x()) return 1;
            HIP_TRY(hipGetLastError());
            *n_matvec_host = nmv;
            *residual_host = sv->rs.resid;
            if (matvec_ms_host) *matvec_ms_host = -1.0;
            return 0;
        }
    }
    hipLaunchKernelGGL(k_scale_by_norm, dim3(grid_for(n)), dim3(DOT_THREADS), 0, st, V, V, norm_partial, n,
                       (LanRecord*)nullptr, (const double2*)nullptr, (const double2*)nullptr, 0ull);
    static const bool dbg_timers = getenv("HTN_DEBUG_HOST_TIMERS") != nullptr;
    auto now_us = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t_enq = 0.0, t_wait = 0.0, t_host = 0.0;
    const double t_begin = now_us();
    double theta = 0.0, res = 0.0, beta = 0.0, amax = 0.0;
    std::vector<double> y;
    for (int restart = 0; restart <= max_restart; ++restart) {
        std::vector<double> alphas, betas, resids;
        if (ex) ex->begin_cycle();
        // Software pipeline of depth 1: step j+1 is enqueued BEFORE the host waits for step j's record, so the
        // GPU never idles during the host's convergence test.  If step j converges, step j+1 was speculative:
        // it only wrote Krylov row j+2, device scalars j+1 and record slot j+1, which nothing reads afterwards.
        // A step that is expected to converge is CLOSED instead (lan_expect_convergence): k_publish_record follows it, the host
        // waits for the record, and nothing further is in flight.  If it did not converge after all, step j+1 follows as an
        // ordinary non-first step -- row j+1 is raw, norm_partial holds its squared norm: the state an open step leaves -- only
        // that its matvec carries no record.
        int enq = 0;                              // steps of this cycle enqueued so far
        for (int j = 0; j < kd; ++j) {
            double tq = now_us();
            if (enq == j) {                       // the first step of the cycle, or the step behind a closed one
                if (enqueue_step(j, j == 0, false)) return 1;
                ++enq, ++nmv;
            }
            if (!closed[j]) {                     // (the last step of a cycle closed itself: j + 1 < kd here)
                if (close_mode == LAN_CLOSE_ALWAYS || (close_mode == LAN_CLOSE_AUTO && lan_expect_convergence(resids, tol))) {
                    if (publish_step(j)) return 1;
                } else {
                    if (enqueue_step(j + 1, false, true)) return 1;
                    ++enq, ++nmv;
                }
            }
            t_enq += now_us() - tq;
            double a1 = 0.0, a2 = 0.0, nn = 0.0;
            tq = now_us();
            if (wait_step(j, &a1, &a2, &nn)) return 1;
            t_wait += now_us() - tq;
            tq = now_us();
            if (timed_step[j]) {
                float ms = 0.f;
                HIP_TRY(htn_event_spin(R->ev_mv1[j]));
                HIP_TRY(hipEventElapsedTime(&ms, R->ev_mv0[j], R->ev_mv1[j]));
                mv_ms += ms;
                ++n_timed;
            }
            const double alpha = a1 + a2;
            if (!(alpha == alpha) || !(nn == nn)) return fail_msg("htn_lanczos_z: NaN in the tridiagonal coefficients (operator or start vector not finite)");
            beta = sqrt(nn > 0.0 ? nn : 0.0);
            if (ex) {
                bool bad = false;
                const bool stop = ex->step(alpha, beta, kd, &bad);
                if (bad) return fail_msg("htn_krylov_expm_z: the QL iteration of the tridiagonal matrix did not converge");
                t_host += now_us() - tq;
                if (stop) break;
                continue;
            }
            if (sv) {
                const bool stop = sv->rs.step(alpha, beta, kd);
                t_host += now_us() - tq;
                if (stop) break;
                continue;
            }
            alphas.push_back(alpha);
            tridiag_lowest(alphas, betas, &theta, y);
            res = fabs(beta * y.back());
            amax = std::max(amax, std::max(fabs(alpha), beta));
            // invariant subspace: beta negligible RELATIVE to the scale of the tridiagonal matrix
            t_host += now_us() - tq;
            const bool conv = res < tol || beta < 1e-14 * std::max(amax, 1e-300);
            if (j < kd - 1 && closed[j]) ++(conv ? g_lan_close_hit : g_lan_close_miss);
            if (j < kd - 1 && !closed[j] && conv) ++g_lan_open_conv;
            if (conv || j == kd - 1) break;
            betas.push_back(beta);
            resids.push_back(res);
        }
        if (ex) {
            // The step of this cycle in one launch.  No drain: the speculative step wrote row m + 1, the combination reads rows
            // 0 .. m - 1 and everything is ordered on the stream; its record, if it still arrives, fails the serial check.
            // INVARIANT FOR CALLERS (the eigen-solver path below has the same one): this path RETURNS with the speculative step
            // and the combination still in flight on `st`.  Whatever touches V, the scratch or the stage buffers next -- reading
            // the result, handing the blocks back to a pool, the next solve -- must be ordered on the same stream (the
            // engine's pool, relay and downloads are; torch's allocator is for its current stream) or wait for it.
            if (!ex->converged && restart == max_restart) {
                HIP_TRY(htn_stream_spin(st));
                snprintf(htn_err_buf(), 512, "htn_krylov_expm_z: not converged after %d restart(s) of krylovdim %d: fraction %.3e of dt remains "
                         "(estimate %.3e, tol %.3e)", max_restart, kd, ex->remaining, ex->est, tol);
                return 1;
            }
            if (!ex->finish()) {
                HIP_TRY(htn_stream_spin(st));
                return fail_msg("htn_krylov_expm_z: no fraction of the step down to 2^-60 meets the tolerance");
            }
            const int m = (int)ex->c.size();
            KrylovCoef kc;
            for (int i = 0; i < DOT_CHUNK; ++i) kc.c[i] = i < m ? make_double2(ex->c[i].real(), ex->c[i].imag()) : make_double2(0.0, 0.0);
            launch_krylov_combine(V, n, m, n, kc, st);
            if (ex->remaining == 0.0) break;
            continue;
        }
        if (sv) {
            // The end of this cycle in one launch (k_krylov_combine2), ordered on the stream behind the speculative step like the
            // combination of the exponential: that step wrote row m + 1, this reads rows 0 .. m.  The rows 0 .. m - 1 are unit
            // vectors; row m, read only when the cycle ran to krylovdim without converging, is the RAW vector its (closed) step left
            // behind, beta_m v_m: its coefficient carries 1 / beta_m.  The next start vector has norm |rho| by construction, so
            // the coefficients are handed over divided by it and the host knows beta_0 of the next cycle without a norm pass.
            htn_resolvent::Resolvent& rs = sv->rs;
            if (!rs.converged && restart == max_restart) {
                HIP_TRY(htn_stream_spin(st));
                snprintf(htn_err_buf(), 512, "htn_krylov_solve_z: not converged after %d restart(s) of krylovdim %d: relative residual %.3e remains "
                         "(tol %.3e)", max_restart, kd, rs.resid, rs.tol);
                return 1;
            }
            const double ynorm = rs.finish();
            const int m = (int)rs.y.size();
            const bool keep = sv->use_guess || restart > 0;
            KrylovCoef2 kc;
            for (int i = 0; i < DOT_CHUNK; ++i) {
                kc.y[i] = i < m ? make_double2(rs.y[i].real(), rs.y[i].imag()) : make_double2(0.0, 0.0);
                kc.r[i] = make_double2(0.0, 0.0);
            }
            if (rs.converged && !keep && ynorm > 0.0) {      // one cycle from zero: |x| = |y|_2, and row 0 becomes x / |x| on the way
                for (int i = 0; i < m; ++i) kc.r[i] = make_double2(rs.y[i].real() / ynorm, rs.y[i].imag() / ynorm);
                launch_krylov_combine2(V, n, m, n, sv->X, 0, 1, kc, st);
                sv->xnorm = ynorm;
                break;
            }
            if (rs.converged) {
                launch_krylov_combine2(V, n, m, n, sv->X, keep ? 1 : 0, 0, kc, st);
                if (normalise_x()) return 1;
                break;
            }
            const double rn = rs.rho_norm();
            if (!(rn > 0.0) || !(beta > 0.0)) return fail_msg("htn_krylov_solve_z: the residual of an unconverged cycle vanished");
            for (int i = 0; i <= m; ++i) {
                const double f = i == m ? 1.0 / (rn * beta) : 1.0 / rn;
                kc.r[i] = make_double2(rs.rho[i].real() * f, rs.rho[i].imag() * f);
            }
            launch_krylov_combine2(V, n, m + 1, n, sv->X, keep ? 1 : 0, 1, kc, st);
            rs.begin_cycle(rn);
            if (rs.converged) {                                  // (|rho| against the rotated residual: a tie at the tolerance)
                if (normalise_x()) return 1;
                break;
            }
            continue;
        }
        // x = sum_i y_i V_i in place in row 0, then normalised: the combine launch of the exponential with the real Ritz
        // coefficients BY VALUE -- no staging buffer, no copy, no memset, and so nothing of the host's to protect by a drain.
        // Per element it is the sum the driver used to take (from zero, i = 0 .. k - 1 in order, the imaginary part of every
        // coefficient exactly 0; the rows past k it re-reads have coefficient 0 and add +-0 to a sum that is never -0): same bits.
        // No drain in front of it either: a speculative step still in flight reads rows <= k and writes row k + 1 and the
        // scalars and record slot of its own index, in stream order BEFORE the combination; its record fails the serial check.
        // INVARIANT FOR CALLERS, as on the exponential path: this function RETURNS with that step and the three or more kernels
        // of the Ritz vector still in flight on `st`; the next restart cycle is enqueued straight behind them.  Whatever touches
        // V, the scratch, Q or the stage buffers next must be ordered on the same stream or wait for it.  (Checked: HipBackend's
        // pool, upload, download, zero and the SVD's fork are all on the context's stream and download / sync wait for it;
        // hipFree of a grown scratch synchronises the device; torch's allocator is stream-ordered for the current stream, which
        // is the one device.py passes.)
        const int k = (int)y.size();
        KrylovCoef kc;
        for (int i = 0; i < DOT_CHUNK; ++i) kc.c[i] = make_double2(i < k ? y[i] : 0.0, 0.0);
        launch_krylov_combine(V, n, k, n, kc, st);
        // (frozen rows: the Ritz vector is a combination of Krylov rows that are orthogonal to Q to rounding each; projecting
        // the sum once more keeps |Q^H x| at rounding whatever the number of rows)
        if (nf > 0) project_out(V);
        else
        hipLaunchKernelGGL(k_norm_partial, dim3(DOT_BLOCKS), dim3(DOT_THREADS), 0, st, V, n, norm_partial);
        hipLaunchKernelGGL(k_scale_by_norm, dim3(grid_for(n)), dim3(DOT_THREADS), 0, st, V, V, norm_partial, n,
                           (LanRecord*)nullptr, (const double2*)nullptr, (const double2*)nullptr, 0ull);
        if (res < tol || beta < 1e-14 * std::max(amax, 1e-300)) break;
    }
    HIP_TRY(hipGetLastError());
    if (dbg_timers)
        fprintf(stderr, "lanczos n=%lld: %d matvecs in %.1f us: enqueue %.1f, waiting for records %.1f, tridiagonal %.1f; process totals: "
                "closed steps converged %lld, not converged %lld, convergence at an open step %lld\n", (long long)n, nmv,
                now_us() - t_begin, t_enq, t_wait, t_host, g_lan_close_hit.load(), g_lan_close_miss.load(), g_lan_open_conv.load());
    *eig_host = ex ? ex->alpha0 : theta;
    *n_matvec_host = nmv;
    *residual_host = ex ? ex->err_total : sv ? sv->rs.resid : res;
    // sampled launches scaled to all launches of this solve (the next solves continue the 1-in-8 sampling phase)
    if (matvec_ms_host) *matvec_ms_host = n_timed ? mv_ms * nmv / n_timed : -1.0;
    return 0;
}

extern "C" int htn_lanczos_z(const htn_gemm_launch* stages, int32_t n_stages, int32_t x_slot, int32_t y_slot,
                             void* Vv, int64_t n, int32_t krylovdim, double tol, int32_t max_restart,
                             void* scratch, int32_t zero_y, htn_exchange2_fn exchange, void* user,
                             double* eig_host, int32_t* n_matvec_host, double* residual_host,
                             double* matvec_ms_host, void* stream_v) {
    // (k_axpy_dots keeps one basis value per Krylov vector in registers: at most DOT_CHUNK = 32 vectors per step)
    if (krylovdim < 2 || krylovdim + 1 > DOT_CHUNK) return fail_msg("htn_lanczos_z: krylovdim must be in 2..31");
    return lanczos_run(stages, n_stages, x_slot, y_slot, Vv, n, krylovdim, tol, max_restart, scratch, zero_y, exchange, user,
                       eig_host, n_matvec_host, residual_host, matvec_ms_host, stream_v, nullptr, 0);
}

extern "C" int htn_lanczos_orth_z(const htn_gemm_launch* stages, int32_t n_stages, int32_t x_slot, int32_t y_slot,
                                  void* Vv, int64_t n, int32_t krylovdim, double tol, int32_t max_restart,
                                  void* scratch, int32_t zero_y, htn_exchange2_fn exchange, void* user,
                                  double* eig_host, int32_t* n_matvec_host, double* residual_host,
                                  double* matvec_ms_host, const void* Q, int32_t n_frozen, void* stream_v) {
    // (the frozen rows sit in the same registers as the Krylov rows: one basis value per row, DOT_CHUNK = 32 rows per pass)
    if (n_frozen < 0 || (n_frozen > 0 && !Q)) return fail_msg("htn_lanczos_orth_z: n_frozen rows need a device pointer Q");
    if (krylovdim < 2 || krylovdim + n_frozen + 1 > DOT_CHUNK)
        return fail_msg("htn_lanczos_orth_z: krylovdim >= 2 and krylovdim + n_frozen <= 31 required");
    return lanczos_run(stages, n_stages, x_slot, y_slot, Vv, n, krylovdim, tol, max_restart, scratch, zero_y, exchange, user,
                       eig_host, n_matvec_host, residual_host, matvec_ms_host, stream_v, (const double2*)Q, n_frozen);
}

// V[0] <- sum_i coef[i] V[i] in place (hubbardtn_hip.h): the combine launch on its own
extern "C" int htn_krylov_combine_z(void* V, int64_t ldv, int32_t nvec, const double* coef_host, int64_t n, void* stream) {
    if (nvec < 1 || nvec > DOT_CHUNK) return fail_msg("htn_krylov_combine_z: nvec must be in 1..32");
    if (!V || !coef_host || n < 0 || ldv < n) return fail_msg("htn_krylov_combine_z: bad arguments (V, coef_host, 0 <= n <= ldv)");
    if (n == 0) return 0;
    KrylovCoef kc;
    for (int i = 0; i < DOT_CHUNK; ++i) kc.c[i] = i < nvec ? make_double2(coef_host[2 * i], coef_host[2 * i + 1]) : make_double2(0.0, 0.0);
    launch_krylov_combine((double2*)V, ldv, nvec, n, kc, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// x = exp(-i dt H) x0 through the basis lanczos_run builds (hubbardtn_hip.h; the host decisions are htn_expm::Expm's)
extern "C" int htn_krylov_expm_z(const htn_gemm_launch* stages, int32_t n_stages, int32_t x_slot, int32_t y_slot, void* Vv, int64_t n,
                                 int32_t krylovdim, double dt_re, double dt_im, double tol, int32_t max_restart, void* scratch,
                                 int32_t zero_y, htn_exchange2_fn exchange, void* user, double* growth_host, double* alpha0_host,
                                 int32_t* n_matvec_host, double* err_host, double* matvec_ms_host, void* stream_v) {
    if (krylovdim < 2 || krylovdim + 1 > DOT_CHUNK) return fail_msg("htn_krylov_expm_z: krylovdim must be in 2..31");
    if (!Vv || !scratch || n <= 0 || !growth_host || !alpha0_host || !n_matvec_host || !err_host) return fail_msg("htn_krylov_expm_z: bad arguments");
    if (!(dt_re == dt_re) || !(dt_im == dt_im) || !(tol >= 0.0)) return fail_msg("htn_krylov_expm_z: dt and tol must be finite, tol >= 0");
    htn_expm::Expm ex;
    ex.dt_re = dt_re, ex.dt_im = dt_im, ex.tol = tol;
    double a0 = 0.0, err = 0.0;
    if (lanczos_run(stages, n_stages, x_slot, y_slot, Vv, n, krylovdim, tol, max_restart < 0 ? 0 : max_restart, scratch, zero_y, exchange,
                    user, &a0, n_matvec_host, &err, matvec_ms_host, stream_v, nullptr, 0, &ex))
        return 1;
    *growth_host = ex.growth;
    *alpha0_host = a0;
    *err_host = err;
    return 0;
}

// X <- (keep ? X : 0) + sum_{i < m} y[i] V[i] and, with rho, V[0] <- sum_{i <= m} rho[i] V[i] (hubbardtn_hip.h): the launch on its own
extern "C" int htn_krylov_combine2_z(void* V, int64_t ldv, int32_t m, const double* y_host, const double* rho_host, void* X, int32_t keep,
                                     int64_t n, void* stream) {
    if (m < 1 || m + 1 > DOT_CHUNK) return fail_msg("htn_krylov_combine2_z: m must be in 1..31");
    if (!V || !X || !y_host || n < 0 || ldv < n) return fail_msg("htn_krylov_combine2_z: bad arguments (V, X, y_host, 0 <= n <= ldv)");
    if (n == 0) return 0;
    KrylovCoef2 kc;
    for (int i = 0; i < DOT_CHUNK; ++i) {
        kc.y[i] = i < m ? make_double2(y_host[2 * i], y_host[2 * i + 1]) : make_double2(0.0, 0.0);
        kc.r[i] = rho_host && i <= m ? make_double2(rho_host[2 * i], rho_host[2 * i + 1]) : make_double2(0.0, 0.0);
    }
    launch_krylov_combine2((double2*)V, ldv, rho_host ? m + 1 : m, n, (double2*)X, keep ? 1 : 0, rho_host ? 1 : 0, kc, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// (z - H) x = b by the restarted minimal residual on the basis lanczos_run builds (hubbardtn_hip.h; the host decisions are
// htn_resolvent::Resolvent's)
extern "C" int htn_krylov_solve_z(const htn_gemm_launch* stages, int32_t n_stages, int32_t x_slot, int32_t y_slot, void* Vv, int64_t n,
                                  int32_t krylovdim, double z_re, double z_im, double tol, int32_t max_restart, void* X, int32_t use_guess,
                                  void* scratch, int32_t zero_y, htn_exchange2_fn exchange, void* user, double* norm_host,
                                  double* residual_host, int32_t* n_matvec_host, double* matvec_ms_host, void* stream_v) {
    if (krylovdim < 2 || krylovdim + 1 > DOT_CHUNK) return fail_msg("htn_krylov_solve_z: krylovdim must be in 2..31");
    if (!Vv || !X || !scratch || n <= 0 || !norm_host || !residual_host || !n_matvec_host) return fail_msg("htn_krylov_solve_z: bad arguments");
    if (!(z_re - z_re == 0.0) || !(z_im - z_im == 0.0) || !(tol >= 0.0)) return fail_msg("htn_krylov_solve_z: z must be finite, tol >= 0");
    SolveHook sv;
    sv.rs.z = htn_resolvent::cplx(z_re, z_im), sv.rs.tol = tol;
    sv.X = (double2*)X, sv.use_guess = use_guess != 0;
    double unused = 0.0;
    if (lanczos_run(stages, n_stages, x_slot, y_slot, Vv, n, krylovdim, tol, max_restart < 0 ? 0 : max_restart, scratch, zero_y, exchange,
                    user, &unused, n_matvec_host, residual_host, matvec_ms_host, stream_v, nullptr, 0, nullptr, &sv))
        return 1;
    *norm_host = sv.xnorm;
    return 0;
}
