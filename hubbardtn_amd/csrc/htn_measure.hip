// Batched block trace-dots (htn_block_trdots_z): out[o] = sum_items w * sum_{r,c} A[r, c] * B[c, r].
// The contraction that closes a two-point correlation function on a bond: a left environment block [n_bra x n_ket] against a
// right environment block [n_ket x n_bra] (htn_mps::corr_pass in htn_correlator.cpp).
//
// Memory-bound: every element of both operands is read once, so both must be read along their contiguous (column) direction.
// An item is cut into 32 x 32 tiles of A.  A workgroup of 256 threads reads the A tile column by column straight into
// registers (32 consecutive complex128 = 512 B per 32 lanes) and the matching B tile -- 32 x 32 of the cols x rows block --
// column by column into LDS, then every thread picks the four transposed partners of its A values out of LDS.  The LDS image
// has a row pitch of 33 elements: thread (r, c) reads element [r][c], 16 lanes with consecutive r land 33 * 4 dwords apart,
// i.e. on 16 different 4-dword bank groups of the 64 banks -- conflict-free for the 16-lane groups of ds_read_b128.  Two images
// alternate, so a tile costs one barrier.
//
// Deterministic, two stages, no atomics.  Stage 1: item q owns HTN_TRDOT_SLOTS work units; unit s adds the tiles s, s + SLOTS,
// ... of its item in that order (thread-private sums over the tiles, then the fixed wave_sum tree and the four wave sums in wave
// order) and stores ONE partial; the units are dealt round-robin to the workgroups of the launch, so a large block is shared by
// up to SLOTS workgroups and the few hundred small items of a normal launch fill the device.  Stage 2: one workgroup per result
// adds, per item of that result, the item's non-empty slots in slot order, times the weight, and the items in list order.
#include <algorithm>

#include "htn_common.h"

namespace {

constexpr int TD = 32;               // tile edge
constexpr int TD_PITCH = TD + 1;     // LDS row pitch (elements)
constexpr int TD_THREADS = 256;
constexpr int SLOTS = HTN_TRDOT_SLOTS;
static_assert(sizeof(htn_trdot_item) == 64, "htn_trdot_item is a 64-byte record");

__device__ __forceinline__ int tiles_of(const htn_trdot_item& it) {
    if (it.rows <= 0 || it.cols <= 0) return 0;
    return ((it.rows + TD - 1) / TD) * ((it.cols + TD - 1) / TD);
}

__global__ __launch_bounds__(TD_THREADS) void k_trdots_partial(const double2* __restrict__ A, const double2* __restrict__ B,
                                                                const htn_trdot_item* __restrict__ items, int n_items,
                                                                double2* __restrict__ partial) {
    __shared__ double2 sB[2][TD * TD_PITCH];
    __shared__ double wsum[2][TD_THREADS / 64];
    const int tid = threadIdx.x, lx = tid & (TD - 1), ly = tid >> 5;      // ly = 0..7
    const int n_units = n_items * SLOTS;
    for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
        const htn_trdot_item it = items[u / SLOTS];
        const int s = u % SLOTS;
        const int nt = tiles_of(it);
        if (s >= nt) continue;               // (uniform over the workgroup; stage 2 reads the first min(SLOTS, nt) slots only)
        const int ntr = (it.rows + TD - 1) / TD;
        const double2* __restrict__ Ab = A + it.a_off;
        const double2* __restrict__ Bb = B + it.b_off;
        double acc_re = 0.0, acc_im = 0.0;
        int buf = 0;
        for (int t = s; t < nt; t += SLOTS, buf ^= 1) {
            const int r0 = (t % ntr) * TD, c0 = (t / ntr) * TD;           // down the rows of A first
            double2 a[4], b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = ly + 8 * k;
                // A tile element (r0 + lx, c0 + c): lanes run down a column of A
                a[k] = (r0 + lx < it.rows && c0 + c < it.cols) ? Ab[(int64_t)(r0 + lx) + (int64_t)(c0 + c) * it.lda] : make_double2(0.0, 0.0);
                // B block is cols x rows: element (c0 + lx, r0 + c), lanes run down a column of B
                b[k] = (c0 + lx < it.cols && r0 + c < it.rows) ? Bb[(int64_t)(c0 + lx) + (int64_t)(r0 + c) * it.ldb] : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) sB[buf][(ly + 8 * k) * TD_PITCH + lx] = b[k];      // image[r local][c local]
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double2 y = sB[buf][lx * TD_PITCH + ly + 8 * k];                     // B[c0 + c, r0 + lx]
                acc_re += a[k].x * y.x - a[k].y * y.y;
                acc_im += a[k].x * y.y + a[k].y * y.x;
            }
            // the next tile writes the other image; the one after it writes this one again, behind that tile's barrier
        }
        const double wr = wave_sum(acc_re), wi = wave_sum(acc_im);
        __syncthreads();                     // the previous unit's readers of wsum are done
        if ((tid & 63) == 0) wsum[0][tid >> 6] = wr, wsum[1][tid >> 6] = wi;
        __syncthreads();
        if (tid == 0) {
            double re = 0.0, im = 0.0;
            for (int w = 0; w < TD_THREADS / 64; ++w) re += wsum[0][w], im += wsum[1][w];
            partial[u] = make_double2(re, im);
        }
    }
}

// one workgroup per result: the threads gather the items' weighted sums chunk by chunk, thread 0 adds them in list order
__global__ __launch_bounds__(TD_THREADS) void k_trdots_reduce(const htn_trdot_item* __restrict__ items, int n_items,
                                                               const double2* __restrict__ partial, double2* __restrict__ out) {
    __shared__ double2 val[TD_THREADS];
    __shared__ int hit[TD_THREADS];
    const int o = blockIdx.x, tid = threadIdx.x;
    double re = 0.0, im = 0.0;
    for (int q0 = 0; q0 < n_items; q0 += TD_THREADS) {
        const int q = q0 + tid;
        int mine = 0;
        double2 v = make_double2(0.0, 0.0);
        if (q < n_items) {
            const htn_trdot_item it = items[q];
            if (it.out == o) {
                mine = 1;
                const int ns = min(SLOTS, tiles_of(it));
                double sr = 0.0, si = 0.0;
                for (int s = 0; s < ns; ++s) {
                    const double2 p = partial[(int64_t)q * SLOTS + s];
                    sr += p.x, si += p.y;
                }
                v = make_double2(it.w_re * sr - it.w_im * si, it.w_re * si + it.w_im * sr);
            }
        }
        val[tid] = v;
        hit[tid] = mine;
        __syncthreads();
        if (tid == 0) {
            const int n = min(TD_THREADS, n_items - q0);
            for (int k = 0; k < n; ++k)
                if (hit[k]) re += val[k].x, im += val[k].y;
        }
        __syncthreads();
    }
    if (tid == 0) out[o] = make_double2(re, im);
}

}  // namespace

extern "C" int64_t htn_trdots_scratch_elems(int32_t n_items) { return (int64_t)(n_items > 0 ? n_items : 0) * SLOTS + 1; }

extern "C" int htn_block_trdots_z(const void* A, const void* B, const htn_trdot_item* items, int32_t n_items, void* out,
                                  int32_t n_out, void* scratch, void* stream) {
    if (n_items < 0 || n_out < 0) return fail_msg("htn_block_trdots_z: negative count");
    if (n_out == 0) return 0;
    if (!out || (n_items > 0 && (!A || !B || !items || !scratch))) return fail_msg("htn_block_trdots_z: NULL argument");
    if ((int64_t)n_items * SLOTS > INT32_MAX) return fail_msg("htn_block_trdots_z: too many items");
    hipStream_t st = (hipStream_t)stream;
    if (n_items > 0) {
        const int grid = (int)std::min<int64_t>((int64_t)n_items * SLOTS, 2048);
        hipLaunchKernelGGL(k_trdots_partial, dim3(grid), dim3(TD_THREADS), 0, st, (const double2*)A, (const double2*)B, items, n_items,
                           (double2*)scratch);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_trdots_reduce, dim3(n_out), dim3(TD_THREADS), 0, st, items, n_items, (const double2*)scratch, (double2*)out);
    HIP_TRY(hipGetLastError());
    return 0;
}
