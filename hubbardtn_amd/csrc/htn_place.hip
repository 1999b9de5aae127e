// Block placement (htn_block_place_z): dst[dst_off + r + c*ldd] = coef * src[src_off + r + c*lds] per item, or zeros for an
// item without a source (src_off = -1).  Builds the site tensors of an MPS a local operator was applied to
// (htn_mps_apply_op / htn_mps_transition in htn_applyop.cpp): every block of the new tensor is a block of the old one times a
// real recoupling coefficient, placed into a sub-block of a larger block, and the sub-blocks nothing maps to are zero.  The
// items of one launch tile their destination exactly once, so no memset precedes it.
//
// Memory-bound: 16 bytes read and 16 written per element.  Items are cut into PT x PT tiles; all tiles of the launch are
// numbered item after item and dealt round-robin to the workgroups, so one large block is shared by the whole launch and a
// thousand 1 x 1 blocks cost a thousand tiles, not a thousand workgroups.  The item list lives on the device only, so every
// workgroup walks it itself: 256 records at a time are staged in LDS with coalesced 16-byte loads and the running tile number
// is advanced from there (a few scalar instructions per item).  Inside a tile 32 consecutive lanes run down a column (512
// contiguous bytes), one global_load_dwordx4 and one global_store_dwordx4 per element.
// No atomics: every destination element is written by exactly one thread of one workgroup; repeated calls are bit-identical.
#include <algorithm>

#include "htn_common.h"

namespace {

constexpr int PT = 32;               // tile edge
constexpr int PL_THREADS = 256;
constexpr int PL_STAGE = 256;        // item records staged in LDS at a time (16 KiB)
static_assert(sizeof(htn_place_item) == 64, "htn_place_item is a 64-byte record");

__global__ __launch_bounds__(PL_THREADS) void k_block_place(double2* __restrict__ dst, const double2* __restrict__ src,
                                                            const htn_place_item* __restrict__ items, int n_items) {
    __shared__ htn_place_item sI[PL_STAGE];
    const int tid = threadIdx.x, lx = tid & (PT - 1), ly = tid >> 5;      // ly = 0..7
    const int64_t G = gridDim.x;
    int64_t base = 0;                                                     // number of the first tile of the current item
    for (int q0 = 0; q0 < n_items; q0 += PL_STAGE) {
        const int nq = min(PL_STAGE, n_items - q0);
        __syncthreads();                                                  // the previous chunk's readers are done
        {
            const int4* __restrict__ g = (const int4*)(items + q0);
            int4* s = (int4*)sI;
            for (int w = tid; w < nq * 4; w += PL_THREADS) s[w] = g[w];
        }
        __syncthreads();
        for (int k = 0; k < nq; ++k) {
            const int rows = sI[k].rows, cols = sI[k].cols;
            if (rows <= 0 || cols <= 0) continue;
            const int ntr = (rows + PT - 1) / PT;
            const int64_t nt = (int64_t)ntr * ((cols + PT - 1) / PT);
            // tiles t of this item with (base + t) % G == blockIdx.x
            int64_t t = ((int64_t)blockIdx.x - base % G + G) % G;
            base += nt;
            if (t >= nt) continue;
            const int64_t d_off = sI[k].dst_off, s_off = sI[k].src_off;
            const int ldd = sI[k].ldd, lds = sI[k].lds;
            const double coef = sI[k].coef;
            for (; t < nt; t += G) {
                const int r = (int)(t % ntr) * PT + lx, c0 = (int)(t / ntr) * PT;
                if (r >= rows) continue;
#pragma unroll
                for (int p = 0; p < PT / 8; ++p) {
                    const int c = c0 + ly + 8 * p;
                    if (c >= cols) break;
                    double2 v = make_double2(0.0, 0.0);
                    if (s_off >= 0) {
                        const double2 x = src[s_off + (int64_t)r + (int64_t)c * lds];
                        v = make_double2(coef * x.x, coef * x.y);
                    }
                    dst[d_off + (int64_t)r + (int64_t)c * ldd] = v;
                }
            }
        }
    }
}

}  // namespace

extern "C" int htn_block_place_z(void* dst, const void* src, const htn_place_item* items, int32_t n_items, void* stream) {
    if (n_items < 0) return fail_msg("htn_block_place_z: negative count");
    if (n_items == 0) return 0;
    if (!dst || !items) return fail_msg("htn_block_place_z: NULL argument");
    // the sizes are on the device: a launch of up to 1024 workgroups (four per CU) takes whatever tiles there are; a workgroup
    // without a tile walks the list and leaves
    const int grid = (int)std::min<int64_t>((int64_t)n_items * 64, 1024);
    hipLaunchKernelGGL(k_block_place, dim3(grid), dim3(PL_THREADS), 0, (hipStream_t)stream, (double2*)dst, (const double2*)src, items, n_items);
    HIP_TRY(hipGetLastError());
    return 0;
}
