// batched strided copy / gather / scale, compiled into htn_svd.hip's translation unit
#pragma once

// ----------------------------------------------------------------------------------------------
// batched strided copy / gather / scale
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_batched_copy(double2* __restrict__ dst, const double2* __restrict__ src,
                                                      const int32_t* __restrict__ idx,
                                                      const double* __restrict__ scl,
                                                      const htn_copy_item* __restrict__ items, double gscale) {
    // grid = (items, COPY_SPLIT): the largest item (a 200 x 250 block) would otherwise occupy ONE workgroup for
    // ~80 us while the other CUs idle; the element range of every item is dealt over gridDim.y workgroups
    const htn_copy_item I = items[blockIdx.x];
    const int total = I.rows * I.cols;
    for (int e = blockIdx.y * blockDim.x + threadIdx.x; e < total; e += blockDim.x * gridDim.y) {
        const int i = e % I.rows, j = e / I.rows;
        // gathered source index along gather_dim of dst
        int gi = i, gj = j;
        if (I.idx_off >= 0) {
            if (I.gather_dim == 0) gi = idx[I.idx_off + i];
            else gj = idx[I.idx_off + j];
        }
        double2 v;
        if (I.op == HTN_OP_N) v = src[I.src_off + (int64_t)gi + (int64_t)gj * I.lds];
        else {
            v = src[I.src_off + (int64_t)gj + (int64_t)gi * I.lds];   // dst(i,j) = conj(src(gj, gi))
            v.y = -v.y;
        }
        double f = gscale;
        if (I.scale_dim >= 0 && I.scl_off >= 0) {
            const double sv = scl[I.scl_off + (I.scale_dim == 0 ? gi : gj)];
            f = I.inv_norm ? (sv > 0.0 ? f / sv : 0.0) : f * sv;
        }
        dst[I.dst_off + (int64_t)i + (int64_t)j * I.ldd] = make_double2(v.x * f, v.y * f);
    }
}

extern "C" int htn_batched_copy_z(void* dst, const void* src, const int32_t* idx, const double* scl,
                                  const htn_copy_item* items, int32_t n_items, double global_scale,
                                  void* stream) {
    if (n_items <= 0) return 0;
    hipLaunchKernelGGL(k_batched_copy, dim3(n_items, 16), dim3(256), 0, (hipStream_t)stream, (double2*)dst,
                       (const double2*)src, idx, scl, items, global_scale);
    HIP_TRY(hipGetLastError());
    return 0;
}
