// Jacobi SVD, piece of htn_svd.hip: k_jacobi_svd, the whole SVD of one block in one workgroup
#pragma once

__global__ __launch_bounds__(JAC_THREADS) void k_jacobi_svd(double2* __restrict__ G, double2* __restrict__ Vj,
                                                            double* __restrict__ S,
                                                            const htn_svd_block* __restrict__ desc,
                                                            int max_sweeps, double tol, int* __restrict__ info,
                                                            int lds_elems, const int* __restrict__ large_slot,
                                                            double cut2) {
    extern __shared__ double2 g_lds[];
    __shared__ double s_ratio[2];      // |G|_F^2 first; then per sweep: largest squared cosine seen | largest tan^2 rotated by
    __shared__ double s_piv[2];
    __shared__ int s_col[64 * JAC_MAXEL];
    __shared__ double s_cn2[64 * JAC_MAXEL];
    if (large_slot && large_slot[blockIdx.x] >= 0) return;      // k_qr_large + block Jacobi own this block
    const htn_svd_block D = desc[blockIdx.x];
    const int m = D.m, n = D.n;
    double2* __restrict__ gglob = G + D.g_off;
    double2* __restrict__ v = Vj + D.v_off;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nwaves = JAC_THREADS / 64;
    const bool in_lds = (int64_t)m * n <= lds_elems;
    const bool accumulate = (D.flags & HTN_SVD_ACCUMULATE) != 0;
    const bool qrcp = (D.flags & HTN_SVD_QRCP) != 0;
    double2* g;
    if (qrcp) {
        // G0 (m0 x n0 = D.pad x D.m) at gglob; X = R^H (n0 x r = m x n), leading dimension mp = GS * E (zero padded),
        // in LDS when it fits, else in the Vj workspace (the planner reserves roundup(m, 64) * n elements there)
        const int m0 = D.pad;
        const int gsx = m <= 16 * JAC_MAXEL ? 16 : (m <= 32 * JAC_MAXEL ? 32 : 64);
        const int E = (m + gsx - 1) / gsx;
        const int mp = gsx * E;
        // (keeping only the leading columns in LDS and the rest in global memory was measured SLOWER than
        // all-global: the mixed case needs flat addressing, 4.4 ms vs 3.1 ms for a 107 x 107 block)
        const bool x_lds = (int64_t)mp * n <= lds_elems;
        const int nl = x_lds ? n : 0;
        const SplitCols X = {(double2*)g_lds, v, nl, mp};
        int rank;                 // columns of X the sweeps have to visit (the others are zero)
        if (m0 <= 16 * JAC_MAXEL) rank = qrcp_mgs<16>(gglob, m0, m, n, X, s_col, s_cn2, s_piv, tid, cut2);
        else if (m0 <= 32 * JAC_MAXEL) rank = qrcp_mgs<32>(gglob, m0, m, n, X, s_col, s_cn2, s_piv, tid, cut2);
        else rank = qrcp_mgs<64>(gglob, m0, m, n, X, s_col, s_cn2, s_piv, tid, cut2);
        {   // |X|_F^2 -> threshold for "numerically zero" columns
            double f = 0.0;
            for (int idx = tid; idx < mp * n; idx += JAC_THREADS) {
                const double2 x = X.col(idx / mp)[idx % mp];
                f += x.x * x.x + x.y * x.y;
            }
            f = wave_sum(f);
            if (lane == 0) s_cn2[wave] = f;          // fixed-order sum over the 16 waves: bit-reproducible
            __syncthreads();
            if (tid == 0) {
                double t = 0.0;
                for (int q = 0; q < JAC_THREADS / 64; ++q) t += s_cn2[q];
                s_ratio[0] = t;
            }
            __syncthreads();
        }
        const double zero2q = 1e-30 * s_ratio[0];
        __syncthreads();
        int swq;
        if (x_lds) {        // everything in LDS: ds_* addressing
            const DenseCols<double2*> dc = {(double2*)g_lds, mp};
            if (gsx == 16) swq = jacobi_dispatch_e<16>(dc, E, rank, max_sweeps, tol, s_ratio, tid, zero2q);
            else if (gsx == 32) swq = jacobi_dispatch_e<32>(dc, E, rank, max_sweeps, tol, s_ratio, tid, zero2q);
            else swq = jacobi_dispatch_e<64>(dc, E, rank, max_sweeps, tol, s_ratio, tid, zero2q);
        } else {            // everything in global memory (L2 resident): global_* addressing
            const DenseCols<double2*> dc = {v, mp};
            if (gsx == 16) swq = jacobi_dispatch_e<16>(dc, E, rank, max_sweeps, tol, s_ratio, tid, zero2q);
            else if (gsx == 32) swq = jacobi_dispatch_e<32>(dc, E, rank, max_sweeps, tol, s_ratio, tid, zero2q);
            else swq = jacobi_dispatch_e<64>(dc, E, rank, max_sweeps, tol, s_ratio, tid, zero2q);
        }
        __syncthreads();
        // column norms + write back with the pivoting undone: row k of X is row s_col[k] of the result
        for (int j = wave; j < n; j += nwaves) {
            double sn = 0.0;
            for (int i = lane; i < m; i += 64) {
                const double2 x = X.col(j)[i];
                sn += x.x * x.x + x.y * x.y;
                gglob[(int64_t)j * m + s_col[i]] = x;
            }
            sn = wave_sum(sn);
            if (lane == 0) S[D.s_off + j] = sqrt(sn);
        }
        if (tid == 0) info[blockIdx.x] = swq;
        return;
    } else {
        // V = identity ; stage G into LDS when it fits
        if (accumulate)
            for (int idx = tid; idx < n * n; idx += JAC_THREADS) {
                const int i = idx % n, j = idx / n;
                v[idx] = make_double2(i == j ? 1.0 : 0.0, 0.0);
            }
        if (in_lds)
            for (int idx = tid; idx < m * n; idx += JAC_THREADS) g_lds[idx] = gglob[idx];
        __syncthreads();
        g = in_lds ? (double2*)g_lds : gglob;
    }
    // |G|_F^2 -> threshold for "numerically zero" columns
    {
        double f = 0.0;
        for (int idx = tid; idx < m * n; idx += JAC_THREADS) {
            const double2 x = g[idx];
            f += x.x * x.x + x.y * x.y;
        }
        f = wave_sum(f);
        if (lane == 0) s_cn2[wave] = f;              // fixed-order sum over the 16 waves: bit-reproducible
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int q = 0; q < JAC_THREADS / 64; ++q) t += s_cn2[q];
            s_ratio[0] = t;
        }
        __syncthreads();
    }
    const double zero2 = 1e-30 * s_ratio[0];
    __syncthreads();
    int sw;
    if (m <= 16 * JAC_MAXEL) sw = jacobi_sweeps<16>(g, v, m, n, max_sweeps, tol, s_ratio, tid, accumulate, zero2);
    else if (m <= 32 * JAC_MAXEL) sw = jacobi_sweeps<32>(g, v, m, n, max_sweeps, tol, s_ratio, tid, accumulate, zero2);
    else sw = jacobi_sweeps<64>(g, v, m, n, max_sweeps, tol, s_ratio, tid, accumulate, zero2);
    __syncthreads();
    // column norms (+ write back; the QR path undoes the pivoting: row k of X is row s_col[k] of the result)
    for (int j = wave; j < n; j += nwaves) {
        double s = 0.0;
        for (int i = lane; i < m; i += 64) {
            const double2 x = g[(int64_t)j * m + i];
            s += x.x * x.x + x.y * x.y;
            if (in_lds) gglob[(int64_t)j * m + i] = x;
        }
        s = wave_sum(s);
        if (lane == 0) S[D.s_off + j] = sqrt(s);
    }
    if (tid == 0) info[blockIdx.x] = sw;
}
