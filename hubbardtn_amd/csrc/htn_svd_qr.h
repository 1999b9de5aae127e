// Jacobi SVD, piece of htn_svd.hip: pivoted QR preconditioner -- MGS QRCP (blocks in LDS), panel-blocked QRCP and k_qr_large
#pragma once

// ---- QR with column pivoting (modified Gram-Schmidt, R only) ---------------------------------------
// Preconditioner of Drmac-Veselic type: G0 P = Q R, then Jacobi runs on X = R^H whose columns are graded
// by the pivoting, which cuts the sweep count from ~18 to a few on Schmidt-type (graded) spectra.  Q is
// never needed: G0 = (Q J) Sigma (P W)^H, and P W -- the normalised Jacobi output with its rows permuted
// back -- is exactly the isometry the caller asked for (it staged G0 = M^H or M accordingly).
// Columns are not swapped physically: s_col[k] is the physical column of logical position k.
template <int GS>
__device__ __forceinline__ int qrcp_mgs(double2* __restrict__ g0, int m0, int n0, int r, const SplitCols X,
                                        int* s_col, double* s_cn2, double* s_piv, int tid, double cut2) {
    const int grp = tid / GS, sub = tid % GS, lane = tid & 63, wave = tid >> 6;
    const int ngroups = JAC_THREADS / GS;
    for (int idx = tid; idx < X.mp * r; idx += JAC_THREADS) X.col(idx / X.mp)[idx % X.mp] = make_double2(0.0, 0.0);
    for (int k = grp; k < n0; k += ngroups) {
        double c = 0.0;
        for (int i = sub; i < m0; i += GS) {
            const double2 x = g0[(int64_t)k * m0 + i];
            c += x.x * x.x + x.y * x.y;
        }
        c = group_sum<GS>(c);
        if (sub == 0) {
            s_cn2[k] = c;
            s_col[k] = k;
        }
    }
    __syncthreads();
    if (wave == 0) {
        double f = 0.0;
        for (int k = lane; k < n0; k += 64) f += s_cn2[k];
        f = wave_sum(f);
        if (lane == 0) s_piv[1] = 1e-30 * f;       // "numerically zero" threshold on squared norms
    }
    __syncthreads();
    const double zero2 = s_piv[1];
    int rank = 0;
    for (int j = 0; j < r; ++j) {
        if (wave == 0) {                            // pivot = remaining column of largest norm
            double best = -1.0, mass = 0.0;
            int bi = j;
            for (int k = j + lane; k < n0; k += 64) {
                mass += s_cn2[k];                   // |R22|_F^2: bounds every remaining singular value (rank cut)
                if (s_cn2[k] > best) {
                    best = s_cn2[k];
                    bi = k;
                }
            }
            mass = wave_sum(mass);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ob = __shfl_xor(best, off, 64);
                const int oi = __shfl_xor(bi, off, 64);
                if (ob > best || (ob == best && oi < bi)) {
                    best = ob;
                    bi = oi;
                }
            }
            if (bi != j)                             // the finished part of R moves with its column
                for (int jj = lane; jj < j; jj += 64) {
                    double2* xc = X.col(jj);
                    const double2 t = xc[j];
                    xc[j] = xc[bi];
                    xc[bi] = t;
                }
            if (lane == 0) {
                const int t = s_col[j];
                s_col[j] = s_col[bi];
                s_col[bi] = t;
                s_cn2[bi] = s_cn2[j];
                s_cn2[j] = best;
                s_piv[0] = mass <= cut2 ? 0.0 : best;
            }
        }
        __syncthreads();
        if (s_piv[0] <= zero2) break;               // numerically rank deficient: remaining R rows are zero
        rank = j + 1;
        const double2* __restrict__ p = g0 + (int64_t)s_col[j] * m0;
        for (int k = j + grp; k < n0; k += ngroups) {
            // every group recomputes |p|^2 itself (bitwise identical everywhere): no normalisation pass
            double2 pv[JAC_MAXEL], av[JAC_MAXEL];
            double pp = 0.0, dr = 0.0, di = 0.0;
            double2* __restrict__ a = g0 + (int64_t)s_col[k] * m0;
#pragma unroll
            for (int e = 0; e < JAC_MAXEL; ++e) {
                const int i = sub + GS * e;
                if (i < m0) {
                    pv[e] = p[i];
                    pp += pv[e].x * pv[e].x + pv[e].y * pv[e].y;
                    if (k > j) {
                        av[e] = a[i];
                        dr += pv[e].x * av[e].x + pv[e].y * av[e].y;      // conj(p) * a
                        di += pv[e].x * av[e].y - pv[e].y * av[e].x;
                    }
                }
            }
            pp = group_sum<GS>(pp);
            const double pn = sqrt(pp);
            if (k == j) {
                if (sub == 0) X.col(j)[j] = make_double2(pn, 0.0);
                continue;
            }
            dr = group_sum<GS>(dr);
            di = group_sum<GS>(di);
            const double fr = dr / pp, fi = di / pp;      // (p^H a) / |p|^2
            double c = 0.0;
#pragma unroll
            for (int e = 0; e < JAC_MAXEL; ++e) {
                const int i = sub + GS * e;
                if (i < m0) {
                    const double2 x = make_double2(av[e].x - (fr * pv[e].x - fi * pv[e].y),
                                                   av[e].y - (fr * pv[e].y + fi * pv[e].x));
                    a[i] = x;
                    c += x.x * x.x + x.y * x.y;
                }
            }
            c = group_sum<GS>(c);
            if (sub == 0) {
                s_cn2[k] = c;
                X.col(j)[k] = make_double2(dr / pn, -di / pn);   // conj(r_jk), r_jk = q^H a
            }
        }
        __syncthreads();
    }
    __syncthreads();
    return rank;
}

// workgroup barrier that orders LDS traffic only (__syncthreads() also drains the vector-memory queue; the
// panel loop below issues global stores of R entries in every step that nobody reads before the kernel ends)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- panel-blocked pivoted QR for blocks that live in global memory ---------------------------------
// qrcp_mgs above streams the whole trailing matrix through one CU once per COLUMN (268 MB for a 256 x 256
// block: 3.8 ms at the ~70 GB/s one CU gets out of L2).  Here the trailing matrix is touched once per PANEL
// of 16 columns:
//   (a) window pivoting: the 16 remaining columns of largest (exactly recomputed) norm form the panel;
//   (b) panel factorisation: one wave owns one panel column IN REGISTERS; 16 steps of modified Gram-Schmidt
//       with greedy pivoting inside the panel, the pivot column broadcast through LDS; a pivot whose norm
//       fell by more than 100x inside the panel is projected a second time ("twice is enough"), so the
//       panel basis Q_p is orthonormal to rounding and (I - Q_p Q_p^H) below is a projector;
//   (c) trailing update, one wave per chunk of 16 columns, on v_mfma_f64_16x16x4_f64:
//       C = Q_p^H A (rows of R), A <- A - Q_p C, new column norms recomputed from the updated columns.
// Between panels this is block MODIFIED Gram-Schmidt (every panel sees the updated trailing matrix), whose
// R factor is backward stable like that of column MGS.  R entries are stored by PHYSICAL column index
// (X[j][phys k] = conj(r_jk)), so nothing is ever swapped and the row permutation handed on is the identity.
// ---- trailing update shared between workgroups ----------------------------------------------------------------------
// The trailing update of a panel (C = Q_p^H A, A <- A - Q_p C on the MFMA pipe) is 55 % of k_qr_large on a 202 x 202 block and
// runs at the MFMA rate of ONE CU (measured 471 of 860 us; window 81, panel steps 299), 77 % on a 400 x 400 block (3.0 of
// 3.9 ms).  With NW > 1 workgroups per block (see the launch site for when) the master (role 0) keeps the pivoting and the
// panel factorisation and publishes, per panel, the panel basis Q_p, the column map and the panel's geometry; every workgroup
// then updates the 16-column chunks ch with ch % NW == role -- all its waves together, qr_trailing_coop -- and the helpers hand
// back the new column norms.  Everything that crosses workgroups inside the launch follows cdna_hip_programming.md section 6,
// Guideline 16 (first table row of MI355X_MICROARCH.md "visibility"): every storing wave drains, workgroup barrier, ONE lane
// raises an epoch with an agent-scope atomic store; the other side polls that word from one lane, workgroup barrier, and every
// load of shared bytes is an sc1 load (served by the L2).  The STORES of the shared bytes -- Q_p, the updated columns of A, the
// rows of R in X -- come in two flavours: write-through (sc1), correct wherever the workgroups run; or plain, kept in the
// XCD's L2, used only when every workgroup of the block has read the same XCD id from the hardware (k_qr_large) -- the
// launch puts a block's workgroups at grid positions of one residue mod 8, which the dispatcher has been seen to deal to one
// XCD, but nothing is assumed: a block that finds itself spread out takes the first flavour.  Polls are bounded (qr_wait_ge).
// Measured, 202 x 202 (tools/ring_prof.py, -DHTN_QR_PROF): one workgroup 858 us (trailing 452); four workgroups through
// memory 964; four through the shared L2 755; the same with all 16 waves of a workgroup on its chunks 619 (trailing 212).
typedef unsigned int qr_u4 __attribute__((ext_vector_type(4)));
struct QrShare {
    int NW, role;
    bool local;              // every workgroup of the block reports the same XCD: bulk stores stay in that XCD's L2 (plain), see k_qr_large
    double2* qn;             // [16 * ldq] panel basis (global copy)
    int* scol;               // [n0] logical -> physical column
    double* cn2;             // [n0] squared norms the helpers computed (by logical position)
    int* meta;               // j0, nb_eff, k_first, last_panel, finished
    unsigned* qflag;         // master -> helpers: number of panels published so far
    unsigned* hflag;         // [NW]: helper -> master: panels completed
    unsigned* fail;
};
__device__ __forceinline__ bool qr_wait_ge(unsigned* flag, unsigned want, unsigned* fail) {
    const long long t0 = wall_clock64();
    for (unsigned spins = 1;; ++spins) {
        if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want) return true;
        __builtin_amdgcn_s_sleep(1);
        if ((spins & 255u) == 0u) {
            if (__hip_atomic_load(fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return false;
            if (wall_clock64() - t0 > 300000000ll) {             // 3 s of the 100 MHz constant clock
                __hip_atomic_store(fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return false;
            }
        }
    }
}
template <bool SH>
__device__ __forceinline__ double2 qr_ld(const double2* base, __amdgpu_buffer_rsrc_t rs, int idx) {
    if (!SH) return base[idx];
    const qr_u4 u = __builtin_amdgcn_raw_buffer_load_b128(rs, idx * 16, 0, 16);
    double2 v;
    __builtin_memcpy(&v, &u, 16);
    return v;
}
template <bool SH>
__device__ __forceinline__ void qr_st(double2* base, __amdgpu_buffer_rsrc_t rs, int idx, double2 v, bool local) {
    if (!SH) {
        base[idx] = v;
        return;
    }
    qr_u4 u;
    __builtin_memcpy(&u, &v, 16);
    if (local) __builtin_amdgcn_raw_buffer_store_b128(u, rs, idx * 16, 0, 0);      // stays in the XCD's L2; the readers' sc1 loads hit it there
    else __builtin_amdgcn_raw_buffer_store_b128(u, rs, idx * 16, 0, 16);
}

// one 16-column chunk of the trailing update by one wave: rows j0 .. of R for its columns (-> X), then the columns themselves
// and their new norms (norm_out[k], LDS for the master, the shared array for a helper)
template <bool SH>
__device__ __forceinline__ void qr_trailing_chunk(double2* __restrict__ g0, __amdgpu_buffer_rsrc_t rg, double2* __restrict__ Xg,
                                                  __amdgpu_buffer_rsrc_t rx, const double2* Qn, int ldq, const int* s_col, int m0,
                                                  int m0p, int n0, int mp, int j0, int nb_eff, int k_first, int ch, bool last_panel,
                                                  double* norm_out, bool norm_shared, int lane, bool local) {
    const int l15 = lane & 15, l4 = lane >> 4;
    const int nks = m0p >> 2;
    const int k = k_first + 16 * ch + l15;
    const bool valid = k < n0;
    const int pk = valid ? s_col[k] : 0;
    const int abase = pk * m0;
    d4 cr = {0.0, 0.0, 0.0, 0.0}, ci = {0.0, 0.0, 0.0, 0.0};
    const double2* qrow = Qn + l15 * ldq + l4;
    double2 ring[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = 4 * u + l4;
        ring[u] = (valid && u < nks && i < m0) ? qr_ld<SH>(g0, rg, abase + i) : make_double2(0.0, 0.0);
    }
    for (int ks0 = 0; ks0 < nks; ks0 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ks = ks0 + u;
            if (ks < nks) {
                const double2 b = ring[u];
                const int inx = 4 * (ks + 4) + l4;
                ring[u] = (valid && ks + 4 < nks && inx < m0) ? qr_ld<SH>(g0, rg, abase + inx) : make_double2(0.0, 0.0);
                const double2 qv = qrow[4 * ks];
                cr = __builtin_amdgcn_mfma_f64_16x16x4f64(qv.x, b.x, cr, 0, 0, 0);
                ci = __builtin_amdgcn_mfma_f64_16x16x4f64(qv.x, b.y, ci, 0, 0, 0);
                cr = __builtin_amdgcn_mfma_f64_16x16x4f64(qv.y, b.y, cr, 0, 0, 0);
                ci = __builtin_amdgcn_mfma_f64_16x16x4f64(-qv.y, b.x, ci, 0, 0, 0);
            }
        }
    }
    // rows j0 + (l4 + 4 reg) of R, column k
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int t = l4 + 4 * reg;
        if (valid && t < nb_eff) qr_st<SH>(Xg, rx, (j0 + t) * mp + pk, make_double2(cr[reg], -ci[reg]), local);
    }
    if (last_panel) return;                       // no later panel reads the trailing columns
    double nrm = 0.0;
    for (int i0 = 0; i0 < m0p; i0 += 16) {
        double2 old[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int i = i0 + l4 + 4 * reg;
            old[reg] = (valid && i < m0) ? qr_ld<SH>(g0, rg, abase + i) : make_double2(0.0, 0.0);
        }
        d4 dr = {0.0, 0.0, 0.0, 0.0}, di = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const double2 qa = Qn[(l4 + 4 * kk) * ldq + i0 + l15];
            dr = __builtin_amdgcn_mfma_f64_16x16x4f64(qa.x, cr[kk], dr, 0, 0, 0);
            di = __builtin_amdgcn_mfma_f64_16x16x4f64(qa.x, ci[kk], di, 0, 0, 0);
            dr = __builtin_amdgcn_mfma_f64_16x16x4f64(-qa.y, ci[kk], dr, 0, 0, 0);
            di = __builtin_amdgcn_mfma_f64_16x16x4f64(qa.y, cr[kk], di, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int i = i0 + l4 + 4 * reg;
            if (valid && i < m0) {
                const double2 x = make_double2(old[reg].x - dr[reg], old[reg].y - di[reg]);
                qr_st<SH>(g0, rg, abase + i, x, local);
                nrm += x.x * x.x + x.y * x.y;
            }
        }
    }
    nrm += __shfl_xor(nrm, 16, 64);      // over the 4 lanes (l4) that share a column
    nrm += __shfl_xor(nrm, 32, 64);
    if (valid && l4 == 0) {
        if (norm_shared) __hip_atomic_store(norm_out + k, nrm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else norm_out[k] = nrm;
    }
}

// a helper workgroup of a block: per published panel, fetch Q_p and the column map, update its chunks, report
// The trailing update of one workgroup's chunks (ch = role, role + NW, ... < nchunks) by ALL its 16 waves.  One wave per chunk
// (qr_trailing_chunk) leaves most of the SIMDs idle once helpers share the chunks: four workgroups x three chunks = three
// busy waves per CU for 12 us (404 f64 MFMAs at 64 clk).  Here S = 4 waves share a chunk when the block is small enough for
// the partial sums to fit the LDS beside the panel (m0p <= 256; `part` != nullptr): part p of a chunk takes every S-th group
// of four k-steps of C = Q_p^H A -- the S partial C tiles are added through LDS in part order, every part ends up with the
// same full C in the MFMA's D layout -- and every S-th row tile of A <- A - Q_p C; part 0 writes the rows of R, the column
// norms are added through LDS in part order.  S depends on the block's size only, never on NW or on which workgroup has the
// chunk: the result is the same bit for bit with or without helpers.  Called by every wave of the workgroup (barriers).
template <bool SH>
__device__ __forceinline__ void qr_trailing_coop(double2* __restrict__ g0, __amdgpu_buffer_rsrc_t rg, double2* __restrict__ Xg,
                                                 __amdgpu_buffer_rsrc_t rx, const double2* Qn, int ldq, const int* s_col, int m0,
                                                 int m0p, int n0, int mp, int j0, int nb_eff, int k_first, int nchunks, int role,
                                                 int NW, bool last_panel, double* norm_out, bool norm_shared, double* part,
                                                 int tid, bool local) {
    __shared__ double s_np[JAC_THREADS / 64][16];
    const int lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int cnt = nchunks > role ? (nchunks - role + NW - 1) / NW : 0;
    if (part == nullptr) {             // one wave per chunk
        for (int q = wave; q < cnt; q += JAC_THREADS / 64)
            qr_trailing_chunk<SH>(g0, rg, Xg, rx, Qn, ldq, s_col, m0, m0p, n0, mp, j0, nb_eff, k_first, role + NW * q, last_panel, norm_out,
                                  norm_shared, lane, local);
        return;
    }
    constexpr int S = 4, CPR = (JAC_THREADS / 64) / S;      // waves per chunk, chunks per round
    const int nks = m0p >> 2;
    for (int r0 = 0; r0 < cnt; r0 += CPR) {                 // (uniform over the workgroup)
        const int ci_ = r0 + wave / S, pp = wave % S;
        const bool act = ci_ < cnt;
        const int ch = role + NW * ci_;
        const int k = k_first + 16 * ch + l15;
        const bool valid = act && k < n0;
        const int pk = valid ? s_col[k] : 0;
        const int abase = pk * m0;
        d4 cr = {0.0, 0.0, 0.0, 0.0}, ci = {0.0, 0.0, 0.0, 0.0};
        if (act) {
            const double2* qrow = Qn + l15 * ldq + l4;
            double2 ring[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ks = 4 * pp + u, i = 4 * ks + l4;
                ring[u] = (valid && ks < nks && i < m0) ? qr_ld<SH>(g0, rg, abase + i) : make_double2(0.0, 0.0);
            }
            for (int ks0 = 4 * pp; ks0 < nks; ks0 += 4 * S) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int ks = ks0 + u;
                    if (ks < nks) {
                        const double2 b = ring[u];
                        const int ksn = ks + 4 * S, inx = 4 * ksn + l4;
                        ring[u] = (valid && ksn < nks && inx < m0) ? qr_ld<SH>(g0, rg, abase + inx) : make_double2(0.0, 0.0);
                        const double2 qv = qrow[4 * ks];
                        cr = __builtin_amdgcn_mfma_f64_16x16x4f64(qv.x, b.x, cr, 0, 0, 0);
                        ci = __builtin_amdgcn_mfma_f64_16x16x4f64(qv.x, b.y, ci, 0, 0, 0);
                        cr = __builtin_amdgcn_mfma_f64_16x16x4f64(qv.y, b.y, cr, 0, 0, 0);
                        ci = __builtin_amdgcn_mfma_f64_16x16x4f64(-qv.y, b.x, ci, 0, 0, 0);
                    }
                }
            }
        }
        // partial C tiles -> LDS ([wave][reg][lane]: conflict-free), added in part order by every part
        {
            double* mine = part + (size_t)wave * 512 + lane;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                mine[64 * reg] = cr[reg];
                mine[64 * (4 + reg)] = ci[reg];
            }
        }
        __syncthreads();
        {
            const double* base = part + (size_t)(wave - pp) * 512 + lane;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                double a = 0.0, b = 0.0;
#pragma unroll
                for (int q = 0; q < S; ++q) {
                    a += base[q * 512 + 64 * reg];
                    b += base[q * 512 + 64 * (4 + reg)];
                }
                cr[reg] = a;
                ci[reg] = b;
            }
        }
        if (pp == 0) {                                  // rows j0 + (l4 + 4 reg) of R, column k
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int t = l4 + 4 * reg;
                if (valid && t < nb_eff) qr_st<SH>(Xg, rx, (j0 + t) * mp + pk, make_double2(cr[reg], -ci[reg]), local);
            }
        }
        if (!last_panel) {                              // (uniform) no later panel reads the trailing columns otherwise
            double nrm = 0.0;
            if (act) {
                for (int i0 = 16 * pp; i0 < m0p; i0 += 16 * S) {
                    double2 old[4];
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int i = i0 + l4 + 4 * reg;
                        old[reg] = (valid && i < m0) ? qr_ld<SH>(g0, rg, abase + i) : make_double2(0.0, 0.0);
                    }
                    d4 dr = {0.0, 0.0, 0.0, 0.0}, di = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        const double2 qa = Qn[(l4 + 4 * kk) * ldq + i0 + l15];
                        dr = __builtin_amdgcn_mfma_f64_16x16x4f64(qa.x, cr[kk], dr, 0, 0, 0);
                        di = __builtin_amdgcn_mfma_f64_16x16x4f64(qa.x, ci[kk], di, 0, 0, 0);
                        dr = __builtin_amdgcn_mfma_f64_16x16x4f64(-qa.y, ci[kk], dr, 0, 0, 0);
                        di = __builtin_amdgcn_mfma_f64_16x16x4f64(qa.y, cr[kk], di, 0, 0, 0);
                    }
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int i = i0 + l4 + 4 * reg;
                        if (valid && i < m0) {
                            const double2 x = make_double2(old[reg].x - dr[reg], old[reg].y - di[reg]);
                            qr_st<SH>(g0, rg, abase + i, x, local);
                            nrm += x.x * x.x + x.y * x.y;
                        }
                    }
                }
            }
            nrm += __shfl_xor(nrm, 16, 64);      // over the 4 lanes (l4) that share a column
            nrm += __shfl_xor(nrm, 32, 64);
            if (l4 == 0) s_np[wave][l15] = nrm;
            __syncthreads();
            if (valid && pp == 0 && l4 == 0) {
                double t = 0.0;
#pragma unroll
                for (int q = 0; q < S; ++q) t += s_np[wave + q][l15];
                if (norm_shared) __hip_atomic_store(norm_out + k, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else norm_out[k] = t;
            }
        }
        __syncthreads();                                // the partial tiles and norms are free for the next round
    }
}

__device__ __forceinline__ void qr_helper(double2* __restrict__ g0, int m0, int n0, int r, double2* __restrict__ Xg, int mp, int* s_col,
                                          double2* Qn, int tid, const QrShare sh, double* part) {
    __shared__ int s_meta[8];
    const int lane = tid & 63, wave = tid >> 6;
    const int m0p = (m0 + 15) & ~15, ldq = m0p + 1;
    const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)g0, 0, m0 * n0 * 16, 0x00020000);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)Xg, 0, mp * r * 16, 0x00020000);
    const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)sh.qn, 0, 16 * ldq * 16, 0x00020000);
    for (unsigned epoch = 1;; ++epoch) {
        if (tid == 0) {
            const bool ok = qr_wait_ge(sh.qflag, epoch, sh.fail);
            s_meta[5] = ok ? 0 : 1;
            for (int q = 0; q < 5; ++q) s_meta[q] = ok ? __hip_atomic_load(sh.meta + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        }
        __syncthreads();
        const int j0 = s_meta[0], nb_eff = s_meta[1], k_first = s_meta[2];
        const bool last_panel = s_meta[3] != 0, finished = s_meta[4] != 0 || s_meta[5] != 0;
        if (finished) break;
        for (int idx = tid; idx < 16 * ldq; idx += JAC_THREADS) Qn[idx] = qr_ld<true>(sh.qn, rq, idx);
        for (int k = k_first + tid; k < n0; k += JAC_THREADS) s_col[k] = __hip_atomic_load(sh.scol + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const int nchunks = (n0 - k_first + 15) >> 4;
        qr_trailing_coop<true>(g0, rg, Xg, rx, Qn, ldq, s_col, m0, m0p, n0, mp, j0, nb_eff, k_first, nchunks, sh.role, sh.NW, last_panel, sh.cn2,
                               true, part, tid, sh.local);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_store(sh.hflag + sh.role, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

#ifdef HTN_QR_PROF          // diagnostic build only (tools/ring_prof.py --qr): 100 MHz ticks per phase of k_qr_large, block 0
__device__ long long g_qr_prof[8];
extern "C" int htn_qr_prof_dump(long long* out) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_qr_prof), sizeof(long long) * 8));
    return 0;
}
#endif
template <int EL, bool SH>
__device__ __forceinline__ int qrcp_blocked(double2* __restrict__ g0, int m0, int n0, int r,
                                            double2* __restrict__ Xg, int mp, int* s_col, double* s_cn2,
                                            double* s_piv, double2* Qn, int tid, double cut2, const QrShare sh, double* part) {
    __shared__ double s_pn[16];
    __shared__ int s_share_ok;
    const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)g0, 0, m0 * n0 * 16, 0x00020000);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)Xg, 0, mp * r * 16, 0x00020000);
    unsigned pub_epoch = 0;
    if (tid == 0) s_share_ok = 1;
    __shared__ double2 s_r[16][17];      // the panel's own R block, [pivot step][owner wave]; flushed once per panel
    __shared__ int s_pc[16];
    __shared__ int s_pos[16];
    __shared__ int s_nb;
    const int lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int m0p = (m0 + 15) & ~15, ldq = m0p + 1;
    for (int idx = tid; idx < mp * r; idx += JAC_THREADS) qr_st<SH>(Xg, rx, idx, make_double2(0.0, 0.0), sh.local);
    for (int k = wave; k < n0; k += JAC_THREADS / 64) {
        double c = 0.0;
        for (int i = lane; i < m0; i += 64) {
            const double2 x = g0[(int64_t)k * m0 + i];       // (written before this launch: plain loads)
            c += x.x * x.x + x.y * x.y;
        }
        c = wave_sum(c);
        if (lane == 0) {
            s_cn2[k] = c;
            s_col[k] = k;
        }
    }
    __syncthreads();
    if (wave == 0) {
        double f = 0.0;
        for (int k = lane; k < n0; k += 64) f += s_cn2[k];
        f = wave_sum(f);
        if (lane == 0) s_piv[1] = 1e-30 * f;       // "numerically zero" threshold on squared norms
    }
    __syncthreads();
    const double zero2 = s_piv[1];
    bool stop = false;
    int j0 = 0, rank = 0;
#ifdef HTN_QR_PROF
    long long qprof[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // window | panel load | panel steps | flush | trailing | total | panels
    const long long qt0 = wall_clock64();
#endif
    while (j0 < r && !stop) {
        JAC_T(QR_PROF, q0);
        const int nbmax = r - j0 < 16 ? r - j0 : 16;
        // ---- (a) window: the nbmax largest remaining columns move to logical positions j0 .. ----
        if (wave == 0) {
            int nb = 0;
            // rank-revealing stop: the squared Frobenius norm of everything not yet factorised (= |R22|_F^2, the
            // residual column norms are recomputed exactly) bounds every remaining singular value; below the
            // caller's cut (htn_jacobi_set_rank_cut) the remaining rows of R are dropped
            double mass = 0.0;
            for (int k = j0 + lane; k < n0; k += 64) mass += s_cn2[k];
            mass = wave_sum(mass);
            for (int t = 0; t < (mass <= cut2 ? 0 : nbmax); ++t) {
                const int j = j0 + t;
                // key = norm bits with the low 10 mantissa bits replaced by 1023 - k: one 64-bit max finds the
                // largest norm, ties (to 2^-42 relative) going to the smallest position
                unsigned long long key = 0ull;
                for (int k = j + lane; k < n0; k += 64) {
                    const unsigned long long kk =
                        ((unsigned long long)__double_as_longlong(s_cn2[k]) & ~0x3FFull) | (unsigned long long)(1023 - k);
                    key = kk > key ? kk : key;
                }
                key = wave_max_u64(key);
                const int bi = 1023 - (int)(key & 0x3FFull);
                const double best = s_cn2[bi];
                if (best <= zero2) break;
                if (lane == 0) {
                    const int tc = s_col[j];
                    s_col[j] = s_col[bi];
                    s_col[bi] = tc;
                    s_cn2[bi] = s_cn2[j];
                    s_cn2[j] = best;
                }
                ++nb;
            }
            if (lane == 0) s_nb = nb;
        }
        __syncthreads();
        JAC_T(QR_PROF, q1);
        JAC_ACC(QR_PROF, qprof, 0, q0, q1);
        int nb = s_nb;
        if (nb == 0) break;                          // numerically rank deficient: remaining R rows are zero
        if (nb < nbmax) stop = true;
        // ---- (b) panel factorisation: wave u < nb owns logical column j0 + u in registers ----
        const bool owner = wave < nb;
        const int pc = owner ? s_col[j0 + wave] : 0;
        double2 a[EL];
        double cn = owner ? s_cn2[j0 + wave] : -1.0;
        const double ns = cn;
#pragma unroll
        for (int e = 0; e < EL; ++e) {
            const int i = lane + 64 * e;
            a[e] = (owner && i < m0) ? qr_ld<SH>(g0, rg, pc * m0 + i) : make_double2(0.0, 0.0);
        }
        if (!owner)                                   // unused panel positions project onto nothing
            for (int i = lane; i < m0p; i += 64) Qn[wave * ldq + i] = make_double2(0.0, 0.0);
        // no global store inside the step loop: a store keeps its source registers busy until it has left the
        // memory pipeline, and the next step would wait for that (s_waitcnt vmcnt(0)) before reusing them
        if (tid < 256) s_r[tid >> 4][tid & 15] = make_double2(0.0, 0.0);
        if (lane == 0) s_pc[wave] = pc;
        bool pending = owner;
        int nb_eff = nb;
        JAC_T(QR_PROF, q2);
        JAC_ACC(QR_PROF, qprof, 1, q1, q2);
        for (int t = 0; t < nb; ++t) {
            if (lane == 0) s_pn[wave] = pending ? cn : -1.0;
            lds_barrier();
            unsigned long long key = 0ull;             // same packing, 4 tag bits: 15 - wave
            {
                const double v = s_pn[l15];
                if (v >= 0.0) key = ((unsigned long long)__double_as_longlong(v) & ~0xFull) | (unsigned long long)(15 - l15);
            }
            key = row_max16_u64(key);
            const int bu = 15 - (int)(key & 0xFull);
            const double best = key ? s_pn[bu] : -1.0;
            if (best <= zero2) {                      // the rest of the panel is numerically zero (uniform)
                nb_eff = t;
                stop = true;
                break;
            }
            if (wave == bu) {
                if (cn < 1e-4 * ns) {                 // second projection against the panel's earlier pivots
                    for (int s2 = 0; s2 < t; ++s2) {
                        double dr = 0.0, di = 0.0;
                        const double2* qs = Qn + s2 * ldq + lane;
#pragma unroll
                        for (int e = 0; e < EL; ++e) {
                            if (lane + 64 * e < m0p) {
                                const double2 q = qs[64 * e];
                                dr += q.x * a[e].x + q.y * a[e].y;
                                di += q.x * a[e].y - q.y * a[e].x;
                            }
                        }
                        dr = wave_sum(dr);
                        di = wave_sum(di);
#pragma unroll
                        for (int e = 0; e < EL; ++e) {
                            if (lane + 64 * e < m0p) {
                                const double2 q = qs[64 * e];
                                a[e].x -= dr * q.x - di * q.y;
                                a[e].y -= dr * q.y + di * q.x;
                            }
                        }
                        if (lane == 0) {
                            const double2 old = s_r[s2][wave];
                            s_r[s2][wave] = make_double2(old.x + dr, old.y - di);
                        }
                    }
                    double c = 0.0;
#pragma unroll
                    for (int e = 0; e < EL; ++e) c += a[e].x * a[e].x + a[e].y * a[e].y;
                    cn = wave_sum(c);
                }
                const double ipn = fast_rsq(cn);
                const double pn = cn * ipn;
#pragma unroll
                for (int e = 0; e < EL; ++e) {
                    const int i = lane + 64 * e;
                    if (i < m0p) Qn[t * ldq + i] = make_double2(a[e].x * ipn, a[e].y * ipn);
                }
                if (lane == 0) {
                    s_r[t][wave] = make_double2(pn, 0.0);
                    s_pos[t] = pc;
                }
                pending = false;
            }
            lds_barrier();
            if (pending) {
                double dr = 0.0, di = 0.0;
                const double2* qt = Qn + t * ldq + lane;       // zero padded up to m0p; a[e] is zero beyond m0
#pragma unroll
                for (int e = 0; e < EL; ++e) {
                    if (lane + 64 * e < m0p) {
                        const double2 q = qt[64 * e];
                        dr += q.x * a[e].x + q.y * a[e].y;          // conj(q) * a
                        di += q.x * a[e].y - q.y * a[e].x;
                    }
                }
                dr = wave_sum(dr);
                di = wave_sum(di);
                double c = 0.0;
#pragma unroll
                for (int e = 0; e < EL; ++e) {
                    if (lane + 64 * e < m0p) {
                        const double2 q = qt[64 * e];
                        a[e].x -= dr * q.x - di * q.y;
                        a[e].y -= dr * q.y + di * q.x;
                        c += a[e].x * a[e].x + a[e].y * a[e].y;
                    }
                }
                cn = wave_sum(c);
                if (lane == 0) s_r[t][wave] = make_double2(dr, -di);   // conj(r_tk)
            }
        }
        __syncthreads();
        JAC_T(QR_PROF, q3);
        JAC_ACC(QR_PROF, qprof, 2, q2, q3);
        if (nb_eff < nb) {                            // zero the positions the early exit left unwritten
            for (int tt = nb_eff + wave; tt < nb; tt += JAC_THREADS / 64)
                for (int i = lane; i < m0p; i += 64) Qn[tt * ldq + i] = make_double2(0.0, 0.0);
        }
        if (tid < nb_eff) s_col[j0 + tid] = s_pos[tid];
        if (tid < 256 && (tid >> 4) < nb_eff && (tid & 15) < nb)      // rows of R before a column's own pivot step: 0
            qr_st<SH>(Xg, rx, (j0 + (tid >> 4)) * mp + s_pc[tid & 15], s_r[tid >> 4][tid & 15], sh.local);
        __syncthreads();
        JAC_T(QR_PROF, q4);
        JAC_ACC(QR_PROF, qprof, 3, q3, q4);
        // ---- (c) trailing update: wave per chunk of 16 logical columns ----
        const int k_first = j0 + nb;
        const int nchunks = (n0 - k_first + 15) >> 4;
        const bool last_panel = stop || k_first >= r;
        const int NW = SH ? sh.NW : 1;
        if (SH && nchunks > 0) {
            // publish the panel: basis, column map of the trailing part, geometry; drain; ONE lane raises the epoch
            const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)sh.qn, 0, 16 * ldq * 16, 0x00020000);
            for (int idx = tid; idx < 16 * ldq; idx += JAC_THREADS) qr_st<true>(sh.qn, rq, idx, Qn[idx], sh.local);
            for (int k = k_first + tid; k < n0; k += JAC_THREADS) __hip_atomic_store(sh.scol + k, s_col[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (tid == 0) {
                __hip_atomic_store(sh.meta + 0, j0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(sh.meta + 1, nb_eff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(sh.meta + 2, k_first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(sh.meta + 3, last_panel ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(sh.meta + 4, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            ++pub_epoch;
            if (tid == 0) __hip_atomic_store(sh.qflag, pub_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // the master's share: chunks ch with ch % NW == 0
        qr_trailing_coop<SH>(g0, rg, Xg, rx, Qn, ldq, s_col, m0, m0p, n0, mp, j0, nb_eff, k_first, nchunks, 0, NW, last_panel, s_cn2, false, part,
                             tid, sh.local);
        if (SH && nchunks > 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this workgroup's own column updates are out before the next panel reads them
            __syncthreads();
            if (tid == 0) {
                bool ok = true;
                for (int h = 1; h < NW && ok; ++h) ok = qr_wait_ge(sh.hflag + h, pub_epoch, sh.fail);
                if (!ok) s_share_ok = 0;
            }
            __syncthreads();
            if (!s_share_ok) {
                stop = true;
            } else if (!last_panel) {
                for (int k = k_first + tid; k < n0; k += JAC_THREADS)
                    if (((k - k_first) >> 4) % NW != 0) s_cn2[k] = __hip_atomic_load(sh.cn2 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
        JAC_T(QR_PROF, q5);
        JAC_ACC(QR_PROF, qprof, 4, q4, q5);
#ifdef HTN_QR_PROF
        qprof[6] += 1;
#endif
        j0 += nb;
        rank += nb_eff;
    }
    __syncthreads();
#ifdef HTN_QR_PROF
    if (tid == 0 && blockIdx.x == 0) {
        qprof[5] = wall_clock64() - qt0;
        for (int q = 0; q < 8; ++q) g_qr_prof[q] = qprof[q];
    }
#endif
    if (SH) {                  // release the helpers (every path out of the panel loop ends here)
        if (tid == 0) {
            __hip_atomic_store(sh.meta + 4, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(sh.qflag, pub_epoch + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (!s_share_ok) rank = -1;
    }
    for (int i = tid; i < n0; i += JAC_THREADS) s_col[i] = i;      // rows of X are physical columns already
    __syncthreads();
    return rank;
}

// one workgroup per LARGE block (X = R^H does not fit the LDS window): pivoted QR only; the sweeps follow as
// multi-launch block Jacobi.  Runs beside k_jacobi_svd (small blocks) on a forked stream.
#define QR_SYNC_WORDS 16         // per large block: panel epoch | helper epochs [1 .. 4] | ... | XCD ids [8 .. 11]
#define QR_BOX_BYTES 137728      // per large block: 16 x 513 complex128 (Q_p) | 512 int (column map) | 512 double (norms) | meta
__global__ __launch_bounds__(JAC_THREADS) void k_qr_large(double2* __restrict__ G, double2* __restrict__ Vj,
                                                          const htn_svd_block* __restrict__ desc,
                                                          const int* __restrict__ large_ids, int* __restrict__ perm,
                                                          double* __restrict__ zero2_out, double cut2,
                                                          int* __restrict__ rank_host, int NW, char* __restrict__ qr_box,
                                                          unsigned* __restrict__ qr_sync, int nl, int nx, int part_off) {
    extern __shared__ double2 g_lds[];
    __shared__ double s_piv[2];
    __shared__ int s_col[64 * JAC_MAXEL];
    __shared__ double s_cn2[64 * JAC_MAXEL];
    __shared__ int s_qlocal;
    // grid position -> (block, role): with helpers (NW > 1) the workgroups of one block sit at positions p = nx s + x with ONE x
    // (nx = 8: the dispatcher has been seen to deal position p to XCD p mod 8), blocks x, x + nx, ... stacked along s
    const int px = (int)(blockIdx.x % (unsigned)nx), ps = (int)(blockIdx.x / (unsigned)nx);
    const int li = (ps / NW) * nx + px, role = ps % NW;
    if (li >= nl) return;             // (a gap of the placement)
    const htn_svd_block D = desc[large_ids[li]];
    const int m = D.m, n = D.n, m0 = D.pad, tid = threadIdx.x;
    const int gsx = m <= 16 * JAC_MAXEL ? 16 : (m <= 32 * JAC_MAXEL ? 32 : 64);
    const int mp = gsx * ((m + gsx - 1) / gsx);
    double2* __restrict__ X = Vj + D.v_off;
    QrShare sh;
    sh.NW = NW, sh.role = role;
    char* box = qr_box + (size_t)li * QR_BOX_BYTES;
    sh.qn = (double2*)box;
    sh.scol = (int*)(box + 16 * 513 * 16);
    sh.cn2 = (double*)(box + 16 * 513 * 16 + 512 * 4);
    sh.meta = (int*)(box + 16 * 513 * 16 + 512 * 4 + 512 * 8);
    sh.qflag = qr_sync + li * QR_SYNC_WORDS;
    sh.hflag = qr_sync + li * QR_SYNC_WORDS + 1;
    sh.fail = qr_sync + nl * QR_SYNC_WORDS;
    sh.local = false;
    if (NW > 1) {
        // the same check as in the ring kernel (ring_run): take the hand-off through the XCD's L2 only if every workgroup of the
        // block READS the same XCD id from the hardware; any other outcome keeps the placement-independent sc1 form
        if (tid == 0) {
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            xcc = (xcc & 0xfu) + 1u;
            unsigned* xw = qr_sync + li * QR_SYNC_WORDS + 8;
            __hip_atomic_store(xw + role, xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int local = 1;
            for (int q = 0; q < NW && local >= 0; ++q) {
                if (!qr_wait_ge(xw + q, 1u, sh.fail)) local = -1;
                else if (__hip_atomic_load(xw + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != xcc) local = 0;
            }
            s_qlocal = local;
        }
        __syncthreads();
        sh.local = s_qlocal > 0;
        // (a timed-out wait has raised the failure word: the master's and the helpers' first hand-off see it and give up)
    }
    // LDS beside the panel for the partial sums of the shared chunks (qr_trailing_coop): blocks of up to 256 rows, when the launch
    // reserved it (part_off = the panel's extent in complex elements)
    double* part = (part_off > 0 && ((m0 + 15) & ~15) <= 256) ? (double*)(g_lds + part_off) : nullptr;
    if (role > 0) {
        qr_helper(G + D.g_off, m0, m, n, X, mp, s_col, (double2*)g_lds, tid, sh, part);
        return;
    }
    int rank;
    if (NW > 1) {
        if (m0 <= 256) rank = qrcp_blocked<4, true>(G + D.g_off, m0, m, n, X, mp, s_col, s_cn2, s_piv, (double2*)g_lds, tid, cut2, sh, part);
        else rank = qrcp_blocked<8, true>(G + D.g_off, m0, m, n, X, mp, s_col, s_cn2, s_piv, (double2*)g_lds, tid, cut2, sh, part);
    } else {
        if (m0 <= 256) rank = qrcp_blocked<4, false>(G + D.g_off, m0, m, n, X, mp, s_col, s_cn2, s_piv, (double2*)g_lds, tid, cut2, sh, part);
        else rank = qrcp_blocked<8, false>(G + D.g_off, m0, m, n, X, mp, s_col, s_cn2, s_piv, (double2*)g_lds, tid, cut2, sh, part);
    }
    if (tid == 0) {
        rank_host[li] = rank;                       // host-pinned: the host sizes the Jacobi tournament with it (< 0: a hand-off timed out)
        // threshold for "numerically zero" columns of X = R^H: |X|_F^2 = |G0|_F^2 (the QR preserves it), summed in fixed order above
        zero2_out[li] = s_piv[1];
        __threadfence_system();
    }
    for (int i = tid; i < m; i += JAC_THREADS) perm[li * 64 * JAC_MAXEL + i] = s_col[i];
}
