// SVD staging of the two-site update, the global truncation rule and the post-SVD finalisation.  Host C++ (no HIP).
// NOT a translation unit of its own: #included by htn_plan.cpp (one unit, see its head); never name it on a build line.
#include "htn_tasks.h"

namespace htn {

// ---- SVD staging ---------------------------------------------------------------------------------------------------
// Default (QRCP): stage G0 = M^H ('right') or M ('left'); the kernel preconditions it by pivoted QR and runs Jacobi on
// R^H, returning (isometry x Sigma) directly.  Blocks with a side > 512 fall back to the plain staging: mode A stages
// the block so that the normalised Jacobi output IS the wanted isometry; mode B (block much wider than tall in that
// orientation) orthogonalises the short side instead and accumulates the rotation J, which then is the isometry.
// A block above 512 in both orientations is staged in mode A like any other; its columns are longer than one
// workgroup's registers hold, and the kernel gives it the multi-CU pair-visit path with row-chunked columns.
int plan_svd(const ThetaLayout& tl, bool right, SvdPlan& out) {
    const size_t n = tl.mats.size();
    out = SvdPlan();
    out.desc.resize(std::max<size_t>(n, 1));
    out.stage.resize(std::max<size_t>(n, 1));
    memset(out.desc.data(), 0, sizeof(htn_svd_block) * out.desc.size());
    memset(out.stage.data(), 0, sizeof(htn_copy_item) * out.stage.size());
    int64_t go = 0, vo = 0, so = 0;
    for (size_t i = 0; i < n; ++i) {
        const auto& M = tl.mats[i];
        out.mids.push_back(M.c);
        const int rows = M.rows, cols = M.cols;
        const int mA = right ? rows : cols, nA = right ? cols : rows;
        htn_svd_block& d = out.desc[i];
        htn_copy_item& st = out.stage[i];
        st.src_off = M.off;
        st.idx_off = -1;
        st.scl_off = -1;
        st.lds = rows;
        st.gather_dim = 0;
        st.scale_dim = -1;
        st.inv_norm = 0;
        const int64_t mm = std::max(rows, cols), kk = std::min(rows, cols);
        out.flops += 4 * (4 * mm * kk * kk + 8 * kk * kk * kk);
        if (std::max(rows, cols) <= 512) {
            const int m0 = nA, n0 = mA;                       // G0 is m0 x n0; Jacobi works on R^H: n0 x r
            const int r = std::min(m0, n0);
            d.g_off = go;
            d.v_off = vo;
            d.s_off = so;
            d.m = n0;
            d.n = r;
            d.flags = HTN_SVD_QRCP;
            d.pad = m0;
            st.dst_off = go;
            st.rows = m0;
            st.cols = n0;
            st.ldd = m0;
            st.op = right ? HTN_OP_C : HTN_OP_N;
            out.transposed.push_back(!right);
            out.accumulate.push_back(0);
            go += (int64_t)m0 * n0;
            vo += (int64_t)((n0 + 63) / 64 * 64) * r;         // padded leading dimension of the kernel's R^H workspace
            so += r;
            out.max_m = std::max(out.max_m, std::max(m0, n0));
            continue;
        }
        const bool modeA = (nA <= 1.25 * mA && mA <= 512) || nA > 512;
        int m, nn;
        bool tr, acc;
        if (modeA) {
            m = mA, nn = nA, tr = !right, acc = false;
        } else {
            m = nA, nn = mA, tr = right, acc = true;
        }
        d.g_off = go;
        d.v_off = vo;
        d.s_off = so;
        d.m = m;
        d.n = nn;
        d.flags = acc ? HTN_SVD_ACCUMULATE : 0;
        d.pad = 0;
        st.dst_off = go;
        st.rows = m;
        st.cols = nn;
        st.ldd = m;
        st.op = tr ? HTN_OP_C : HTN_OP_N;
        out.transposed.push_back(tr);
        out.accumulate.push_back(acc);
        out.any_accumulate |= acc;
        go += (int64_t)m * nn;
        vo += acc ? (int64_t)nn * nn : 0;
        so += nn;
        out.max_m = std::max(out.max_m, m);
    }
    out.g_size = go;
    out.v_size = vo;
    out.s_size = so;
    return 0;
}

// ---- global truncation ----------------------------------------------------------------------------
//   cutoff   -> truncbelow(10^-svalue), src:1007-1010 (keep Schmidt values > cutoff)
//   chi_full -> truncdim(D), src:1363-1365 (largest values while sum (2S+1) kept <= D)
// Order at the cut: by sqrt(2S+1) * Schmidt value (= tilde value) for weighting 0, by the Schmidt value for 1; ties
// broken by sector then index, so kept sets are prefixes per sector; the largest multiplet is always kept.
void truncate(const std::vector<double>& vals, const std::vector<int>& lens, const std::vector<int>& qdims, int chi_full,
              double cutoff, int weighting, std::vector<int>& counts, double& trunc_weight, double& kept_norm) {
    const double rel_floor = 1e-14;
    const size_t nsec = lens.size();
    counts.assign(nsec, 0);
    double smax = 0.0, total = 0.0;
    for (double v : vals) {
        smax = std::max(smax, v);
        total += v * v;
    }
    // The candidates of every sector are a PREFIX of its descending list (both filters are monotone inside a sector), so the
    // global order "key descending, ties by sector then index" is a k-way merge of at most a few dozen sorted runs: a heap
    // of one cursor per sector instead of a sort of every value (this runs on the host with the GPU idle, once per bond).
    struct Cur {
        double key;
        int sid, idx;
    };
    auto worse = [](const Cur& a, const Cur& b) {        // heap order: the BEST cursor on top
        if (a.key != b.key) return a.key < b.key;
        if (a.sid != b.sid) return a.sid > b.sid;
        return a.idx > b.idx;
    };
    std::vector<size_t> start(nsec);
    std::vector<Cur> heap;
    size_t p = 0;
    for (size_t k = 0; k < nsec; ++k) {
        start[k] = p;
        p += (size_t)lens[k];
    }
    auto admissible = [&](size_t k, int i) {
        if (i >= lens[k]) return false;
        const double v = vals[start[k] + i], schmidt = v / sqrt((double)qdims[k]);
        return schmidt > cutoff && v > rel_floor * smax;
    };
    auto key_of = [&](size_t k, int i) { return weighting == 0 ? vals[start[k] + i] : vals[start[k] + i] / sqrt((double)qdims[k]); };
    for (size_t k = 0; k < nsec; ++k)
        if (admissible(k, 0)) heap.push_back({key_of(k, 0), (int)k, 0});
    std::make_heap(heap.begin(), heap.end(), worse);
    int64_t tot = 0;
    double kept_w = 0.0;
    size_t kept = 0;
    while (!heap.empty()) {
        std::pop_heap(heap.begin(), heap.end(), worse);
        const Cur c = heap.back();
        heap.pop_back();
        if (chi_full > 0) {
            tot += qdims[c.sid];
            if (tot > chi_full && kept > 0) break;      // (the largest multiplet is always kept)
            if (tot > chi_full) {                        // the very first candidate alone exceeds the limit: keep it, stop
                counts[c.sid] += 1;
                const double v = vals[start[c.sid] + c.idx];
                kept_w += v * v;
                ++kept;
                break;
            }
        }
        counts[c.sid] += 1;
        const double v = vals[start[c.sid] + c.idx];
        kept_w += v * v;
        ++kept;
        if (admissible((size_t)c.sid, c.idx + 1)) {
            heap.push_back({key_of((size_t)c.sid, c.idx + 1), c.sid, c.idx + 1});
            std::push_heap(heap.begin(), heap.end(), worse);
        }
    }
    // the discarded weight is summed over what was discarded (the kept values are a prefix of every sector): total - kept_w
    // cancels to an ulp of the total, 1e-16, where the true value is zero or the 1e-30 of values below the floor
    double disc = 0.0;
    for (size_t k = 0; k < nsec; ++k)
        for (int i = counts[k]; i < lens[k]; ++i) disc += vals[start[k] + i] * vals[start[k] + i];
    trunc_weight = total > 0.0 ? disc / total : 0.0;
    kept_norm = sqrt(kept_w);
}

// ---- post-SVD finalisation -------------------------------------------------------------------------------------------
// Writes the truncated A (left layout) and B (right layout) into ONE output buffer (A at offA, B at offB).  keep[i] =
// kept count of block i of sp.  The per-update column-index array (kept columns in value order, block after block) is
// supplied at run time; here only its offsets are fixed.
//   iso_g : isometry columns taken from G' and divided by sigma           (global scale 1)
//   cen_g : centre tensor taken from G' (mode B; sigma cancels)           (global scale 1/nrm)
//   iso_v : isometry taken from the accumulated rotation J (mode B)       (global scale 1)
//   cen   : mode-A centres, U^H M or M V, as grouped-GEMM segments with alpha = 1
//           buffers: BUF_X = theta (scaled by 1/nrm by the caller), BUF_S1 = BUF_Y = the output buffer
void plan_finalize(const ThetaLayout& tl, const SvdPlan& sp, const std::vector<int>& keep, const SiteLayout& layA,
                   const SiteLayout& layB, bool right, int64_t offA, int64_t offB, FinalizePlan& out) {
    out = FinalizePlan();
    TaskList cen;
    int64_t ioff = 0;
    for (size_t i = 0; i < sp.mids.size(); ++i) {
        const int k = keep[i];
        if (k == 0) continue;
        const Sec c = sp.mids[i];
        const auto& M = tl.mats[i];
        const htn_svd_block& d = sp.desc[i];
        const int64_t oA = offA + layA.mats[layA.mat(c)].off;
        const int64_t oB = offB + layB.mats[layB.mat(c)].off;
        const bool acc = sp.accumulate[i];
        htn_copy_item itA, itB;
        memset(&itA, 0, sizeof(itA));
        memset(&itB, 0, sizeof(itB));
        // A (rows x k, ld rows): gather columns ; B (k x cols, ld k): conjugate-transposed gather of columns
        itA.dst_off = oA, itA.rows = M.rows, itA.cols = k, itA.ldd = M.rows;
        itA.idx_off = ioff, itA.gather_dim = 1, itA.op = HTN_OP_N, itA.scl_off = d.s_off;
        itB.dst_off = oB, itB.rows = k, itB.cols = M.cols, itB.ldd = k;
        itB.idx_off = ioff, itB.gather_dim = 0, itB.op = HTN_OP_C, itB.scl_off = d.s_off;
        ioff += k;
        if (right && !acc) {                 // mode A: G = M, G' = U Sigma; centre S V^H = U^H M
            itA.src_off = d.g_off, itA.lds = d.m, itA.scale_dim = 1, itA.inv_norm = 1;
            out.iso_g.push_back(itA);
            const int bi = cen.block(mk(c.N, c.j), BUF_Y, oB, k, M.cols, k);
            cen.gemm(bi, BUF_S1, oA, M.rows, HTN_OP_C, BUF_X, M.off, M.rows, HTN_OP_N, M.rows, 1.0);
        } else if (right && acc) {           // mode B: G = M^H, G' = V Sigma, J = U
            itA.src_off = d.v_off, itA.lds = d.n, itA.scale_dim = -1, itA.inv_norm = 0;
            out.iso_v.push_back(itA);
            itB.src_off = d.g_off, itB.lds = d.m, itB.scale_dim = -1, itB.inv_norm = 0;
            out.cen_g.push_back(itB);        // S V^H = conj(G')^T
        } else if (!right && !acc) {         // mode A: G = M^H, G' = V Sigma; centre U S = M V
            itB.src_off = d.g_off, itB.lds = d.m, itB.scale_dim = 0, itB.inv_norm = 1;
            out.iso_g.push_back(itB);
            const int bi = cen.block(mk(c.N, c.j), BUF_Y, oA, M.rows, k, M.rows);
            cen.gemm(bi, BUF_X, M.off, M.rows, HTN_OP_N, BUF_S1, oB, k, HTN_OP_C, M.cols, 1.0);
        } else {                             // mode B: G = M, G' = U Sigma, J = V
            itB.src_off = d.v_off, itB.lds = d.n, itB.scale_dim = -1, itB.inv_norm = 0;
            out.iso_v.push_back(itB);
            itA.src_off = d.g_off, itA.lds = d.m, itA.scale_dim = -1, itA.inv_norm = 0;
            out.cen_g.push_back(itA);        // U S = G'
        }
    }
    out.n_idx = ioff;
    out.has_cen = !cen.blocks.empty();
    if (out.has_cen) cen.finalize(out.cen);
}

}  // namespace htn
