// Task-list assembly of the planners: output blocks with their GEMM / COPY segments (TaskList) -> the htn_tile / htn_seg
// records of one grouped-GEMM launch (Tasks, htn_core.h).  Host C++ (no HIP).
#pragma once
#include <string.h>

#include <algorithm>

#include "htn_core.h"

namespace htn {

// an all-zero record of the C ABI (padding included: task lists are compared and cached as bytes)
template <class T>
inline T zero_record() {
    T z;
    memset(&z, 0, sizeof(z));
    return z;
}

struct SegRec {
    int32_t type, buf_a;
    int64_t a_off;
    int32_t lda, op_a, buf_b;
    int64_t b_off;
    int32_t ldb, op_b, k;
    cplx alpha;
    bool same(const SegRec& o) const {
        return type == o.type && buf_a == o.buf_a && a_off == o.a_off && lda == o.lda && op_a == o.op_a && buf_b == o.buf_b &&
               b_off == o.b_off && ldb == o.ldb && op_b == o.op_b && k == o.k;
    }
    htn_seg record() const {
        htn_seg r = zero_record<htn_seg>();
        r.a_off = a_off;
        r.b_off = b_off;
        r.buf_a = buf_a;
        r.buf_b = buf_b;
        r.lda = lda;
        r.ldb = ldb;
        r.k = k;
        r.op_a = op_a;
        r.op_b = op_b;
        r.type = type;
        r.alpha_re = alpha.real();
        r.alpha_im = alpha.imag() == 0.0 ? 0.0 : alpha.imag();      // never -0.0 for real coefficients
        return r;
    }
};
struct TLBlock {
    int32_t buf;
    int64_t off;
    int32_t m, n, ld;
    std::vector<SegRec> segs;
};
struct BRow {
    int64_t off;
    int32_t buf, ld, m, n;
    int64_t seg_begin, seg_count, ncopy, ksum;
};

// segment records + block table -> Tasks: K pre-split of the GEMM segments into 16-deep slabs (tile.pad[1] = 1: the
// kernel's quads walk the slab list without reading segment records) and all tiles, longest first (LPT order).  A list
// without segments or without tiles (no blocks at all, too) holds one zero record in their place: counts 0, nothing to launch,
// but never an empty upload.
inline void emit_tasks(std::vector<htn_seg>& segs, std::vector<BRow>& B, int64_t flops, Tasks& out) {
    std::vector<int64_t> cum(segs.size() + 1, 0);
    for (size_t i = 0; i < segs.size(); ++i)
        cum[i + 1] = cum[i] + (segs[i].type == HTN_SEG_GEMM ? (segs[i].k + 15) / 16 : 1);
    std::vector<htn_seg> rep((size_t)cum.back());
    for (size_t i = 0; i < segs.size(); ++i) {
        const int64_t nch = cum[i + 1] - cum[i];
        for (int64_t c = 0; c < nch; ++c) {
            htn_seg s = segs[i];
            if (s.type == HTN_SEG_GEMM) {
                const int64_t k0 = c * 16;
                s.a_off += s.op_a == HTN_OP_N ? k0 * s.lda : k0;
                s.b_off += s.op_b == HTN_OP_N ? k0 : k0 * s.ldb;
                s.k = (int32_t)std::min<int64_t>(16, s.k - k0);
            }
            rep[(size_t)(cum[i] + c)] = s;
        }
    }
    for (auto& b : B) {
        const int64_t e = cum[(size_t)(b.seg_begin + b.seg_count)], s0 = cum[(size_t)b.seg_begin];
        b.seg_count = e - s0;
        b.seg_begin = s0;
    }
    std::vector<htn_tile> tiles;
    std::vector<int64_t> work;
    for (auto& b : B) {
        const int ntr = (b.m + HTN_TILE - 1) / HTN_TILE, ntc = (b.n + HTN_TILE - 1) / HTN_TILE;
        for (int loc = 0; loc < ntr * ntc; ++loc) {
            const int r0 = (loc / ntc) * HTN_TILE, c0 = (loc % ntc) * HTN_TILE;
            htn_tile t = zero_record<htn_tile>();
            t.c_off = b.off;
            t.buf_c = b.buf;
            t.ldc = b.ld;
            t.m = std::min(HTN_TILE, b.m - r0);
            t.n = std::min(HTN_TILE, b.n - c0);
            t.row0 = r0;
            t.col0 = c0;
            t.seg_begin = (int32_t)b.seg_begin;
            t.seg_count = (int32_t)b.seg_count;
            t.pad[0] = (int32_t)b.ncopy;
            t.pad[1] = 1;
            tiles.push_back(t);
            work.push_back((int64_t)t.m * t.n * (b.ksum + 1));
        }
    }
    std::vector<int> order(tiles.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return work[a] > work[b]; });
    out = Tasks();
    out.tiles.resize(tiles.size());
    for (size_t i = 0; i < order.size(); ++i) out.tiles[i] = tiles[order[i]];
    out.ntiles = (int32_t)tiles.size();
    out.segs.swap(rep);
    out.nsegs = (int32_t)out.segs.size();
    out.flops = flops;
    if (out.segs.empty()) out.segs.push_back(zero_record<htn_seg>());
    if (out.tiles.empty()) out.tiles.push_back(zero_record<htn_tile>());
}

class TaskList {
public:
    std::vector<TLBlock> blocks;
    KeyMap idx;
    int block(const Key& key, int buf, int64_t off, int m, int n, int ld) {
        auto it = idx.find(key);
        if (it != idx.end()) return it->second;
        const int i = (int)blocks.size();
        idx[key] = i;
        blocks.push_back({buf, off, m, n, ld, {}});
        return i;
    }
    int find(const Key& key) const {
        auto it = idx.find(key);
        return it == idx.end() ? -1 : it->second;
    }
    void add(int bi, const SegRec& r) {
        auto& v = blocks[bi].segs;
        for (auto& s : v)
            if (s.same(r)) {          // segments with identical operands are merged (alpha summed), first position kept
                s.alpha += r.alpha;
                return;
            }
        v.push_back(r);
    }
    void gemm(int bi, int buf_a, int64_t a_off, int lda, int op_a, int buf_b, int64_t b_off, int ldb, int op_b, int k, cplx alpha) {
        add(bi, {HTN_SEG_GEMM, buf_a, a_off, lda, op_a, buf_b, b_off, ldb, op_b, k, alpha});
    }
    void copy(int bi, int buf_b, int64_t b_off, int ldb, cplx alpha) {
        add(bi, {HTN_SEG_COPY, 0, 0, 1, HTN_OP_N, buf_b, b_off, ldb, HTN_OP_N, 0, alpha});
    }
    void finalize(Tasks& out) {
        std::vector<htn_seg> segs;
        std::vector<BRow> B;
        int64_t flops = 0;
        for (auto& b : blocks) {
            const int64_t pos = (int64_t)segs.size();
            int64_t ncopy = 0, ksum = 0;
            for (int pass = 0; pass < 2; ++pass)            // GEMM segments first, COPY segments last (stable)
                for (auto& s : b.segs) {
                    if (s.alpha == cplx(0.0, 0.0)) continue;
                    if ((s.type == HTN_SEG_GEMM) != (pass == 0)) continue;
                    segs.push_back(s.record());
                    if (s.type == HTN_SEG_GEMM) ksum += s.k;
                    else ++ncopy;
                }
            flops += 8 * (int64_t)b.m * b.n * ksum;
            B.push_back({b.off, b.buf, b.ld, b.m, b.n, pos, (int64_t)segs.size() - pos, ncopy, ksum});
        }
        emit_tasks(segs, B, flops, out);
    }
};

inline Key tkey(Sec a, int s1, Sec c, int s2, Sec b) { return mk(a.N, a.j, s1, c.N, c.j, s2, b.N, b.j); }

}  // namespace htn
