// Load balance of one grouped-GEMM launch: split-K across workgroups + placement-aware order (balance_tiles, htn_core.h).
// Host C++ (no HIP).
// NOT a translation unit of its own: #included by htn_plan.cpp (one unit, see its head); never name it on a build line.
//
// Cost model of k_grouped_gemm_z (htn_gemm.hip): a tile is one 4-wave workgroup, one wave per SIMD; a tile with q = 1, 2
// or 4 quadrants splits its S slabs 4 / q ways, so it keeps each SIMD of its CU busy for ceil(S q / 4) slab units (16 MFMAs,
// ~0.6 us at the clock the chip holds under MFMA load).  A launch is bound by the most loaded CU, and where a workgroup lands
// is deterministic while every CU still has a free slot (measured, tools/gemm_prof.py): workgroup p goes to XCD p % 8 and,
// inside the XCD, to its CUs in a fixed rotation -- workgroup 256 + j lands on the CU of workgroup j.  Hence:
//   1. tiles whose load exceeds the cap (a fraction of the balanced share of a CU) are cut: first spatially into their
//      quadrants, then -- if one quadrant is still too long -- into parts along K (split-K across workgroups: the parts run
//      on different CUs and meet through the workspace, see the kernel; that hand-off costs several us);
//   2. the parts are dealt in LAYERS of n_cus: layer 0 = the n_cus longest, one per CU; every later layer gives each CU
//      one more part, longest part to the least loaded CU -- preferably a CU of the XCD where the part's output strip
//      already lives (operands then come out of that XCD's L2); GEMM_RESIDENT layers are co-resident (occupancy);
//   3. whatever does not fit those layers follows longest first: it is dispatched dynamically as slots free up.
#include "htn_core.h"

namespace htn {
namespace {

#define GEMM_RESIDENT 6      // workgroups of k_grouped_gemm_z co-resident per CU (its launch bounds: 6 waves per SIMD)

// tuning knobs of the environment, read once per process (0 / unset: the rule below decides)
struct Knobs {
    int cap, cap_k, xcd, layers;
};
const Knobs& knobs() {
    auto env = [](const char* name, int dflt) { return getenv(name) ? atoi(getenv(name)) : dflt; };
    static const Knobs k = {env("HTN_GEMM_CAP", 0), env("HTN_GEMM_CAPK", 0), env("HTN_GEMM_XCD", 1), env("HTN_GEMM_LAYERS", GEMM_RESIDENT)};
    return k;
}

inline int slabs(const htn_tile& T) { return std::max(0, T.seg_count - T.pad[0]); }
inline int ways(const htn_tile& T) { return 4 / ((T.m > 16 ? 2 : 1) * (T.n > 16 ? 2 : 1)); }
inline int load(const htn_tile& T) {
    const int g = ways(T);
    return (slabs(T) + g - 1) / g + 1;      // + 1: prologue / epilogue
}

// what flows from step to step
struct Launch {
    int n_cus, NX, per;                          // CU (x, k) <-> launch position 8 k + x of a layer
    std::vector<htn_tile> parts;                 // the records of the launch, after both cuts
    int ws = 0;                                  // workspace slabs handed to the K parts
    std::vector<int> order;                      // parts, longest first
    std::vector<std::vector<int>> layers;        // part indices of every resident layer, with the XCD each one goes to
    std::vector<std::vector<int>> layer_x;
    std::vector<char> used;                      // part is in a resident layer
    std::vector<std::vector<int>> cu_tiles;      // per CU: its part of layer 0, 1, ...
};

// 1a. spatial cut: a tile of 2 or 4 quadrants whose load exceeds the cap becomes 2 or 4 one-quadrant tiles sharing its
//     segment list (same MFMA work, spread over 2 or 4 CUs; every one of them splits K four ways; nothing to reduce).
//     (Holding the cuts back so that the launch fits the chip at once -- 1024 workgroups -- was measured slower, 26.3 vs
//     24.4 us at chi = 1024: the tiles left whole cost more than the ~60 workgroups that start late.)
std::vector<htn_tile> cut_quadrants(const Tasks& t, int cap) {
    std::vector<htn_tile> src;
    src.reserve((size_t)t.ntiles * 2);
    for (int i = 0; i < t.ntiles; ++i) {
        const htn_tile& T = t.tiles[i];
        const int g = ways(T);
        if (g == 4 || (slabs(T) + g - 1) / g <= cap) {
            src.push_back(T);
            continue;
        }
        for (int r0 = 0; r0 < T.m; r0 += 16)
            for (int c0 = 0; c0 < T.n; c0 += 16) {
                htn_tile Q = T;
                Q.row0 = T.row0 + r0, Q.col0 = T.col0 + c0;
                Q.m = std::min(16, T.m - r0), Q.n = std::min(16, T.n - c0);
                src.push_back(Q);
            }
    }
    return src;
}

// 1b. K cut: a tile still longer than cap_k (and a quarter) becomes parts of about cap_k slab units; the parts of one tile
//     share a ticket and a run of workspace slabs, both numbered in list order
void cut_k(const std::vector<htn_tile>& src, int cap_k, Launch& L) {
    L.parts.reserve(src.size() + 64);
    int tickets = 0;
    for (size_t i = 0; i < src.size(); ++i) {
        htn_tile T = src[i];
        T.part = 0, T.nparts = 1, T.ws_slot = 0, T.ticket = 0;
        const int S = slabs(T), g = ways(T), ld = (S + g - 1) / g;
        const int np = ld > cap_k + cap_k / 4 ? (ld + cap_k - 1) / cap_k : 1;
        if (np <= 1 || T.pad[1] == 0 || tickets >= HTN_WS_TICKET_ELEMS * 4 - 1) {
            L.parts.push_back(T);
            continue;
        }
        const int base = ld / np, extra = ld % np;         // slab units per part: the first `extra` parts take one more
        int pos = 0;
        for (int p = 0; p < np; ++p) {
            const int u = base + (p < extra ? 1 : 0);
            const int cnt = p == np - 1 ? S - pos : std::min(g * u, S - pos);
            htn_tile P = T;
            P.seg_begin = T.seg_begin + pos;
            P.seg_count = cnt + (p == np - 1 ? T.pad[0] : 0);     // COPY segments ride with the last part
            P.pad[0] = p == np - 1 ? T.pad[0] : 0;
            P.part = p, P.nparts = np, P.ws_slot = L.ws, P.ticket = tickets;
            L.parts.push_back(P);
            pos += cnt;
        }
        L.ws += np;
        ++tickets;
    }
}

// 2a. the resident layers and the XCD of every part in them: its strip's home if that XCD still has room in the layer
void deal_layers(Launch& L) {
    const int n = (int)L.parts.size(), NX = L.NX;
    L.order.resize(n);
    for (int i = 0; i < n; ++i) L.order[i] = i;
    std::stable_sort(L.order.begin(), L.order.end(), [&](int a, int b) { return load(L.parts[a]) > load(L.parts[b]); });
    const int n_layers = std::min(std::max(knobs().layers, 1), (n + L.n_cus - 1) / L.n_cus);
    std::vector<int64_t> x_load(NX, 0);
    std::unordered_map<Key, int, KeyHash> home;
    L.used.assign((size_t)n, 0);
    int next = 0;
    for (int l = 0; l < n_layers; ++l) {
        const int cnt = std::min(L.n_cus, n - next);
        std::vector<int> room(NX, L.per), xs(cnt), li(cnt);
        if (cnt < L.n_cus)            // last, partial layer: launch positions are filled in order, XCD x gets ceil / floor
            for (int x = 0; x < NX; ++x) room[x] = cnt / NX + (x < cnt % NX ? 1 : 0);
        for (int j = 0; j < cnt; ++j) {
            const htn_tile& T = L.parts[L.order[next + j]];
            const Key k = mk(T.buf_c, (int32_t)(T.c_off & 0x7fffffff), (int32_t)(T.c_off >> 31), T.row0);
            auto it = home.find(k);
            int x = it == home.end() ? -1 : it->second;
            if (x < 0 || room[x] == 0) {
                int y = -1;
                for (int c = 0; c < NX; ++c)
                    if (room[c] > 0 && (y < 0 || x_load[c] < x_load[y])) y = c;
                if (x < 0) home[k] = y;
                x = y;
            }
            --room[x];
            xs[j] = x;
            li[j] = L.order[next + j];
            L.used[li[j]] = 1;
            x_load[x] += load(T);
        }
        next += cnt;
        L.layers.push_back(li);
        L.layer_x.push_back(xs);
    }
}

// 2b. inside the XCD: longest part of the layer to the least loaded CU that has no part of this layer yet
void place_in_xcd(Launch& L) {
    std::vector<int64_t> cu_load((size_t)L.n_cus, 0);
    L.cu_tiles.assign((size_t)L.n_cus, {});
    for (size_t l = 0; l < L.layers.size(); ++l) {
        const std::vector<int>& li = L.layers[l];
        std::vector<int> idx(li.size());
        for (size_t j = 0; j < idx.size(); ++j) idx[j] = (int)j;
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return load(L.parts[li[a]]) > load(L.parts[li[b]]); });
        std::vector<char> taken((size_t)L.n_cus, 0);
        for (int j : idx) {
            const int i = li[j], x = L.layer_x[l][j];
            int best = -1;
            for (int k = 0; k < L.per; ++k) {
                const int c = k * L.NX + x;
                if (!taken[c] && (best < 0 || cu_load[c] < cu_load[best])) best = c;
            }
            taken[best] = 1;
            L.cu_tiles[best].push_back(i);
            cu_load[best] += load(L.parts[i]);
        }
    }
}

// 3. launch order: CUs that take part in the last (possibly partial) layer come first inside their XCD -- the rotation of
//    an XCD restarts at its first CU with every layer; what is in no resident layer follows, longest first
std::vector<htn_tile> launch_order(const Launch& L) {
    std::vector<std::vector<int>> cus(L.NX);
    for (int x = 0; x < L.NX; ++x) {
        for (int k = 0; k < L.per; ++k) cus[x].push_back(k * L.NX + x);
        std::stable_sort(cus[x].begin(), cus[x].end(),
                         [&](int a, int b) { return L.cu_tiles[a].size() > L.cu_tiles[b].size(); });
    }
    std::vector<htn_tile> fin;
    fin.reserve(L.parts.size());
    for (size_t l = 0; l < L.layers.size(); ++l)
        for (int k = 0; k < L.per; ++k)
            for (int x = 0; x < L.NX; ++x) {
                const int c = cus[x][k];
                if (L.cu_tiles[c].size() > l) fin.push_back(L.parts[L.cu_tiles[c][l]]);
            }
    for (int i : L.order)
        if (!L.used[i]) fin.push_back(L.parts[i]);
    return fin;
}

}  // namespace

int balance_tiles(Tasks& t, int n_cus) {
    const int nt = t.ntiles;
    if (nt <= 0) return 0;
    int64_t total = 0;
    for (int i = 0; i < nt; ++i) total += load(t.tiles[i]);
    const int64_t share = (total + n_cus - 1) / n_cus;        // balanced load of one CU
    // spatial cut: no hand-off, so a small fraction of the share -- but only while the launch has fewer workgroups than the
    // CUs can hold (4 per CU): beyond that more workgroups add prologues and operand re-reads, not parallelism
    const int slots = GEMM_RESIDENT * n_cus;                   // workgroups the chip holds at once
    int cap = nt >= slots ? (1 << 30) : std::max((int)(2 * share / 5), 4);
    int cap_k = std::max((int)share, 12);                       // K cut: the hand-off costs several us
    if (knobs().cap > 0) cap = knobs().cap;
    if (knobs().cap_k > 0) cap_k = knobs().cap_k;
    Launch L;
    L.n_cus = n_cus;
    L.NX = (knobs().xcd && n_cus % 8 == 0) ? 8 : 1;
    L.per = n_cus / L.NX;
    cut_k(cut_quadrants(t, cap), cap_k, L);
    deal_layers(L);
    place_in_xcd(L);
    t.tiles = launch_order(L);
    t.ntiles = (int32_t)t.tiles.size();
    return L.ws;
}

}  // namespace htn
