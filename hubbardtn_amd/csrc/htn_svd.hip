// batched Jacobi SVD + strided copy kernels (libhubbardtn_hip.so)
//
// ONE translation unit: this file holds the host driver and #includes the kernels, one piece per path (the pieces are not
// units of their own: the compiler sees what it saw when all of it was one file).  Which block goes where is decided on the
// host, by htn_jacobi_svd_z, jacobi_svd_tall and jacobi_svd_core below:
//
//   block                                                          path                     piece
//   ------------------------------------------------------------   ----------------------   ------------------
//   at most 512 rows; plain, or QRCP with padded rows x columns    one workgroup:           htn_svd_one.h
//     inside the LDS window (JAC_LDS_ELEMS, classify_large)          k_jacobi_svd             (rotations, sweep loops, SplitCols /
//                                                                                             DenseCols: htn_svd_cols.h; its QRCP,
//                                                                                             qrcp_mgs: htn_svd_qr.h)
//   QRCP, at most 512 rows, larger than the window ("large")       k_qr_large first,        htn_svd_qr.h
//     then, by default, when plan_ring finds CU slots for all        the ring:                htn_svd_ring.h
//     large blocks of the call                                       k_jacobi_ring
//     otherwise, or with HTN_SVD_PAIRS=1                             pair visits:             htn_svd_visits.h
//                                                                    k_jacobi_pairs_gram,
//                                                                    k_jacobi_check, k_jacobi_finish
//   plain (non-QRCP), more than 512 rows ("tall")                  tall visits:             htn_svd_visits.h
//                                                                    k_jacobi_tall_*,
//                                                                    k_jacobi_check
//   QRCP with more than 512 rows                                   refused
//
// Pair visits and tall visits share the tournament (jacobi_tournament), the sweep pipeline (jacobi_sweep_pipeline) and the
// 16 x 16 Gram-visit core (jg_* in htn_svd_visits.h).  Every path stops its sweeps by ONE rule, jacobi_last_sweep
// (htn_svd_cols.h), from two numbers per block and sweep: the largest squared cosine the sweep saw before its rotations and
// the largest tan^2 it rotated by -- kept in LDS by the one-workgroup kernel, in two 64-bit words per block by the visits
// (integer maxima on the bit patterns, read and zeroed by k_jacobi_check) and by the ring (its sync block).
// htn_batched_copy.h (k_batched_copy, htn_batched_copy_z) is unrelated
// to the SVD and only lives in this unit.
#include <algorithm>
#include <utility>
#include <vector>

#include "htn_common.h"

// Phase ticks of the diagnostic builds (100 MHz constant clock): JAC_T(ON, var) takes a stamp, JAC_ACC(ON, arr, slot, a, b)
// adds b - a to arr[slot] of the build's tick array.  ON is QR_PROF (k_qr_large, -DHTN_QR_PROF) or RING_PROF (k_jacobi_ring,
// -DHTN_RING_PROF): 1 in that build only, and where it is 0 both expand to nothing.
#ifdef HTN_QR_PROF
#define QR_PROF 1
#else
#define QR_PROF 0
#endif
#ifdef HTN_RING_PROF
#define RING_PROF 1
#else
#define RING_PROF 0
#endif
#define JAC_T_1(var) const long long var = wall_clock64()
#define JAC_T_0(var)
#define JAC_ACC_1(arr, slot, a, b) arr[slot] += (b) - (a)
#define JAC_ACC_0(arr, slot, a, b)
#define JAC_PICK_(name, on) name##on
#define JAC_PICK(name, on) JAC_PICK_(name, on)
#define JAC_T(on, var) JAC_PICK(JAC_T_, on)(var)
#define JAC_ACC(on, arr, slot, a, b) JAC_PICK(JAC_ACC_, on)(arr, slot, a, b)

#include "htn_svd_cols.h"
#include "htn_svd_qr.h"
#include "htn_svd_one.h"
#include "htn_svd_visits.h"
#include "htn_svd_ring.h"

// per-stream scratch of the multi-launch path (grown on demand; htn_common.h: owned by the stream's registry entry and
// released by the backend that owns the stream)
struct JacScratch {
    int device = -1;
    int cu_count = 0;
    int xcd_local = 0;                  // 1: in the last ring launch every block's workgroups found themselves on one XCD
    HtnBuf dev{HTN_BUF_DEVICE};         // [large_ids | slot of every block | perm | zero2 | ratio | done | sweeps | qsync | items]
    HtnBuf pinned{HTN_BUF_PINNED};      // host -> device staging (work lists, ids)
    HtnBuf flags{HTN_BUF_MAPPED};       // device -> host: [active count per sweep | rank per large block | ring sweeps]; its own block
    // ring Jacobi: flags / arrival counters / maxima, and the work items with their pinned staging.  Not poisoned: the part
    // of either that a launch reads is zeroed / uploaded on the stream in front of that launch, at every call.
    HtnBuf ring_sync{HTN_BUF_DEVICE, false};
    HtnBuf ring_items{HTN_BUF_DEVICE, false};
    HtnBuf ring_items_h{HTN_BUF_PINNED};
    HtnBuf ring_mbox{HTN_BUF_DEVICE};   // ring Jacobi: mailboxes
    HtnBuf qr_box{HTN_BUF_DEVICE};      // k_qr_large with helper workgroups: per-block panel basis / column map / norms (sc1 traffic)
    HtnBuf tall_dev{HTN_BUF_DEVICE};    // tall-block path: [skip | ids | zero2 | partials | ratio | done | sweeps | items]
    HtnBuf tall_pin{HTN_BUF_PINNED};    // its host -> device staging: [items | skip | ids]
    HtnBuf tall_flags{HTN_BUF_MAPPED};  // device -> host: active tall blocks per sweep
    hipStream_t aux = nullptr;          // forked stream: small blocks run beside the large-block pipeline
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_sweep[2] = {nullptr, nullptr};
    // only what the members cannot do: their device, and the forked stream drained before the buffers go (they free after
    // this body, in reverse order of declaration)
    ~JacScratch() {
        if (device >= 0) (void)hipSetDevice(device);
        if (aux) {
            (void)hipStreamSynchronize(aux);
            (void)hipStreamDestroy(aux);
        }
        for (hipEvent_t ev : {ev_fork, ev_join, ev_sweep[0], ev_sweep[1]})
            if (ev) (void)hipEventDestroy(ev);
    }
};
static HtnStreamRegistry<JacScratch> g_js_res;

void htn_svd_release_stream(hipStream_t st) { g_js_res.release(st); }

static int js_get(hipStream_t st, JacScratch** out) {
    return g_js_res.get(st, out, [](JacScratch& js) -> int {
        HIP_TRY(hipDeviceGetAttribute(&js.cu_count, hipDeviceAttributeMultiprocessorCount, js.device));
        HIP_TRY(hipStreamCreateWithFlags(&js.aux, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&js.ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&js.ev_join, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&js.ev_sweep[0], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&js.ev_sweep[1], hipEventDisableTiming));
        return 0;
    });
}

// ---- the pieces both multi-launch paths (pair visits of large blocks, tall blocks) share ---------------------------------
// Panel-pair work lists of one outer sweep, one per round of the round-robin tournament over the panels of JAC_PANEL
// columns of each block: round r is items[off[r] .. off[r + 1]), one launch.  The order of the rounds and of the items in
// a round fixes which pairs meet in which launch, hence the bits of the result.
struct JacTournament {
    std::vector<JacPairItem> items;
    std::vector<size_t> off;
    int n_rounds() const { return (int)off.size() - 1; }
    unsigned round_size(int r) const { return (unsigned)(off[r + 1] - off[r]); }
};
static JacTournament jacobi_tournament(const int* n_cols, int n_blk) {
    const int w = JAC_PANEL;
    std::vector<std::vector<JacPairItem>> rounds;
    std::vector<JacPairItem> intra;
    for (int li = 0; li < n_blk; ++li) {
        const int n = n_cols[li];
        if (n < 1) continue;
        const int nb = (n + w - 1) / w;
        const int nbp = nb + (nb & 1);
        if ((int)rounds.size() < nbp - 1) rounds.resize(nbp - 1);
        for (int r = 0; r < nbp - 1; ++r)
            for (int p = 0; p < nbp / 2; ++p) {
                int a = p == 0 ? nbp - 1 : (r + p) % (nbp - 1);
                int c = p == 0 ? r : (r + nbp - 1 - p) % (nbp - 1);
                if (a >= nb || c >= nb) continue;
                if (a > c) std::swap(a, c);
                JacPairItem it = {li, a * w, std::min(w, n - a * w), c * w, std::min(w, n - c * w), {0, 0, 0}};
                rounds[r].push_back(it);
            }
        // the pairs inside each panel, two panels per workgroup, once per outer sweep
        for (int a = 0; a < nb; a += 2) {
            const int c = a + 1;
            JacPairItem it = {li, a * w, std::min(w, n - a * w), c < nb ? c * w : 0,
                              c < nb ? std::min(w, n - c * w) : 0, {1, 0, 0}};
            intra.push_back(it);
        }
    }
    // the intra-panel visit closes the sweep: one outer sweep fewer than with it in front (measured on graded
    // spectra and in the DMRG sweep; the cross visits leave the panels' own pairs slightly non-orthogonal)
    rounds.push_back(intra);
    JacTournament T;
    for (auto& rl : rounds) {
        T.off.push_back(T.items.size());
        T.items.insert(T.items.end(), rl.begin(), rl.end());
    }
    T.off.push_back(T.items.size());
    return T;
}
// through the pinned staging block, ONE copy on the stream
static int upload_tournament(const JacTournament& T, JacPairItem* h_items, JacPairItem* d_items, hipStream_t st) {
    if (T.items.empty()) return 0;
    memcpy(h_items, T.items.data(), sizeof(JacPairItem) * T.items.size());
    HIP_TRY(hipMemcpyAsync(d_items, h_items, sizeof(JacPairItem) * T.items.size(), hipMemcpyHostToDevice, st));
    return 0;
}

// Outer sweeps, enqueued one ahead of the host's knowledge (depth-1 pipeline, like htn_lanczos_z): the device decides
// convergence itself (k_jacobi_check writes h_active[sweep]), the host only learns when to stop enqueuing.  enqueue(sweep)
// launches one sweep and its check on `st`; its end is marked here with ev_sweep[sweep & 1].
// Speculation is bounded by the caller's expectation (htn_svd_opts.sweeps_hint, normally what the previous update of
// the same bond needed): the sweep expected to be the last is NOT followed by a speculative one -- an outer sweep that
// finds every block done still costs its launches (26 x 4.5 us at chi = 1024).  A wrong hint costs one host round trip
// per extra sweep instead.
// Returns the sweeps used, -1 after a HIP error (recorded like HIP_TRY does).
template <class Enqueue>
static int jacobi_sweep_pipeline(int max_sweeps, int hint, hipEvent_t* ev_sweep, const volatile int* h_active,
                                 hipStream_t st, Enqueue enqueue) {
    hipError_t err = hipSuccess;
    int enq = 0, used = 0;
    auto enqueue_next = [&]() {
        enqueue(enq);
        err = hipEventRecord(ev_sweep[enq & 1], st);
        ++enq;
    };
    if (max_sweeps > 0) enqueue_next();
    for (int sweep = 0; sweep < max_sweeps && err == hipSuccess; ++sweep) {
        const bool expect_last = hint > 0 && sweep + 1 >= hint;
        if (sweep + 1 < max_sweeps && !expect_last && enq == sweep + 1) enqueue_next();
        if (err == hipSuccess) err = htn_event_spin(ev_sweep[sweep & 1]);
        if (err != hipSuccess) break;
        used = sweep + 1;
        if (h_active[sweep] == 0) break;
        if (sweep + 1 < max_sweeps && enq == sweep + 1) enqueue_next();
    }
    return err == hipSuccess ? used : -htn_fail("jacobi_sweep_pipeline", err);
}

// ---- blocks of at most 512 rows -------------------------------------------------------------------------------------------
// what every phase of one call needs
struct JacCall {
    double2 *G, *Vj;
    double* S;
    const htn_svd_block *desc, *desc_host;
    int n_blocks, max_sweeps;
    double tol, cut2;            // cut2: square of htn_svd_opts.rank_cut (0: none)
    int split;                   // htn_svd_opts.split_elems (test mode), 0: off
    int32_t* info_dev;
    hipStream_t st;
    std::vector<int> large;      // blocks of the multi-launch path, in batch order
    std::vector<int> n_eff;      // their columns taking part (the rank the QR found, with a rank cut)
    int nl() const { return (int)large.size(); }
};
static int jac_padded_rows(int m) {
    const int gsx = m <= 16 * JAC_MAXEL ? 16 : (m <= 32 * JAC_MAXEL ? 32 : 64);
    return gsx * ((m + gsx - 1) / gsx);
}
// dynamic LDS window of k_jacobi_svd for the matrix: 144 KiB leaves room for the static shared variables
static const int JAC_LDS_ELEMS = 9216;     // complex128 elements = 144 KiB

// one-time kernel attributes: per device and thread safe (the attribute lives with the device's code object)
static int jac_set_kernel_attributes() {
    static std::mutex attr_mu;
    static bool attr_set[64] = {};
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(attr_mu);
    if (dev >= 0 && dev < 64 && !attr_set[dev]) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_jacobi_svd, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    JAC_LDS_ELEMS * (int)sizeof(double2)));
        HIP_TRY(hipFuncSetAttribute((const void*)k_qr_large, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    16 * (64 * JAC_MAXEL + 1) * (int)sizeof(double2)));
        HIP_TRY(hipFuncSetAttribute((const void*)k_jacobi_pairs_gram, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (16 * (64 * JAC_MAXEL + 1) + JG_GU_ELEMS) * (int)sizeof(double2)));
        HIP_TRY(hipFuncSetAttribute((const void*)k_jacobi_ring, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    2 * RING_PANEL_ELEMS * (int)sizeof(double2)));
        attr_set[dev] = true;
    }
    return 0;
}

// blocks that do not fit one CU's LDS go to the multi-launch block-Jacobi path (needs the host copy of desc)
static std::vector<int> classify_large(const htn_svd_block* desc_host, int n_blocks, int split) {
    const int large_min = split > 0 ? std::min(split, JAC_LDS_ELEMS) : JAC_LDS_ELEMS;
    std::vector<int> large;
    if (desc_host)
        for (int b = 0; b < n_blocks; ++b) {
            const htn_svd_block& D = desc_host[b];
            if (!(D.flags & HTN_SVD_QRCP) || D.n < 2) continue;
            if ((int64_t)jac_padded_rows(D.m) * D.n > large_min) large.push_back(b);
        }
    return large;
}

// the scratch of one call, carved from the stream's blocks
struct JacCoreBufs {
    // device: [large_ids | slot of every block | perm | zero2 | ratio | done | sweeps | qsync | items]
    int *d_ids, *d_slot, *d_perm;
    double* d_zero;
    unsigned long long* d_ratio;      // per block: [largest squared cosine | largest tan^2] of the sweep, as bits
    int *d_done, *d_sw;
    unsigned* d_qsync;           // QR_SYNC_WORDS per block + failure word
    JacPairItem* d_items;
    // pinned staging (host -> device): [items | ids | slot of every block]
    JacPairItem* h_items;
    int *h_ids, *h_slot;         // [ids | slot] contiguous like the device copy: ONE upload
    // device -> host flags (their own coherent block, read by the host only behind a completed event):
    // [active count per sweep | rank per large block | ring path: outer sweeps per large block (0: the launch failed)]
    volatile int *h_active, *h_rank, *h_ring_sw;
    int *d_active, *d_rank, *d_ring_sw;
};
static int carve_core_scratch(JacScratch& js, int nl, int n_blocks, int max_sweeps, size_t n_items_max, JacCoreBufs* B) {
    const size_t off_ids = 0, off_slot = off_ids + sizeof(int) * nl, off_perm = off_slot + sizeof(int) * n_blocks;
    const size_t off_zero = off_perm + sizeof(int) * nl * 64 * JAC_MAXEL;
    const size_t off_ratio = (off_zero + sizeof(double) * nl + 7) / 8 * 8, off_done = off_ratio + 16 * nl;      // ratio: 2 words per block
    const size_t off_sw = off_done + sizeof(int) * nl, off_qsync = off_sw + sizeof(int) * nl;
    const size_t off_items = (off_qsync + sizeof(unsigned) * (QR_SYNC_WORDS * (size_t)nl + 8) + 31) / 32 * 32;
    if (js.dev.reserve(off_items + sizeof(JacPairItem) * n_items_max)) return 1;
    if (js.pinned.reserve(sizeof(JacPairItem) * n_items_max + 4 * (size_t)(nl + n_blocks) + 128)) return 1;
    if (js.flags.reserve(sizeof(int) * ((size_t)(max_sweeps + 1) + 2 * (size_t)nl + 16))) return 1;
    char* d = (char*)js.dev.p;
    B->d_ids = (int*)(d + off_ids);
    B->d_slot = (int*)(d + off_slot);
    B->d_perm = (int*)(d + off_perm);
    B->d_zero = (double*)(d + off_zero);
    B->d_ratio = (unsigned long long*)(d + off_ratio);
    B->d_done = (int*)(d + off_done);
    B->d_sw = (int*)(d + off_sw);
    B->d_qsync = (unsigned*)(d + off_qsync);
    B->d_items = (JacPairItem*)(d + off_items);
    char* h = (char*)js.pinned.p;
    B->h_items = (JacPairItem*)h;
    B->h_ids = (int*)(h + sizeof(JacPairItem) * n_items_max);
    B->h_slot = B->h_ids + nl;
    B->h_active = (volatile int*)js.flags.p;
    B->h_rank = B->h_active + (max_sweeps + 1);
    B->h_ring_sw = B->h_rank + nl;
    B->d_active = (int*)js.flags.dev;
    B->d_rank = B->d_active + (max_sweeps + 1);
    B->d_ring_sw = B->d_rank + nl;
    return 0;
}

// Ring path: CU slots and panel width of every large block; batches of <= #CU workgroups (all workgroups of a launch must
// be co-resident: they wait for each other).
struct RingPlan {
    std::vector<RingItem> items;                     // in GRID order of their launch (gaps: P = 0)
    std::vector<std::pair<int, int>> batches;        // (first item, grid size) of each launch
    int wgs = 0;                                     // workgroups with work (flag / id words are indexed densely)
    int64_t mbox_elems = 0;
};
// n_xcd > 1: XCD-aware placement (see jacobi_svd_core); ring_cap: CU slots of the chip.  false: some block needs more
// slots than the ring supports.
static bool plan_ring(const JacCall& c, int n_xcd, int ring_cap, RingPlan* plan) {
    *plan = RingPlan();
    struct Blk {
        int li, P, w, mp;
    };
    std::vector<Blk> blks;
    for (int li = 0; li < c.nl(); ++li) {
        const htn_svd_block& D = c.desc_host[c.large[li]];
        const int gsx = ring_gs(D.m);
        const int mp = gsx * ring_e(D.m);
        int wcap = std::min(RING_THREADS / gsx, RING_PANEL_ELEMS / mp);
        if (gsx == 16 && wcap > 16 && wcap < 32) wcap = 16;      // 16 pairs = one busy wave per SIMD; 17..31 would put two on one
        if (c.split > 0) wcap = std::min(wcap, 3);               // test mode: small blocks still get several CU slots
        const int n = std::max(c.n_eff[li], 1);
        const int P = std::max(1, (n + 2 * wcap - 1) / (2 * wcap));
        if (wcap < 1 || P > RING_MAX_P || P > ring_cap) return false;
        blks.push_back({li, P, (n + 2 * P - 1) / (2 * P), mp});
    }
    std::stable_sort(blks.begin(), blks.end(), [](const Blk& a, const Blk& b) { return a.P > b.P; });
    std::vector<char> placed(blks.size(), 0);
    size_t left = blks.size();
    int nx = n_xcd;                                       // (a block with more slots than one XCD has CUs: dense placement)
    for (const Blk& B : blks)
        if (B.P > ring_cap / nx) nx = 1;
    const int lane_cap = ring_cap / nx;                   // CU slots of one XCD (of the chip when nx = 1)
    while (left) {
        const int first = (int)plan->items.size();
        std::vector<int> lane_used((size_t)nx, 0);
        struct Put {
            int q, x, s0;
        };
        std::vector<Put> puts;
        for (size_t q = 0; q < blks.size(); ++q) {
            if (placed[q]) continue;
            int x = 0;
            for (int y = 1; y < nx; ++y)
                if (lane_used[y] < lane_used[x]) x = y;
            if (lane_used[x] + blks[q].P > lane_cap) continue;
            puts.push_back({(int)q, x, lane_used[x]});
            lane_used[x] += blks[q].P;
            placed[q] = 1;
            --left;
        }
        int depth = 0;
        for (int y = 0; y < nx; ++y) depth = std::max(depth, lane_used[y]);
        const int grid = depth * nx;
        plan->items.resize((size_t)first + grid, RingItem{0, 0, 0, 0, 0, 0, 0});
        for (const Put& pt : puts) {
            const Blk& B = blks[pt.q];
            for (int k = 0; k < B.P; ++k)
                plan->items[(size_t)first + (size_t)(pt.s0 + k) * nx + pt.x] = {B.li, k, B.P, B.w, c.n_eff[B.li], plan->wgs,
                                                                                 plan->mbox_elems};
            plan->mbox_elems += (int64_t)B.P * 4 * B.w * B.mp;
            plan->wgs += B.P;
        }
        plan->batches.push_back({first, grid});
    }
    return true;
}

// pivoted QR of the large blocks on the call's stream: helper count, LDS size, the helpers' exchange block, the launch
static int launch_qr_large(const JacCall& c, JacScratch& js, const JacCoreBufs& B, int n_xcd) {
    const int nl = c.nl();
    int max_m0 = 0, min_m0 = 1 << 30, max_n0 = 0;
    for (int b : c.large) {
        max_m0 = std::max(max_m0, (int)c.desc_host[b].pad);
        min_m0 = std::min(min_m0, (int)c.desc_host[b].pad);
        max_n0 = std::max(max_n0, (int)c.desc_host[b].m);
    }
    const size_t qr_panel_elems = (size_t)16 * (((max_m0 + 15) & ~15) + 1);
    // + 64 KiB for the partial tiles of the cooperative trailing update, when some block is small enough to use them and the
    // panel of the largest leaves the room
    const bool coop = ((min_m0 + 15) & ~15) <= 256 && qr_panel_elems * sizeof(double2) + 65536 + 30720 <= 163840;
    const size_t qr_lds = qr_panel_elems * sizeof(double2) + (coop ? 65536 : 0);
    // workgroups per block: the master + helpers for the trailing update (all co-resident: they wait for each other)
    static const bool qr_single = htn_env_flag("HTN_QR_SINGLE");
    // Measured (tools/ring_prof.py, HTN_QR_PROF): in the placement-independent form every shared byte goes to memory and
    // comes back from memory (sc1), so a chunk's operand loads wait ~2 us each instead of an L2 hit: 202 x 202 blocks LOSE
    // (trailing 483 -> 655 us with four workgroups), 400 x 400 blocks gain (3.0 -> 2.3 ms).
    static const int env_nw = getenv("HTN_QR_NW") ? atoi(getenv("HTN_QR_NW")) : 0;      // (experiments: helpers at any size)
    // Helpers (profiles/r03_ring_qr_phase_times.txt): from 160 columns on always (202 x 202: 855 us alone, 697 with four
    // workgroups through memory, 623 through one XCD's L2; 400 x 400: 3.9 -> 2.5 ms); below, only while the kernels keep
    // finding a block's workgroups on one XCD (100 x 100: 266 -> 253 us through the L2).
    int NW = qr_single ? 1 : ((max_n0 >= 160 || js.xcd_local) ? 4 : 1);
    if (env_nw > 0 && !qr_single) NW = std::min(env_nw, 4);
    // placement: the workgroups of a block at grid positions of one residue mod 8 (see k_qr_large); the gaps count
    // against the co-residency bound like everything else
    const int cus = std::max(1, std::min(js.cu_count > 0 ? js.cu_count : 256, 256));
    const int qnx = (NW > 1 && n_xcd > 1) ? n_xcd : 1;
    const int nl_pad = (nl + qnx - 1) / qnx * qnx;
    NW = std::max(1, std::min(NW, cus / std::max(nl_pad, 1)));
    if (NW > 1 && js.qr_box.reserve((size_t)nl * QR_BOX_BYTES)) return 1;
    const int qgrid_nx = NW > 1 ? qnx : 1;
    hipLaunchKernelGGL(k_qr_large, dim3((NW > 1 ? nl_pad : nl) * NW), dim3(JAC_THREADS), qr_lds, c.st, c.G, c.Vj, c.desc, B.d_ids,
                       B.d_perm, B.d_zero, c.cut2, B.d_rank, NW, (char*)js.qr_box.p, B.d_qsync, nl, qgrid_nx,
                       coop ? (int)qr_panel_elems : 0);
    return 0;
}

// Ring path: all sweeps of the large blocks in one launch per batch, then the join with the small blocks and the host's
// look at the sweep counts
static int run_ring(const JacCall& c, JacScratch& js, const JacCoreBufs& B, const RingPlan& plan, int n_xcd, bool two_partner,
                    bool staged_send, int32_t* sweeps_used) {
    const int nl = c.nl(), n_wg = plan.wgs, n_items = (int)plan.items.size();
    // sync block (32-bit words): [flags: 2 per workgroup | arrivals: nl x max_sweeps | failure word | XCD ids: 1 per
    // workgroup | pad] then the 64-bit maxima, 2 x nl x max_sweeps; zeroed as ONE block that starts its allocation and is a
    // multiple of 16 bytes.  Two maxima per block and sweep: squared cosine, tan^2 (jacobi_last_sweep).
    const int arrive_off = 2 * n_wg, fail_off = arrive_off + nl * c.max_sweeps, xcc_off = fail_off + 1;
    const int conv_off = (xcc_off + n_wg + 3) & ~3;
    const size_t sync_bytes = ((size_t)conv_off * 4 + (size_t)nl * c.max_sweeps * 16 + 15) & ~(size_t)15;
    if (js.ring_sync.reserve(sync_bytes)) return 1;
    if (js.ring_mbox.reserve(sizeof(double2) * (size_t)std::max<int64_t>(plan.mbox_elems, 1))) return 1;
    if (js.ring_items.reserve(sizeof(RingItem) * n_items) || js.ring_items_h.reserve(sizeof(RingItem) * n_items)) return 1;
    memcpy(js.ring_items_h.p, plan.items.data(), sizeof(RingItem) * n_items);
    for (int li = 0; li < nl; ++li) B.h_ring_sw[li] = 0;
    HIP_TRY(hipMemcpyAsync(js.ring_items.p, js.ring_items_h.p, sizeof(RingItem) * n_items, hipMemcpyHostToDevice, c.st));
    HIP_TRY(hipMemsetAsync(js.ring_sync.p, 0, sync_bytes, c.st));
    RingArgs ra;
    ra.Vj = c.Vj, ra.G = c.G, ra.S = c.S, ra.desc = c.desc, ra.large_ids = B.d_ids;
    ra.perm = B.d_perm, ra.zero2 = B.d_zero, ra.mbox = (double2*)js.ring_mbox.p, ra.sync = (unsigned*)js.ring_sync.p;
    ra.arrive_off = arrive_off, ra.fail_off = fail_off, ra.conv_off = conv_off, ra.max_sweeps = c.max_sweeps, ra.tol = c.tol;
    ra.xcc_off = xcc_off;
    ra.two_partner = two_partner ? 1 : 0;
    ra.staged_send = staged_send ? 1 : 0;
    ra.info = c.info_dev, ra.sweeps_out = B.d_ring_sw;
    for (auto& bt : plan.batches) {
        ra.items = (const RingItem*)js.ring_items.p + bt.first;
        hipLaunchKernelGGL(k_jacobi_ring, dim3((unsigned)bt.second), dim3(RING_THREADS), 2 * RING_PANEL_ELEMS * sizeof(double2),
                           c.st, ra);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamWaitEvent(c.st, js.ev_join, 0));
    HIP_TRY(htn_stream_spin(c.st));      // the staging blocks are reused by the next call; the sweep counts are read below
    int used = 0;
    for (int li = 0; li < nl; ++li) {
        if (B.h_rank[li] < 0) return fail_msg("htn_jacobi_svd_z: a hand-off of the multi-workgroup QR timed out");
        if (B.h_ring_sw[li] <= 0 && c.n_eff[li] >= 2)
            return fail_msg("htn_jacobi_svd_z: a hand-off of the ring Jacobi kernel timed out");
        used = std::max(used, (int)B.h_ring_sw[li] % 1000);
    }
    // what the kernel saw of the placement steers the NEXT call's choice of QR helpers (below 160 columns they only pay
    // when the block's workgroups share an L2)
    int all_local = n_xcd > 1 ? 1 : 0;
    for (int li = 0; li < nl; ++li)
        if (c.n_eff[li] >= 2 && B.h_ring_sw[li] < 1000) all_local = 0;
    js.xcd_local = all_local;
    if (sweeps_used) *sweeps_used = used;
    return 0;
}

// Pair-visit path: one launch per tournament round and outer sweep, then the join with the small blocks and the finish
static int run_pair_visits(const JacCall& c, JacScratch& js, const JacCoreBufs& B, const JacTournament& T, int hint,
                           int32_t* sweeps_used) {
    const int nl = c.nl();
    int max_mp = 0;
    for (int b : c.large) max_mp = std::max(max_mp, jac_padded_rows(c.desc_host[b].m));
    const size_t gram_lds_bytes = (size_t)(16 * (max_mp + 1) + JG_GU_ELEMS) * sizeof(double2);
    const int used = jacobi_sweep_pipeline(c.max_sweeps, hint, js.ev_sweep, B.h_active, c.st, [&](int sweep) {
        for (int r = 0; r < T.n_rounds(); ++r)
            if (T.round_size(r))
                hipLaunchKernelGGL(k_jacobi_pairs_gram, dim3(T.round_size(r)), dim3(256), gram_lds_bytes, c.st, c.Vj, c.desc,
                                   B.d_ids, B.d_items + T.off[r], B.d_zero, B.d_ratio, B.d_done, c.tol, 1);
        hipLaunchKernelGGL(k_jacobi_check, dim3(1), dim3(64), 0, c.st, B.d_ratio, B.d_done, B.d_sw, nl, c.tol, B.d_active + sweep);
    });
    if (used < 0) return 1;
    if (sweeps_used) *sweeps_used = used;
    HIP_TRY(hipStreamWaitEvent(c.st, js.ev_join, 0));
    hipLaunchKernelGGL(k_jacobi_finish, dim3(nl), dim3(JAC_THREADS), 0, c.st, c.G, (const double2*)c.Vj, c.S, c.desc, B.d_ids,
                       B.d_perm, B.d_sw, B.d_done, c.info_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(htn_stream_spin(c.st));      // the pinned staging block is reused by the next call
    return 0;
}

// every block of at most 512 rows (QRCP or not); skip_dev / skip_host (n_blocks entries, NULL = none): blocks another path
// owns (the tall blocks), left untouched here
static int jacobi_svd_core(void* G, void* Vj, double* S, const htn_svd_block* desc, const htn_svd_block* desc_host,
                           int32_t n_blocks, int32_t max_m_host, int32_t max_sweeps, double tol, int32_t* info_dev,
                           const htn_svd_opts* opts, void* stream, const int* skip_dev, const unsigned char* skip_host) {
    if (n_blocks <= 0) return 0;
    if (max_m_host > 64 * JAC_MAXEL) return fail_msg("htn_jacobi_svd_z: block taller than 512 rows");
    // per-call settings (ABI 2): nothing process-wide is read or written here
    const double rank_cut = opts && opts->rank_cut > 0.0 ? opts->rank_cut : 0.0;
    JacCall c = {(double2*)G, (double2*)Vj, S, desc, desc_host, n_blocks, max_sweeps, tol, rank_cut * rank_cut,
                 opts && opts->split_elems > 0 ? opts->split_elems : 0, info_dev, (hipStream_t)stream, {}, {}};
    int32_t* sweeps_used = opts ? opts->sweeps_used : nullptr;
    if (jac_set_kernel_attributes()) return 1;
    c.large = classify_large(desc_host, n_blocks, c.split);
    if (sweeps_used) *sweeps_used = 0;
    if (c.large.empty()) {
        hipLaunchKernelGGL(k_jacobi_svd, dim3(n_blocks), dim3(JAC_THREADS), JAC_LDS_ELEMS * sizeof(double2), c.st, c.G, c.Vj, S,
                           desc, max_sweeps, tol, info_dev, JAC_LDS_ELEMS, skip_dev, c.cut2);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const int nl = c.nl();
    // the tournament is built AFTER the QR has been enqueued (and, with a rank cut, after it has reported the ranks):
    // room for the one of the full column counts
    size_t n_items_max = 0;
    for (int b : c.large) {
        const int nb = (desc_host[b].n + JAC_PANEL - 1) / JAC_PANEL, nbp = nb + (nb & 1);
        n_items_max += (size_t)(nbp - 1) * (nbp / 2) + (nb + 1) / 2;
        c.n_eff.push_back(desc_host[b].n);
    }
    JacScratch* jsp = nullptr;
    JacCoreBufs B;
    if (js_get(c.st, &jsp) || carve_core_scratch(*jsp, nl, n_blocks, max_sweeps, n_items_max, &B)) return 1;
    JacScratch& js = *jsp;
    for (int b = 0; b < n_blocks; ++b) B.h_slot[b] = skip_host && skip_host[b] ? nl : -1;
    for (int li = 0; li < nl; ++li) B.h_slot[c.large[li]] = li;
    for (int li = 0; li < nl; ++li) B.h_ids[li] = c.large[li];
    for (int k = 0; k <= max_sweeps; ++k) B.h_active[k] = 1;
    // every small copy / fill is a separate blit launch on the stream: they are enqueued BEFORE the QR (nothing here
    // depends on it unless a rank cut sizes the tournament), merged where the regions are contiguous
    HIP_TRY(hipMemcpyAsync(B.d_ids, B.h_ids, sizeof(int) * (nl + n_blocks), hipMemcpyHostToDevice, c.st));
    HIP_TRY(hipMemsetAsync(B.d_ratio, 0, 24 * (size_t)nl + sizeof(unsigned) * (QR_SYNC_WORDS * (size_t)nl + 8), c.st));      // ratio (16 nl) | done (4 nl) | sweeps (4 nl) | qsync
    // Ring path (default): all sweeps of the large blocks in one launch per batch of <= #CU workgroups.  The multi-launch
    // pair-visit path stays for blocks the ring cannot take (more CU slots than the chip has) and behind HTN_SVD_PAIRS=1.
    static const bool force_pairs = htn_env_flag("HTN_SVD_PAIRS");
    // XCD-aware placement: a block's workgroups go to grid positions 8 s + x with ONE x -- the dispatcher has been seen to
    // deal position p to XCD p mod 8 (tools/gemm_prof.py), so they share an L2 and the kernel, after CHECKING the XCD ids it
    // reads at run time, hands panels over through that L2.  Speed only: a block whose workgroups find themselves on
    // different XCDs uses the placement-independent hand-off.  HTN_RING_NO_XCD=1: dense placement, as before.
    static const bool no_xcd = htn_env_flag("HTN_RING_NO_XCD");
    // HTN_RING_STAGED_SEND=1: the panel exchange of the ring kernel staged through LDS (ring_send / ring_recv) instead of the
    // direct one (ring_send_col / ring_recv_cols); same bits, the reference for tests and phase times
    static const bool ring_staged = htn_env_flag("HTN_RING_STAGED_SEND");
    // HTN_RING_TWO_PARTNER=1: cross steps with two partner columns each (ring_cross; measured no faster);
    // read at every call, so one process can run both forms
    const bool ring_two_partner = htn_env_flag("HTN_RING_TWO_PARTNER");
    const int n_xcd = (!no_xcd && js.cu_count > 0 && js.cu_count % 8 == 0) ? 8 : 1;
    const int ring_cap = std::max(1, std::min(js.cu_count > 0 ? js.cu_count : 256, 256));
    RingPlan plan;
    JacTournament T;
    bool use_ring = !force_pairs && plan_ring(c, n_xcd, ring_cap, &plan);
    if (c.cut2 <= 0.0 && !use_ring) {
        T = jacobi_tournament(c.n_eff.data(), nl);
        if (upload_tournament(T, B.h_items, B.d_items, c.st)) return 1;
    }
    // large blocks: pivoted QR on this stream, then the sweeps; the small blocks run their whole SVD beside
    // them on the forked stream and join before the call returns
    HIP_TRY(hipEventRecord(js.ev_fork, c.st));
    HIP_TRY(hipStreamWaitEvent(js.aux, js.ev_fork, 0));
    hipLaunchKernelGGL(k_jacobi_svd, dim3(n_blocks), dim3(JAC_THREADS), JAC_LDS_ELEMS * sizeof(double2), js.aux, c.G, c.Vj, S,
                       desc, max_sweeps, tol, info_dev, JAC_LDS_ELEMS, (const int*)B.d_slot, c.cut2);
    HIP_TRY(hipEventRecord(js.ev_join, js.aux));
    if (launch_qr_large(c, js, B, n_xcd)) return 1;
    if (c.cut2 > 0.0) {        // the tournament is sized by the ranks the QR found: wait for them (one sync per call)
        HIP_TRY(hipEventRecord(js.ev_sweep[0], c.st));
        HIP_TRY(htn_event_spin(js.ev_sweep[0]));
        for (int li = 0; li < nl; ++li) c.n_eff[li] = std::min(c.n_eff[li], (int)B.h_rank[li]);
        if (use_ring) use_ring = plan_ring(c, n_xcd, ring_cap, &plan);
        if (!use_ring) {
            T = jacobi_tournament(c.n_eff.data(), nl);
            if (upload_tournament(T, B.h_items, B.d_items, c.st)) return 1;
        }
    }
    if (use_ring) return run_ring(c, js, B, plan, n_xcd, ring_two_partner, ring_staged, sweeps_used);
    return run_pair_visits(c, js, B, T, opts && opts->sweeps_hint > 0 ? opts->sweeps_hint : 0, sweeps_used);
}

// ---- plain (non-QRCP) blocks with columns longer than 512 rows ("tall"): streamed pair visits ---------------------------
// `tall`: their indices; everything else of the batch goes to jacobi_svd_core from here, on the same stream and first
static int jacobi_svd_tall(void* G, void* Vj, double* S, const htn_svd_block* desc, const htn_svd_block* desc_host,
                           int32_t n_blocks, int32_t max_m_rest, int32_t max_sweeps, double tol, int32_t* info_dev,
                           const htn_svd_opts* opts, void* stream, const std::vector<int>& tall) {
    const int nt = (int)tall.size();
    hipStream_t st = (hipStream_t)stream;
    JacScratch* jsp = nullptr;
    if (js_get(st, &jsp)) return 1;
    JacScratch& js = *jsp;
    // the tournament of the pair-visit path: round-robin over panels of JAC_PANEL columns, the intra-panel visits last
    std::vector<int> n_cols(nt);
    for (int li = 0; li < nt; ++li) n_cols[li] = desc_host[tall[li]].n;
    const JacTournament T = jacobi_tournament(n_cols.data(), nt);
    const size_t n_items = T.items.size();
    // device scratch [skip | ids | zero2 | partials | ratio | done | sweeps | items]; ratio | done | sweeps zeroed as one
    const size_t off_skip = 0, off_ids = off_skip + sizeof(int) * n_blocks;
    const size_t off_zero = (off_ids + sizeof(int) * nt + 7) / 8 * 8, off_part = off_zero + sizeof(double) * nt;
    const size_t off_ratio = off_part + sizeof(double) * nt * TALL_PARTS, off_done = off_ratio + 16 * (size_t)nt;      // ratio: 2 words per block
    const size_t off_sw = off_done + sizeof(int) * nt, off_items = (off_sw + sizeof(int) * nt + 31) / 32 * 32;
    const size_t flag_elems = (size_t)std::max(max_sweeps, 0) + 1;
    if (js.tall_dev.reserve(off_items + sizeof(JacPairItem) * std::max<size_t>(n_items, 1))) return 1;
    if (js.tall_pin.reserve(sizeof(JacPairItem) * std::max<size_t>(n_items, 1) + sizeof(int) * (n_blocks + nt))) return 1;
    if (js.tall_flags.reserve(sizeof(int) * flag_elems)) return 1;
    char* d = (char*)js.tall_dev.p;
    int* d_skip = (int*)(d + off_skip);
    int* d_ids = (int*)(d + off_ids);
    double* d_zero = (double*)(d + off_zero);
    double* d_part = (double*)(d + off_part);
    unsigned long long* d_ratio = (unsigned long long*)(d + off_ratio);
    int* d_done = (int*)(d + off_done);
    int* d_sw = (int*)(d + off_sw);
    JacPairItem* d_items = (JacPairItem*)(d + off_items);
    JacPairItem* h_items = (JacPairItem*)js.tall_pin.p;
    int* h_skip = (int*)((char*)js.tall_pin.p + sizeof(JacPairItem) * std::max<size_t>(n_items, 1));
    int* h_ids = h_skip + n_blocks;      // [skip | ids] contiguous like the device copy: ONE upload
    volatile int* h_active = (volatile int*)js.tall_flags.p;
    int* d_active = (int*)js.tall_flags.dev;
    std::vector<unsigned char> skip(n_blocks, 0);
    for (int li = 0; li < nt; ++li) skip[tall[li]] = 1;
    for (int b = 0; b < n_blocks; ++b) h_skip[b] = skip[b] ? 0 : -1;      // k_jacobi_svd leaves blocks with a slot >= 0
    for (int li = 0; li < nt; ++li) h_ids[li] = tall[li];
    for (size_t k = 0; k < flag_elems; ++k) h_active[k] = 1;
    HIP_TRY(hipMemcpyAsync(d_skip, h_skip, sizeof(int) * (n_blocks + nt), hipMemcpyHostToDevice, st));
    if (upload_tournament(T, h_items, d_items, st)) return 1;
    HIP_TRY(hipMemsetAsync(d_ratio, 0, 24 * (size_t)nt, st));      // ratio (16 nt) | done (4 nt) | sweeps (4 nt)
    // everything else first: small blocks, QRCP large blocks (their call returns once they are done)
    int core_used = 0;
    if (nt < n_blocks) {
        if (jacobi_svd_core(G, Vj, S, desc, desc_host, n_blocks, max_m_rest, max_sweeps, tol, info_dev, opts, stream, d_skip,
                            skip.data()))
            return 1;
        if (opts && opts->sweeps_used) core_used = *opts->sweeps_used;
    }
    int max_n = 1;
    for (int li = 0; li < nt; ++li) max_n = std::max(max_n, (int)desc_host[tall[li]].n);
    hipLaunchKernelGGL(k_jacobi_tall_init, dim3(nt, TALL_PARTS), dim3(256), 0, st, (double2*)G, (double2*)Vj, desc, d_ids, d_part);
    hipLaunchKernelGGL(k_jacobi_tall_zero, dim3(1), dim3(64), 0, st, (const double*)d_part, d_zero, nt);
    HIP_TRY(hipGetLastError());
    const int hint = opts && opts->sweeps_hint > 0 ? opts->sweeps_hint : 0;
    const int used = jacobi_sweep_pipeline(max_sweeps, hint, js.ev_sweep, h_active, st, [&](int sweep) {
        for (int r = 0; r < T.n_rounds(); ++r)
            if (T.round_size(r))
                hipLaunchKernelGGL(k_jacobi_tall_visit, dim3(T.round_size(r)), dim3(TALL_THREADS), 0, st, (double2*)G,
                                   (double2*)Vj, desc, d_ids, d_items + T.off[r], d_zero, d_ratio, d_done, tol);
        hipLaunchKernelGGL(k_jacobi_check, dim3(1), dim3(64), 0, st, d_ratio, d_done, d_sw, nt, tol, d_active + sweep);
    });
    if (used < 0) return 1;
    hipLaunchKernelGGL(k_jacobi_tall_finish, dim3((unsigned)((max_n + 3) / 4), (unsigned)nt), dim3(256), 0, st,
                       (const double2*)G, S, desc, d_ids, d_sw, d_done, info_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(htn_stream_spin(st));      // the staging blocks are reused by the next call
    if (opts && opts->sweeps_used) *opts->sweeps_used = std::max(core_used, used);
    return 0;
}

// Entry point: blocks of at most 512 rows go to jacobi_svd_core; plain (non-QRCP) blocks with longer columns ("tall") to the
// streamed pair-visit path above, on the same stream, after the core path has been enqueued (its large blocks finish first)
extern "C" int htn_jacobi_svd_z(void* G, void* Vj, double* S, const htn_svd_block* desc,
                                const htn_svd_block* desc_host, int32_t n_blocks, int32_t max_m_host,
                                int32_t max_sweeps, double tol, int32_t* info_dev, const htn_svd_opts* opts,
                                void* stream) {
    if (n_blocks <= 0) return 0;
    std::vector<int> tall;
    int max_m_rest = 0;
    if (desc_host) {
        for (int b = 0; b < n_blocks; ++b) {
            const htn_svd_block& D = desc_host[b];
            if (!(D.flags & HTN_SVD_QRCP) && D.m > 64 * JAC_MAXEL) tall.push_back(b);
            else max_m_rest = std::max(max_m_rest, std::max(D.m, D.pad));
        }
    } else if (max_m_host > 64 * JAC_MAXEL) {
        return fail_msg("htn_jacobi_svd_z: blocks taller than 512 rows need the host copy of the descriptors (desc_host)");
    }
    if (tall.empty())
        return jacobi_svd_core(G, Vj, S, desc, desc_host, n_blocks, max_m_host, max_sweeps, tol, info_dev, opts, stream,
                               nullptr, nullptr);
    if (max_m_rest > 64 * JAC_MAXEL) return fail_msg("htn_jacobi_svd_z: block taller than 512 rows");
    return jacobi_svd_tall(G, Vj, S, desc, desc_host, n_blocks, max_m_rest, max_sweeps, tol, info_dev, opts, stream, tall);
}

#include "htn_batched_copy.h"
