// Internal to the sweep engine (htn_engine.cpp and the files around it: htn_site.cpp, htn_overlap.cpp, htn_correlator.cpp,
// htn_applyop.cpp, htn_variance.cpp, htn_sample.cpp, htn_idmrg.cpp, htn_capi.cpp):
// the handles behind the C ABI, device buffers, the compiled-plan records of the plan cache, and the htn_mps state itself.
// Those files form ONE translation unit (htn_engine.cpp includes the others): the using-directive below and the shared types in
// namespace htn never meet another unit's names.  What a single one of those files uses stays in that file.  Host C++ (no HIP): device work goes through htn::Backend.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>

#include "htn_core.h"

using namespace htn;

// Handles are reference counted: an htn_mps keeps its context and its MPO alive, so destroying the handles in any order
// (garbage-collected host languages do exactly that) is safe; the last release frees the object.
struct htn_ctx {
    std::atomic<int> refs{1};
    std::unique_ptr<Backend> be;
    int rank = 0, world = 1;
    bool shard = false;              // zero y + reduce after every matvec (world > 1, or forced for tests)
    htn_exchange2_fn exch = nullptr;
    void* exch_user = nullptr;
};
struct htn_mpo {
    std::atomic<int> refs{1};
    htn_ctx* ctx;
    Mpo mpo;
};
inline void ctx_release(htn_ctx* c) {
    if (c && --c->refs == 0) delete c;
}
inline void mpo_release(htn_mpo* m) {
    if (m && --m->refs == 0) {
        htn_ctx* c = m->ctx;
        delete m;
        ctx_release(c);
    }
}

namespace htn {

inline double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct DBuf {
    Backend* be;
    void* p;
    size_t bytes;
    DBuf(Backend* b, size_t n) : be(b), p(nullptr), bytes(n) { p = be->alloc(std::max<size_t>(n, 16)); }
    ~DBuf() {
        if (p) be->release(p);
    }
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
};
typedef std::shared_ptr<DBuf> DBufP;
// device buffer of host data (copy items, descriptors, column indices, scale factors, small matrices)
template <class T>
DBufP upload_vec(Backend* be, const std::vector<T>& v) {
    auto b = std::make_shared<DBuf>(be, sizeof(T) * std::max<size_t>(v.size(), 1));
    if (!b->p) return nullptr;
    if (!v.empty() && be->upload(b->p, v.data(), sizeof(T) * v.size())) return nullptr;
    return b;
}
struct DView {                     // complex128 window of a device buffer
    DBufP base;
    int64_t off = 0;
    cplx* ptr() const { return base ? (cplx*)base->p + off : nullptr; }
};

// plain rows x cols copy, op N: no gather, no scaling (callers set what differs)
inline htn_copy_item copy_item(int64_t dst_off, int32_t ldd, int64_t src_off, int32_t lds, int32_t rows, int32_t cols) {
    htn_copy_item it;
    memset(&it, 0, sizeof(it));
    it.dst_off = dst_off, it.src_off = src_off, it.idx_off = -1, it.scl_off = -1;
    it.rows = rows, it.cols = cols, it.ldd = ldd, it.lds = lds, it.op = HTN_OP_N, it.scale_dim = -1;
    return it;
}

// host wall time of the stages of one update; with `profile` every lap ends in a stream sync (GPU-inclusive times)
struct StageClock {
    Backend* be;
    bool profile;
    double t0, last;
    double plan = 0.0, lanczos = 0.0, svd = -1.0, env = 0.0;      // svd < 0: what the other stages leave of the total
    StageClock(Backend* b, bool p) : be(b), profile(p), t0(now()), last(t0) {}
    double lap() {
        if (profile) be->sync();
        const double t = now(), d = t - last;
        last = t;
        return d;
    }
};

struct DevTasks {
    DBufP mem;
    const htn_tile* tiles = nullptr;
    const htn_seg* segs = nullptr;
    int32_t ntiles = 0, nsegs = 0;
    int32_t ws_slots = 0;          // split-K workspace slabs the list needs (balance_tiles)
    int64_t flops = 0;
};

struct ApplyC {
    DevTasks dz, dy;
    bool has_z = false;
    int64_t zsize = 0, flops = 0;
    int32_t ntiles = 0, nsegs = 0;
};
template <class Lay>
struct TwoStageC {                 // compiled two-stage contraction (EnvPlan / OvlPlan): stage 1 -> BUF_Z, stage 2 -> BUF_Y
    std::shared_ptr<const Lay> lay;        // layout of the result (not set: the caller names it -- projector rows)
    DevTasks d1, d2;
    int64_t zsize = 0, flops = 0;
};
typedef TwoStageC<EnvLayout> EnvC;
typedef TwoStageC<OvlLayout> OvlC;
struct SvdC {
    SvdPlan sp;
    DBufP stage, desc;
    // sector-sharded SVD (world > 1): the blocks this rank owns (LPT over ~ m n^2), as their own staging / descriptor lists
    std::vector<htn_svd_block> own_desc;
    DBufP own_stage, own_desc_dev;
    int n_own = 0;
};
struct FinC {
    SiteLayoutP layA, layB;
    DBufP items;                   // iso_g | cen_g | iso_v copy items
    const htn_copy_item *ig = nullptr, *cg = nullptr, *iv = nullptr;
    int n_ig = 0, n_cg = 0, n_iv = 0;
    DevTasks cen;
    bool has_cen = false;
};

struct Spectrum {
    std::vector<Sec> secs;
    std::vector<std::vector<double>> vals;
};
struct RelayC {                    // copy items that re-lay a site tensor from one layout kind to another (or copy it)
    DBufP items;
    int n = 0;
};
struct Gauge1C {                   // compiled gauge move of a one-site update: QR / LQ descriptors + absorption into the neighbour
    std::vector<htn_qr_block> desc;
    DBufP desc_dev;
    int64_t rsize = 0;
    DevTasks absorb;
};
struct MeetC {                     // the items that pair the left and the right half of a correlator on one bond (htn_block_trdots_z)
    std::vector<htn_trdot_item> items;
    DBufP items_dev;
};
struct OrthState {                 // one attached state phi: overlap environments <psi|phi> per bond, carried along the sweep
    htn_mps* phi = nullptr;
    std::vector<OvlLayoutP> Llay, Rlay;
    std::vector<DView> Lbuf, Rbuf;
};
struct Solve {                     // the eigenproblem of one update (compiled apply, vector length) and what the solver returned
    std::shared_ptr<ApplyC> ap;
    int64_t n = 0;
    double E = 0.0, res = 0.0, mv_ms = 0.0;
    int nmv = 0;
    double growth = 1.0;           // evolving updates: |x| / |x0| of the exponential
    double xnorm = 0.0;            // correction-vector updates: |theta_new| and <p|theta_new>
    cplx bx = 0.0;
};
struct BondWork {                  // what flows between the steps of one two-site update (htn_mps::update_bond)
    ThetaLayoutP tl;
    Solve sol;
    // device buffers: all live until the update returns and go back to the pool in reverse order of declaration
    DView V, z, Qb;                // Krylov basis (row 0: theta, then the optimised tensor); Z stage of the apply; projector rows
    DView X;                       // correction-vector updates: start value, then the solution (Qb: the right-hand side)
    std::shared_ptr<SvdC> sc;
    DView G, Vj;
    DBufP S, idx;                  // s_elems singular values | per-block sweep counts (int32); kept columns, block after block
    size_t s_elems = 0;
    std::vector<double> s_host;    // host copy of S
    int jac_sweeps = 0;
    std::vector<int> lens, qd, counts;     // per block: values, quantum dimension, kept values
    std::vector<std::vector<int>> order;   // per block: its columns by descending value
    std::vector<double> vals;              // all values, block after block, each block descending
    double nrm = 0.0, tw = 0.0;
    BondP mid;
    double tA = 0.0, tB = 0.0, tC = 0.0, tD = 0.0;      // HTN_DEBUG_HOST_TIMERS: after the SVD call, download, truncation, finalise plan
};

}  // namespace htn

struct SiteWork;                   // one-site updates (htn_site.cpp)
struct CorrProbe;                  // what the probe pass of one correlator entry differs in (htn_correlator.cpp)

struct htn_mps {
    std::atomic<int> refs{1};      // htn_mps_destroy drops one reference (htn_idmrg_window hands out extra ones)
    htn_ctx* ctx;
    htn_mpo* mpo_handle = nullptr;
    Backend* be;
    const Mpo* mpo;
    int L;
    std::vector<BondP> bonds;
    std::vector<SiteLayoutP> site_lay;
    std::vector<DView> site_buf;
    std::vector<EnvLayoutP> Llay, Rlay;
    std::vector<DView> Lbuf, Rbuf;
    std::unordered_map<std::string, std::shared_ptr<const void>> cache;
    int64_t hits = 0, misses = 0;
    double energy = 0.0;
    std::map<int, Spectrum> spectra;
    std::map<int, std::pair<std::pair<int, double>, double>> cut_hint;      // bond -> ((chi, cutoff), smallest kept value)
    std::map<int, int> sweeps_hint;     // bond -> outer Jacobi sweeps its large blocks needed last time (htn_svd_opts.sweeps_hint)
    std::vector<int32_t> idx_host;
    std::vector<OrthState> orth;        // htn_mps_set_orthogonal: the sweep stays in the orthogonal complement of these states
    int orth_dropped = 0;               // projector vectors dropped as numerically dependent in the last bond update
    int centre = 0;                     // site that carries the centre (htn_mps_create: 0; every update moves it)
    // Every update normalises the tensors it writes.  A state made by htn_mps_apply_op carries <O psi|O psi> in its tensors
    // (raw_n2 >= 0) until its first update, and from then on beside them: the state is amp x (the stored tensors).  Overlaps and
    // transition amplitudes multiply by amp; every other state has amp = 1 and raw_n2 < 0 for life -- but a correction vector
    // (htn_bond_solve / htn_cv_sweep), whose amp is the norm of its last local solution.
    double amp = 1.0, raw_n2 = -1.0;
    void norm_absorbed() {
        if (raw_n2 >= 0.0) amp = sqrt(raw_n2), raw_n2 = -1.0;
    }

    template <class T, class F>
    std::shared_ptr<T> cached(const std::string& key, F build) {
        auto it = cache.find(key);
        if (it != cache.end()) {
            ++hits;
            return std::const_pointer_cast<T>(std::static_pointer_cast<const T>(it->second));
        }
        if (cache.size() > 20000) cache.clear();
        ++misses;
        std::shared_ptr<T> v = build();
        if (v) cache[key] = v;
        return v;
    }
    static std::string ikey(const char* tag, int i) {
        std::string k(tag);
        k.append((const char*)&i, sizeof(i));
        return k;
    }
    DBufP dalloc(size_t bytes) {
        auto b = std::make_shared<DBuf>(be, bytes);
        return b->p ? b : nullptr;
    }
    DView zalloc(int64_t n, bool zero) {
        DView v;
        v.base = dalloc(sizeof(cplx) * (size_t)std::max<int64_t>(n, 1));
        if (v.base && zero) be->zero(v.base->p, sizeof(cplx) * (size_t)std::max<int64_t>(n, 1));
        return v;
    }
    DView ws;                      // split-K workspace of the grouped GEMM: [tickets | slabs], grown on demand
    int64_t ws_slots = -1;
    int ensure_ws(int slots) {
        if (slots <= ws_slots) return 0;
        const int64_t want = std::max<int64_t>(2 * (int64_t)slots, 256);
        ws = zalloc(HTN_WS_ELEMS(want), false);
        if (!ws.base) return set_error("device allocation of the split-K workspace failed");
        if (be->zero(ws.ptr(), sizeof(cplx) * HTN_WS_TICKET_ELEMS)) return 1;      // tickets start at zero; the kernel resets them
        ws_slots = want;
        return 0;
    }
    int upload_tasks(const Tasks& t_in, DevTasks& d) {
        Tasks balanced;
        const Tasks* tp = &t_in;
        d.ws_slots = 0;
        if (be->kind() == HTN_BACKEND_HIP && t_in.ntiles > 0) {        // (the CPU baseline runs tiles as they are)
            balanced = t_in;
            balanced.tiles.resize((size_t)t_in.ntiles);
            d.ws_slots = balance_tiles(balanced, 256);
            tp = &balanced;
        }
        const Tasks& t = *tp;
        const size_t tb = (sizeof(htn_tile) * t.tiles.size() + 63) / 64 * 64, sb = sizeof(htn_seg) * t.segs.size();
        d.mem = dalloc(tb + sb);
        if (!d.mem) return set_error("device allocation of a task list failed");
        if (be->upload(d.mem->p, t.tiles.data(), sizeof(htn_tile) * t.tiles.size())) return 1;
        if (be->upload((char*)d.mem->p + tb, t.segs.data(), sb)) return 1;
        d.tiles = (const htn_tile*)d.mem->p;
        d.segs = (const htn_seg*)((char*)d.mem->p + tb);
        d.ntiles = t.ntiles;
        d.nsegs = t.nsegs;
        d.flops = t.flops;
        return 0;
    }
    // (htn_plan_apply_dump shows the lists BEFORE balancing: those are what the Python statement of the planner emits)
    SiteLayoutP site_layout(char kind, BondP bl, BondP br) {
        return cached<const SiteLayout>(std::string("slay") + kind + bl->key + "|" + br->key,
                                        [&] { return build_site_layout(mpo->sym, kind, bl, br); });
    }
    ThetaLayoutP theta_layout(BondP bl, BondP br) {
        return cached<const ThetaLayout>(std::string("tl") + bl->key + "|" + br->key,
                                         [&] { return build_theta_layout(mpo->sym, bl, br); });
    }
    int gemm(const DevTasks& d, std::initializer_list<std::pair<int, const void*>> bufs) {
        if (d.ntiles == 0) return 0;
        if (ensure_ws(d.ws_slots)) return 1;
        const void* table[HTN_MAX_BUFS] = {nullptr};
        for (auto& kv : bufs) table[kv.first] = kv.second;
        table[HTN_BUF_WS] = ws.ptr();
        return be->grouped_gemm(table, d.tiles, d.ntiles, d.segs);
    }

    // compiled two-stage plan: upload t1 and t2, record zsize (and the flops)
    template <class C, class P>
    std::shared_ptr<C> compile2(std::shared_ptr<C> e, const P& p) {
        if (upload_tasks(p.t1, e->d1) || upload_tasks(p.t2, e->d2)) return nullptr;
        e->zsize = p.zsize;
        e->flops = p.t1.flops + p.t2.flops;
        return e;
    }
    // ---- htn_engine.cpp: environments, H_eff applies, the two-site update ----
    int env_step(char side, int i);
    int env_launch(bool left, const EnvC& c, const cplx* in, const cplx* site, DView* out);
    int left_env(int i) { return env_step('L', i); }
    int right_env(int i) { return env_step('R', i); }
    // H_eff applies (two-site: make_apply, one-site: make_apply1, zero-site on a bond: make_apply0)
    std::shared_ptr<ApplyC> compile_apply(ApplyPlan& p, bool deal_y);
    std::shared_ptr<ApplyC> make_apply(int i, const ThetaLayout& tl);
    std::shared_ptr<ApplyC> make_apply1(int i, const SiteLayout& lay);
    std::shared_ptr<ApplyC> make_apply0(int b);
    int apply_stages(const ApplyC& ap, const DView& L, const DView& R, const DView& z, htn_gemm_launch* stages);
    int apply_once(const ApplyC& ap, const DView& L, const DView& R, int64_t n, const void* x_host, void* y_host, bool exchange);
    int theta_into(int i, const ThetaLayout& tl, cplx* dst);
    // two-site update: update_bond runs these once each, in this order
    int bond_solve(int i, bool optimise, const htn_sweep_opts& o, StageClock& clk, BondWork& w, const cplx* evolve_dt = nullptr,
                   const cplx* solve_z = nullptr);
    std::shared_ptr<SvdC> make_svd(int i, const ThetaLayout& tl, bool right);
    int bond_svd(int i, bool right, const htn_sweep_opts& o, BondWork& w);
    int bond_truncate(int i, const htn_sweep_opts& o, BondWork& w);
    int bond_finalise(int i, bool right, BondWork& w);
    int bond_advance(int i, bool right);
    void bond_spectrum(int i, const BondWork& w);
    void fill_stats(htn_bond_stats* st, int bond, int direction, const Solve& sol, int64_t env_elems, int jacobi_sweeps,
                    int64_t svd_flops, double trunc_weight, const StageClock& clk);
    int update_bond(int i, int direction, bool right, bool optimise, const htn_sweep_opts& o, htn_bond_stats* st,
                    const cplx* evolve_dt = nullptr, double* log_growth = nullptr, const cplx* solve_z = nullptr, double* cv_out = nullptr);
    // correction-vector sweeps (htn_bond_solve / htn_cv_sweep): update_bond with Backend::krylov_solve as the solver
    int cv_checks(const htn_sweep_opts& o, const char* who) const;
    int cv_sweep(cplx z, const htn_sweep_opts& o, htn_bond_stats* st, double* cv_out);
    int sweep(const htn_sweep_opts& o, htn_bond_stats* st, double* E);
    int set_mpo(htn_mpo* m);
    // ---- htn_site.cpp: one-site DMRG (htn_site_update / htn_dmrg1_sweep) and time evolution (htn_bond_evolve /
    // htn_site_evolve / htn_tdvp2_sweep; one-site TDVP: htn_site_evolve_move / htn_tdvp1_sweep) ----
    int relay(const SiteLayout& from, const cplx* src, const SiteLayout& to, cplx* dst);
    int site_solve(int i, const SiteLayout& from, const SiteLayout& lay, bool optimise, const cplx* evolve_dt, const htn_sweep_opts& o,
                   StageClock& clk, SiteWork& w);
    int update_site(int i, int direction, bool optimise, const htn_sweep_opts& o, htn_bond_stats* st);
    int sweep1(const htn_sweep_opts& o, htn_bond_stats* st, double* E);
    int evolve_checks(const htn_sweep_opts& o, const char* who) const;
    int evolve_site(int i, cplx dt, const htn_sweep_opts& o, htn_bond_stats* st, double* log_growth);
    int tdvp2_sweep(cplx dt, const htn_sweep_opts& o, htn_bond_stats* st, double* E, double* log_norm);
    int bond0_checks(int b, const char* who) const;
    int evolve_site_move(int i, int direction, cplx dt_fwd, cplx dt_back, const htn_sweep_opts& o, htn_bond_stats* st, double* log_growth);
    int tdvp1_sweep(cplx dt, const htn_sweep_opts& o, htn_bond_stats* st, double* E, double* log_norm);
    // ---- htn_overlap.cpp: overlap environments, attached states ----
    // overlap transfers with `ket` as the ket state (this = bra): in -> out across site i
    int ovl_step(char side, const htn_mps* ket, int i, const OvlLayoutP& inl, const DView& in, OvlLayoutP* outl, DView* out);
    int ovl_boundary(const htn_mps* ket, int b, OvlLayoutP* outl, DView* out);
    int ovl_project(const OrthState& o, int i, const ThetaLayout& tl, cplx* dst);
    int orth_attach(htn_mps* const* others, int n);
    void orth_detach();
    int set_orthogonal(const htn_mps* const* others, int n);      // htn_mps_set_orthogonal
    int overlap(const htn_mps* ket, double* out_host);            // htn_mps_overlap
    // ---- htn_correlator.cpp: correlation functions, one probe pass behind the one-site and the bond-operator entry ----
    int corr_checks(const char* who, const htn_site_op& pass, const char* ends_note);
    DView site_as(const SiteLayout& want, int i);
    int probe_step(char side, const Mpo& pm, const MpoSite& W, const EnvLayoutP& inl, const cplx* in, int i, const std::string& key,
                   EnvLayoutP* outl, DView* out);
    int corr_pass(const CorrProbe& p, cplx* out_host, double* norm_host);
    int correlator(const htn_corr_channel& ch, cplx* out_host, double* norm_host);       // htn_mps_correlator
    int correlator2(const htn_corr_channel2& ch, cplx* out_host, double* norm_host);     // htn_mps_correlator2
    // ---- htn_applyop.cpp: a local operator applied to the state, transition amplitudes of all sites ----
    int apply_op(int site, const htn_site_op* op, htn_mps** out, double* norm2_host);      // htn_mps_apply_op (this = the source, only read)
    int transition(const htn_site_op* op, const htn_mps* ket, cplx* out_host);             // htn_mps_transition (this = the bra)
    // ---- htn_variance.cpp: the two-site energy variance ----
    int variance(double* site_host, double* bond_host, double* energy_host, double* split_host);      // htn_mps_variance
    // ---- htn_sample.cpp: perfect sampling of site multiplets ----
    int sample(int32_t n_samples, const double* u_host, const int32_t* measure_host, int32_t batch, int32_t* out_host, double* logp_host,
               double* split_host);                                                                   // htn_mps_sample
};

// ---- pieces of the engine that more than one file uses ------------------------------------------------------------------
htn_sweep_opts norm_opts(const htn_sweep_opts* o);      // the defaults of htn_sweep_opts filled in (htn_engine.cpp)
// construction of an htn_mps, shared by htn_mps_create, htn_mps_set_mpo and the IDMRG2 driver (htn_engine.cpp)
htn_mps* mps_new(htn_ctx* ctx, const htn_mpo* mpo);
struct MpsGuard {              // drops a half-built htn_mps (and the references it took) on an error return
    htn_mps* p;
    ~MpsGuard() {
        if (p) htn_mps_destroy(p);
    }
};
int mps_load_bonds(htn_mps* e, const int32_t* bond_ptr, const htn_sector* sectors);
int mps_load_sites(htn_mps* e, const int32_t* sub_ptr, const htn_subblock* subs, const int64_t* data_ptr, const void* data_host);
int mps_finish(htn_mps* e, const void* left_env_host, const void* right_env_host, const DView* left_dev, const DView* right_dev);
int site1_checks(const htn_mps* m, int i, const char* who);      // what every one-site entry asks of the state (htn_site.cpp)
// the IDMRG2 growth driver behind htn_idmrg_* (htn_idmrg.cpp)
int idmrg_create(htn_ctx* ctx, const htn_mpo* mpo, const htn_idmrg_opts* opts, htn_idmrg** out);
void idmrg_free(htn_idmrg* d);
int32_t idmrg_boundary(const htn_idmrg* d, int32_t side, htn_sector* out);
int idmrg_step(htn_idmrg* d, const int32_t* bond_ptr, const htn_sector* sectors, const int32_t* sub_ptr, const htn_subblock* subs,
               const int64_t* data_ptr, const void* data_host, htn_idmrg_stats* stats);
int idmrg_window(htn_idmrg* d, htn_mps** out);
