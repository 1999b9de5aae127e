// Jacobi SVD, piece of htn_svd.hip: ring block Jacobi (k_jacobi_ring) with its two diagnostic builds
#pragma once

// =====================================================================================================================
// Ring block Jacobi: the large blocks' sweeps in ONE launch
// =====================================================================================================================
// The multi-launch path above pays, per tournament round, a kernel boundary plus a visit that re-derives everything from
// global memory (columns -> LDS, Gram, P U back): 15 us per round, ~210 dependent rounds per centre bond at chi = 1024, with
// a tenth of the chip busy.  Here a block of n columns is given P workgroups (one per CU, 1024 threads) that stay resident
// for ALL sweeps.  The columns are cut into 2 P panels of w columns; every workgroup keeps two panels in LDS (w * mp <= 4608
// elements each) and plays the classic round-robin ("caterpillar") tournament on panels: in each of the 2 P - 1 rounds of a
// sweep it rotates its w x w cross pairs directly on the LDS-resident columns (plain one-sided rotations, one group of GS
// lanes per pair, the panel-T column of a group kept in registers for the whole round), then the panels move one position:
// top panels to the next workgroup, bottom panels to the previous one (workgroup 0 keeps its top, the last one turns its
// top into its bottom).  Once per sweep the pairs INSIDE the resident panels are rotated.  A sweep costs
// (2 P - 1) x (w steps of ~0.5 us + one panel exchange) instead of ~(n / 8) x 15 us.
//
// Hand-off between workgroups inside the launch (cdna_hip_programming.md section 6, Guideline 16, form R1 / first table row of
// MI355X_MICROARCH.md "visibility"): the payload goes out as 16-byte WRITE-THROUGH (sc1) stores into the receiver's mailbox,
// every storing wave drains (s_waitcnt vmcnt(0)), workgroup barrier, ONE lane stores the round's epoch into the receiver's
// flag with an agent-scope atomic store; the receiver polls that one word with relaxed agent-scope loads from ONE lane,
// workgroup barrier, then EVERY load of the payload is an sc1 load.  No placement assumption: correctness does not depend on
// which CU or XCD a workgroup landed on.  Mailbox slots alternate by epoch parity; neighbours exchange in both directions in
// every round, so a sender can be at most one round ahead of its receiver and never overwrites a slot that is still unread.
// All workgroups of a launch are co-resident (the host caps the grid at the CU count; LDS use forces one per CU); every poll
// is bounded by wall-clock time and a shared failure word, so a launch always drains.
#define RING_THREADS 512
#define RING_PANEL_ELEMS 4608         // complex128 elements of one resident panel (2 panels = 144 KiB of LDS)
#define RING_MAX_P 64
struct RingItem {
    int32_t li;        // large-block index (large_ids[li] = block in desc)
    int32_t k, P;      // CU slot of this workgroup, CU slots of the block
    int32_t w;         // panel width: panel q = columns [q w, min((q + 1) w, n))
    int32_t n;         // columns taking part (the rank the QR found, <= desc.n)
    int32_t g0;        // grid index of the block's slot 0 (flag addressing)
    int64_t mbox;      // element offset of the block's mailboxes: slot k owns 4 slots [role][parity] of w * mp elements
};                     // 32 bytes
typedef unsigned int ring_u4 __attribute__((ext_vector_type(4)));
// Lanes per column (GS) and elements per lane (E).  A rotation step is a dependent chain (LDS read -> dots -> DPP sums ->
// rotation arithmetic -> update -> LDS write -> barrier) and every VALU instruction of a wave costs 4 clocks whatever it does,
// so the sums and the scalar arithmetic of a rotation must be amortised over many elements per lane.  Measured per step of
// 15-16 pairs on a 202 x 202 block: 64 lanes x 4 elements (one pair per wave, 16 waves) 1.86 us -- 260 wave instructions per
// pair, 64 of them useful, VALU-issue bound; 16 lanes x 14 elements (FOUR pairs per wave, the sums stay inside one DPP row)
// 1.06 us; 32 lanes x 7 elements (two pairs per wave, two busy waves per SIMD) 1.12 us.  Beyond 256 rows a lane cannot hold
// a column in 16 lanes' registers: 64 lanes x <= 8 elements.
__host__ __device__ __forceinline__ int ring_gs(int m) { return m <= 256 ? 16 : 64; }
__host__ __device__ __forceinline__ int ring_e(int m) {
    const int g = ring_gs(m);
    return (m + g - 1) / g;
}
// one lane polls one word (relaxed, agent scope); false: timed out or another workgroup reported failure
__device__ __forceinline__ bool ring_wait_ge(unsigned* flag, unsigned want, unsigned* fail) {
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

// LDS panel (cnt contiguous elements) -> mailbox slot, 16-byte stores (the caller drains and raises the flag): sc1
// (write-through to memory, any placement) or, when the block's workgroups have FOUND themselves on one XCD (`local`, see
// ring_run), plain stores that stay in that XCD's L2 -- the reader's sc1 loads are served from the same L2
__device__ __forceinline__ void ring_send(const double2* __restrict__ src, double2* slot, int cnt, int tid, bool local) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)slot, 0, cnt * 16, 0x00020000);
    if (local) {
        for (int idx = tid; idx < cnt; idx += RING_THREADS) {
            const double2 v = src[idx];
            ring_u4 u;
            __builtin_memcpy(&u, &v, 16);
            __builtin_amdgcn_raw_buffer_store_b128(u, rs, idx * 16, 0, 0);
        }
    } else {
        for (int idx = tid; idx < cnt; idx += RING_THREADS) {
            const double2 v = src[idx];
            ring_u4 u;
            __builtin_memcpy(&u, &v, 16);
            __builtin_amdgcn_raw_buffer_store_b128(u, rs, idx * 16, 0, 16);       // aux 16 = sc1
        }
    }
}
// the epoch word that tells a neighbour its panel has arrived (after the drain and the barrier): agent scope, or -- all
// workgroups of the block on one XCD -- a store that stays in the shared L2 (the poll is an agent-scope load either way)
__device__ __forceinline__ void ring_flag(unsigned* flag, unsigned epoch, bool local) {
    if (local) __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// mailbox slot -> LDS panel, every load sc1; all loads of a thread in flight together (cnt <= 9 * 512)
__device__ __forceinline__ void ring_recv(double2* dst, const double2* slot, int cnt, int tid) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)slot, 0, cnt * 16, 0x00020000);
    // (unconditional loads: the descriptor's range check returns zeros beyond cnt, and a conditionally filled register
    // array makes the compiler carry -- and spill -- the whole array as one tuple)
#define RING_LD(q) const ring_u4 u##q = __builtin_amdgcn_raw_buffer_load_b128(rs, (tid + q * RING_THREADS) * 16, 0, 16)
    RING_LD(0);
    RING_LD(1);
    RING_LD(2);
    RING_LD(3);
    RING_LD(4);
    RING_LD(5);
    RING_LD(6);
    RING_LD(7);
    RING_LD(8);
#undef RING_LD
    auto put = [&](int idx, ring_u4 u) {
        if (idx < cnt) {
            double2 v;
            __builtin_memcpy(&v, &u, 16);
            dst[idx] = v;
        }
    };
    put(tid + 0 * RING_THREADS, u0);
    put(tid + 1 * RING_THREADS, u1);
    put(tid + 2 * RING_THREADS, u2);
    put(tid + 3 * RING_THREADS, u3);
    put(tid + 4 * RING_THREADS, u4);
    put(tid + 5 * RING_THREADS, u5);
    put(tid + 6 * RING_THREADS, u6);
    put(tid + 7 * RING_THREADS, u7);
    put(tid + 8 * RING_THREADS, u8);
}

// ---- the direct exchange (default; HTN_RING_STAGED_SEND=1 keeps ring_send / ring_recv above) ---------------------------
// Same protocol, same slots, same bits; what the staged form did for nothing is gone:
//   send     the last cross step of a round stores the columns it holds in registers straight to the neighbour's slot
//            (ring_cross, SEND) -- no LDS round trip, no copy loop, no barrier of its own;
//   receive  the two directions are independent: waves 0-3 take the top panel, waves 4-7 the bottom one (a workgroup at an
//            end of the ring receives one panel with all waves), one lane per direction polls, the others of that half watch
//            a word in LDS, and the loads of a half start when ITS flag is up;
//   norms    a half loads in the layout of the rotations (a group of GS lanes per column, lane sub holds rows sub + GS e), so
//            the squared column norms the next round starts from are summed from the registers on their way to LDS -- same
//            lanes, same element order, same reduction as the recomputation in ring_cross, hence the same bits.
// One column of E register elements, times its scale, to column offset `off` of a mailbox slot (16-byte stores, sc1 unless
// `local`, see ring_send).  ALL E elements go out: rows m .. mp - 1 of a panel are zeros in registers as they are in LDS, and
// they arrive as zeros.
__device__ __forceinline__ void ring_store16(double2 x, __amdgpu_buffer_rsrc_t rs, int elem, bool local) {
    ring_u4 u;
    __builtin_memcpy(&u, &x, 16);
    if (local) __builtin_amdgcn_raw_buffer_store_b128(u, rs, elem * 16, 0, 0);
    else __builtin_amdgcn_raw_buffer_store_b128(u, rs, elem * 16, 0, 16);          // aux 16 = sc1
}
template <int GS, int E>
__device__ __forceinline__ void ring_send_col(const double2 (&v)[E], double s, __amdgpu_buffer_rsrc_t rs, int off, bool local) {
#pragma unroll
    for (int e = 0; e < E; ++e) ring_store16(make_double2(v[e].x * s, v[e].y * s), rs, off + GS * e, local);
}
// mailbox slot -> LDS panel of nc columns by ng groups of GS lanes (this lane: group g, lane sub), every load sc1, all loads
// of a lane in flight together: two columns per group where the planner can give a group two (w <= 32 against 16 groups of a
// half up to 144 rows, w <= 8 against 4 waves of a half in the 64-lane form), one where it cannot (w <= 16 from 145 rows on) --
// the loops only say that nothing is assumed.  The descriptor's range check returns zeros for a column that is not there.
// norm[c] <- squared norm of column c, scale[c] <- 1 (bottom panels).
template <int GS, int E>
__device__ __forceinline__ void ring_recv_cols(double2* dst, const double2* slot, int nc, int g, int ng, int sub, double* norm,
                                               double* scale) {
    constexpr int mp = GS * E;
    constexpr bool PAIRS = GS == 64 || E <= 9;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)slot, 0, nc * mp * 16, 0x00020000);
    auto put = [&](int c, const ring_u4 (&u)[E]) {
        if (c < nc) {
            double2* col = dst + c * mp + sub;
            double t = 0.0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                double2 v;
                __builtin_memcpy(&v, &u[e], 16);
                t = fma(v.x, v.x, fma(v.y, v.y, t));
                col[GS * e] = v;
            }
            t = group_sum<GS>(t);
            if (sub == 0) {
                norm[c] = t;
                if (scale) scale[c] = 1.0;
            }
        }
    };
    for (int c0 = g; c0 < nc; c0 += (PAIRS ? 2 : 1) * ng) {
        ring_u4 u0[E];
#pragma unroll
        for (int e = 0; e < E; ++e) u0[e] = __builtin_amdgcn_raw_buffer_load_b128(rs, (c0 * mp + sub + GS * e) * 16, 0, 16);
        if constexpr (PAIRS) {
            const int c1 = c0 + ng;
            ring_u4 u1[E];
#pragma unroll
            for (int e = 0; e < E; ++e) u1[e] = __builtin_amdgcn_raw_buffer_load_b128(rs, (c1 * mp + sub + GS * e) * 16, 0, 16);
            put(c0, u0);
            put(c1, u1);
        } else put(c0, u0);
    }
}
// where the register send of a round goes (ring_cross, SEND)
struct RingOut {
    __amdgpu_buffer_rsrc_t slot_t, slot_b;      // the neighbours' slots for this workgroup's top / bottom panel
    bool send_t;                                // the top panel leaves (every workgroup but the first and the last)
    bool keep_t;                                // the top panel is needed in this workgroup's LDS afterwards (first: it stays; last: it becomes the bottom)
    bool local;
};

// Rotation of a column pair held in registers; returns the squared cosine seen.  With g = a^H b, h = |b|^2 - |a|^2:
//   q = sign(h) 2 / (|h| + sqrt(h^2 + 4 |g|^2)) = tan / |g|,  c = 1 / sqrt(1 + q^2 |g|^2),
//   [a' b'] = [a b] [[c, c q g], [-c q conj(g), c]]
// -- real diagonal, so neither |g| nor the phase g / |g| is ever formed (three reciprocal-type operations instead of
// five); against the textbook form b' carries an extra unit phase, which a one-sided Jacobi SVD is free to choose.
// NORMS = false: aa / bb come in as the tracked squared norms of the two columns and go out updated by Rutishauser's
// identities |a'|^2 = |a|^2 - q |g|^2, |b'|^2 = |b|^2 + q |g|^2 (as LAPACK's xGESVJ tracks them); they only steer the
// rotation angle and the stopping test and are recomputed from the columns at the start of every round, i.e. after at
// most w updates.  Halves the dot products and the reductions of a rotation.
template <int GS, int E, bool NORMS>
__device__ __forceinline__ double ring_rotate(double2 (&a)[E], const double2 (&b)[E], double2* b_out, double& aa, double& bb,
                                              double tol2, double zero2) {
    double gr = 0.0, gi = 0.0;
    if (NORMS) {
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            sa = fma(a[e].x, a[e].x, fma(a[e].y, a[e].y, sa));
            sb = fma(b[e].x, b[e].x, fma(b[e].y, b[e].y, sb));
        }
        aa = group_sum<GS>(sa);
        bb = group_sum<GS>(sb);
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        gr = fma(a[e].x, b[e].x, fma(a[e].y, b[e].y, gr));      // conj(a) * b
        gi = fma(a[e].x, b[e].y, fma(-a[e].y, b[e].x, gi));
    }
    gr = group_sum<GS>(gr);
    gi = group_sum<GS>(gi);
    if (aa <= zero2 || bb <= zero2) return 0.0;
    const double g2 = fma(gr, gr, gi * gi);
    const double ab = aa * bb;
    if (g2 == 0.0) return 0.0;
    // the squared cosine only steers the stopping test: the hardware reciprocal (no Newton step) is plenty
    const double ratio2 = g2 * __builtin_amdgcn_rcp(ab);
    if (g2 <= tol2 * ab) return ratio2;
    // ANY real q gives an exactly unitary rotation once c = 1 / sqrt(1 + q^2 |g|^2) is accurate; q itself only sets the
    // angle, so the hardware rsq / rcp seeds (relative error ~1e-8: the pair is left with a cosine 1e-8 times the one it
    // had, below what the next sweep's quadratic convergence leaves anyway) do without their Newton steps
    const double h = bb - aa;
    const double w2 = fma(h, h, 4.0 * g2);
    const double w = w2 * __builtin_amdgcn_rsq(w2);
    double q = 2.0 * __builtin_amdgcn_rcp(fabs(h) + w);
    q = h >= 0.0 ? q : -q;
    const double c = fast_rsq(fma(q * q, g2, 1.0));
    const double cq = c * q;
    const double sr = cq * gr, si = -cq * gi;                   // sig = c q conj(g):  a' = c a - sig b,  b' = conj(sig) a + c b
    aa = fma(-q, g2, aa);
    bb = fma(q, g2, bb);
    // b' goes straight to its column in LDS (only a rotated column is written back), a is updated IN PLACE (scale, then
    // accumulate): neither needs a register copy where the rotated and the skipped path meet
#pragma unroll
    for (int e = 0; e < E; ++e) {
        double2 nb;
        nb.x = fma(si, a[e].y, fma(sr, a[e].x, c * b[e].x));
        nb.y = fma(-si, a[e].x, fma(sr, a[e].y, c * b[e].y));
        b_out[GS * e] = nb;
        double x = a[e].x * c, y = a[e].y * c;
        x = fma(-sr, b[e].x, x);
        y = fma(-sr, b[e].y, y);
        a[e].x = fma(si, b[e].y, x);
        a[e].y = fma(-si, b[e].x, y);
    }
    return ratio2;
}

// Per-step split of a cross step (diagnostic build -DHTN_RING_PROF -DHTN_RING_STEP_PROF only, tools/ring_prof.py): shader-clock
// stamps at the boundaries of LDS read | dot + sums | angle | update + write | barrier.  Each stamp drains the wave's LDS
// operations (s_waitcnt lgkmcnt(0)), so a phase holds its own LDS latency, and the steps get slower (202 x 202: cross rotations
// 222 instead of 180 us per sweep): the phase times of -DHTN_RING_PROF alone are the ones to compare.  Elsewhere the stamps
// compile to nothing.
struct RingStamps {
    long long t[6];
};
#if defined(HTN_RING_STEP_PROF) && !defined(HTN_RING_PROF)
#error "HTN_RING_STEP_PROF needs HTN_RING_PROF (the split is stored with the phase times)"
#endif
#ifdef HTN_RING_STEP_PROF
#define RING_ST(st, i)                                                                                      \
    do {                                                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"((st).t[i])::"memory");                  \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
    } while (0)
#else
#define RING_ST(st, i) \
    do {               \
    } while (0)
#endif

// The same rotation in SCALED ("fast") form for the cross rounds: a column is kept as (scale, stored vector) with true column =
// scale * stored.  With the true g = sa sb g_st the update  [a' b'] = [a b] [[c, c q g], [-c q conj(g), c]]  becomes
//   a_st' = a_st - (q sb^2 conj(g_st)) b_st,   b_st' = b_st + (q sa^2 g_st) a_st,   sa' = c sa,   sb' = c sb
// -- 8 real multiply-adds per element pair instead of 12 (the factor c moves into the two scales).  Scales start at 1 in
// every round and are applied when the round ends (at most w factors c >= 1/sqrt 2 accumulate: no range issue).
// OUT = true (the round's last step when the columns leave from registers): b' goes, times its final scale, to column offset
// out_off of the mailbox slot out_rs instead of to b_out, and `sent` is set; a pair that is not rotated leaves `sent` alone
// and the caller sends b as it stands.  The same multiply-adds on the same operands.
// sec2max <- max(sec2max, 1 + tan^2 of this rotation): 1 + q^2 |g|^2 is the argument of the rsq that gives c, so the second
// number of the stopping rule (jacobi_last_sweep) costs one v_max_f64 per rotation.  tan^2 = sec2max - 1 resolves 2e-16,
// and the rule compares tan^2 with tol^2 / mx >= 1e-13 (it is asked only where mx <= 0.1 tol).
template <int GS, int E, bool OUT = false>
__device__ __forceinline__ double ring_rotate_scaled(double2 (&a)[E], const double2 (&b)[E], double2* b_out, double& aa, double& bb,
                                                     double& sa, double& sb, double tol2, double zero2, double& sec2max, RingStamps& st,
                                                     __amdgpu_buffer_rsrc_t out_rs = __amdgpu_buffer_rsrc_t(), int out_off = 0,
                                                     bool out_local = false, bool* sent = nullptr) {
    // conj(a_st) * b_st in FOUR independent chains (even / odd elements x re / im): a dependent f64 multiply-add cannot issue
    // back to back, and with one busy wave per SIMD nothing else fills the slots
    double gr = 0.0, gi = 0.0, gr1 = 0.0, gi1 = 0.0;
#pragma unroll
    for (int e = 0; e + 1 < E; e += 2) {
        gr = fma(a[e].x, b[e].x, fma(a[e].y, b[e].y, gr));
        gi = fma(a[e].x, b[e].y, fma(-a[e].y, b[e].x, gi));
        gr1 = fma(a[e + 1].x, b[e + 1].x, fma(a[e + 1].y, b[e + 1].y, gr1));
        gi1 = fma(a[e + 1].x, b[e + 1].y, fma(-a[e + 1].y, b[e + 1].x, gi1));
    }
    if (E & 1) {
        gr = fma(a[E - 1].x, b[E - 1].x, fma(a[E - 1].y, b[E - 1].y, gr));
        gi = fma(a[E - 1].x, b[E - 1].y, fma(-a[E - 1].y, b[E - 1].x, gi));
    }
    gr = group_sum<GS>(gr + gr1);
    gi = group_sum<GS>(gi + gi1);
    RING_ST(st, 2);
    if (aa <= zero2 || bb <= zero2) return 0.0;
    const double ss = sa * sb;
    const double g2 = ss * ss * fma(gr, gr, gi * gi);           // |g|^2 of the true columns
    const double ab = aa * bb;
    if (g2 == 0.0) return 0.0;
    const double ratio2 = g2 * __builtin_amdgcn_rcp(ab);
    if (g2 <= tol2 * ab) return ratio2;
    const double h = bb - aa;
    const double w2 = fma(h, h, 4.0 * g2);
    const double w = w2 * __builtin_amdgcn_rsq(w2);
    double q = 2.0 * __builtin_amdgcn_rcp(fabs(h) + w);
    q = h >= 0.0 ? q : -q;
    const double sec2 = fma(q * q, g2, 1.0);
    const double c = fast_rsq(sec2);
    sec2max = fmax(sec2max, sec2);
    aa = fma(-q, g2, aa);
    bb = fma(q, g2, bb);
    const double qb = q * sb * sb, qa = q * sa * sa;
    const double mur = qb * gr, mui = -qb * gi;                 // mu = q sb^2 conj(g_st)
    const double nur = qa * gr, nui = qa * gi;                  // nu = q sa^2 g_st
    sa *= c;
    sb *= c;
    RING_ST(st, 3);
    // b' first (computed and handed to LDS), a' afterwards: the update of a (in registers, needed only by the next step's dot)
    // covers the drain of the LDS writes that the barrier after the step waits for.  Interleaved per element, the last
    // writes left the VALU with nothing to do; the arithmetic is the same.  Cross rotations per sweep: 202 x 202 189 -> 180 us,
    // 400 x 400 486 -> 427 us (profiles/r04_ring_qr_phase_times.txt).
    if constexpr (OUT) {
        *sent = true;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            double2 nb;
            nb.x = fma(-nui, a[e].y, fma(nur, a[e].x, b[e].x));
            nb.y = fma(nui, a[e].x, fma(nur, a[e].y, b[e].y));
            ring_store16(make_double2(nb.x * sb, nb.y * sb), out_rs, out_off + GS * e, out_local);
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            double x = fma(-mur, b[e].x, a[e].x), y = fma(-mur, b[e].y, a[e].y);
            a[e].x = fma(mui, b[e].y, x);
            a[e].y = fma(-mui, b[e].x, y);
        }
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            double2 nb;
            nb.x = fma(-nui, a[e].y, fma(nur, a[e].x, b[e].x));
            nb.y = fma(nui, a[e].x, fma(nur, a[e].y, b[e].y));
            b_out[GS * e] = nb;
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            double x = fma(-mur, b[e].x, a[e].x), y = fma(-mur, b[e].y, a[e].y);
            a[e].x = fma(mui, b[e].y, x);
            a[e].y = fma(-mui, b[e].x, y);
        }
    }
    RING_ST(st, 4);
    return ratio2;
}

// all nt x nb cross pairs of the two resident panels: group g owns T column g in registers (and its tracked norm), B columns
// pass through LDS, their tracked norms through bnorm[]
//   TWO = false (one partner per step, the default): in step s group g meets B column (g + s) mod wm; wm steps, one workgroup
//     barrier each.
//   TWO = true (two partners per step, GS = 16 only, HTN_RING_TWO_PARTNER=1): T columns 2i, 2i+1 sit in rows 2i, 2i+1 of ONE
//     wave and meet the B pair (2j, 2j+1), j = (i + s) mod ceil(wm / 2), in two phases -- (2i, 2j) | (2i+1, 2j+1), then (2i, 2j+1) | (2i+1, 2j).  The
//     B columns change rows between the phases through LDS inside the wave (the wave's LDS operations complete in order; the
//     drain plus the compiler barrier keep the read after the write), so a workgroup barrier comes once per two meetings.
//     The same rotations (ring_rotate_scaled) in another order inside the round; every cross pair still meets once per round.
//     Odd or ragged panels: the missing column's row sits the phase out.  Measured no faster than TWO = false (202 x 202: the
//     barrier is ~15 % of a step, the phase-2 read waits for the phase-1 writes, odd w wastes a phase per round) and one sweep
//     more on some blocks of the headline: kept behind the switch.
// split (diagnostic build): per-phase shader-clock sums of group 0 over the steps in which all its meetings rotated.
//   have_t / have_b: the panel came in through ring_recv_cols, which left the squared norms of its columns in tnorm[] /
//     bnorm[] (and bscale[] = 1): nothing to recompute.
//   SEND = true (TWO = false, nt > 0, nb > 0; the direct exchange): the round's LAST step hands the panels over from registers.
//     In that step group g < wm holds B column j = (g + wm - 1) mod wm -- every B column exactly once: rotated in registers if
//     g owns a T column, read from LDS as it stands if not (ragged panels) -- and stores it, times its scale, to the slot
//     out.slot_b; group g < nt stores its T column to out.slot_t (send_t) and / or writes it to LDS (keep_t).  The bottom
//     panel always leaves, so it is not written back to LDS, and there is no barrier here: the caller's drain + barrier
//     before the flag is the next one.
// Returns the largest squared cosine seen; sec2max <- max(sec2max, 1 + largest tan^2 rotated by), see ring_rotate_scaled.
template <int GS, int E, bool TWO, bool SEND>
__device__ __forceinline__ double ring_cross(double2* T, double2* B, int nt, int nb, int tid, double tol2, double zero2, double* bnorm,
                                             double* bscale, const double* tnorm, bool have_t, bool have_b, const RingOut& out,
                                             long long* split, double& sec2max) {
    static_assert(!TWO || GS == 16, "two partners per step need both rows of a pair in one wave");
    static_assert(!(TWO && SEND), "the two-partner step keeps the staged send");
    constexpr int mp = GS * E;
    const int grp = tid / GS, sub = tid % GS;
    const int wm = nt > nb ? nt : nb;
    double ratio = 0.0;
    if (nt == 0 || nb == 0) return ratio;                      // (uniform over the workgroup)
    const bool own = grp < nt;
    double2 a[E];
    double aa = 0.0, sa = 1.0;
    if (own) {
#pragma unroll
        for (int e = 0; e < E; ++e) a[e] = T[grp * mp + sub + GS * e];
        if (have_t) aa = tnorm[grp];
        else {
            double t = 0.0;
#pragma unroll
            for (int e = 0; e < E; ++e) t = fma(a[e].x, a[e].x, fma(a[e].y, a[e].y, t));
            aa = group_sum<GS>(t);
        }
    }
    if (!have_b && grp < nb) {            // exact squared norm of B column grp; its scale starts at 1
        const double2* bc = B + grp * mp + sub;
        double sb = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const double2 v = bc[GS * e];
            sb = fma(v.x, v.x, fma(v.y, v.y, sb));
        }
        sb = group_sum<GS>(sb);
        if (sub == 0) {
            bnorm[grp] = sb;
            bscale[grp] = 1.0;
        }
    }
    if (!have_b) __syncthreads();      // (uniform; a received panel's norms were written before the barrier that ended the receive)
    constexpr int phases = TWO ? 2 : 1;
    const int hp = TWO ? (wm + 1) >> 1 : wm;                   // steps per round
    const int row = TWO ? (grp & 1) : 0, pr = TWO ? (grp >> 1) : grp;
    (void)split;
    for (int s = 0; s < (SEND ? hp - 1 : hp); ++s) {
        int jp = pr + s;
        jp = jp >= hp ? jp - hp : jp;                           // (pr < hp for every group that owns a T column)
#ifdef HTN_RING_STEP_PROF
        long long acc[4] = {0, 0, 0, 0};
        bool all = true;
#endif
        RingStamps st;
#pragma unroll
        for (int ph = 0; ph < phases; ++ph) {
            const int j = TWO ? 2 * jp + (row ^ ph) : jp;
            st.t[4] = 0;
            RING_ST(st, 0);
            if (own && j < nb) {
                double2 b[E];
                double2* bc = B + j * mp + sub;
#pragma unroll
                for (int e = 0; e < E; ++e) b[e] = bc[GS * e];
                double bb = bnorm[j], sb = bscale[j];
                RING_ST(st, 1);
                const double rr = ring_rotate_scaled<GS, E>(a, b, bc, aa, bb, sa, sb, tol2, zero2, sec2max, st);
                ratio = fmax(ratio, rr);
                if (sub == 0) {
                    bnorm[j] = bb;
                    bscale[j] = sb;
                }
            }
#ifdef HTN_RING_STEP_PROF
            if (st.t[4] == 0) all = false;
            else {
                acc[0] += st.t[1] - st.t[0];
                acc[1] += st.t[2] - st.t[1];
                acc[2] += st.t[3] - st.t[2];
                acc[3] += st.t[4] - st.t[3];
            }
#endif
            // between the phases: the B column this row wrote is read by the other row of the wave
            if (TWO && ph == 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
#ifdef HTN_RING_STEP_PROF
        const long long tb = st.t[4];
#endif
        __syncthreads();
#ifdef HTN_RING_STEP_PROF
        RING_ST(st, 5);
        if (tid == 0 && all && tb != 0) {
            for (int q = 0; q < 4; ++q) split[q] += acc[q];
            split[4] += st.t[5] - tb;
            split[5] += 1;
            split[6] += phases;
        }
#endif
    }
    if constexpr (SEND) {      // the last step: the columns leave from registers
        int jp = pr + hp - 1;
        jp = jp >= hp ? jp - hp : jp;
        RingStamps st;
        if (grp < hp && jp < nb) {
            double2 b[E];
            const double2* bc = B + jp * mp + sub;
#pragma unroll
            for (int e = 0; e < E; ++e) b[e] = bc[GS * e];
            double bb = bnorm[jp], sb = bscale[jp];
            bool sent = false;
            if (own) {
                const double rr = ring_rotate_scaled<GS, E, true>(a, b, nullptr, aa, bb, sa, sb, tol2, zero2, sec2max, st, out.slot_b,
                                                                  jp * mp + sub, out.local, &sent);
                ratio = fmax(ratio, rr);
            }
            if (!sent) ring_send_col<GS, E>(b, sb, out.slot_b, jp * mp + sub, out.local);
        }
        if (own) {
            if (out.send_t) ring_send_col<GS, E>(a, sa, out.slot_t, grp * mp + sub, out.local);
            if (out.keep_t) {
#pragma unroll
                for (int e = 0; e < E; ++e) T[grp * mp + sub + GS * e] = make_double2(a[e].x * sa, a[e].y * sa);
            }
        }
        return ratio;
    }
    if (own) {                 // the scales come out with the columns: T from registers, B in place
#pragma unroll
        for (int e = 0; e < E; ++e) T[grp * mp + sub + GS * e] = make_double2(a[e].x * sa, a[e].y * sa);
    }
    if (grp < nb) {
        const double sb = bscale[grp];
        if (sb != 1.0) {
            double2* bc = B + grp * mp + sub;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double2 v = bc[GS * e];
                bc[GS * e] = make_double2(v.x * sb, v.y * sb);
            }
        }
    }
    __syncthreads();
    return ratio;
}

// the pairs inside each resident panel (circle tournament per panel, both panels side by side)
template <int GS, int E>
__device__ __forceinline__ double ring_intra(double2* T, int nt, double2* B, int nb, int tid, double tol2, double zero2, double& t2max) {
    constexpr int mp = GS * E;
    const int grp = tid / GS, sub = tid % GS;
    const int npT = nt + (nt & 1), npB = nb + (nb & 1), hT = npT >> 1, hB = npB >> 1;
    const int steps = (npT > npB ? npT : npB) - 1;
    double ratio = 0.0;
    for (int r = 0; r < steps; ++r) {
        double2* base = nullptr;
        int np = 0, pn = 0, p = 0;
        if (grp < hT) base = T, np = npT, pn = nt, p = grp;
        else if (grp < hT + hB) base = B, np = npB, pn = nb, p = grp - hT;
        if (base && r < np - 1) {
            const int md = np - 1;
            int i, j;
            if (p == 0) i = np - 1, j = r;
            else {
                i = r + p;
                i = i >= md ? i - md : i;
                j = r + md - p;
                j = j >= md ? j - md : j;
            }
            if (i < pn && j < pn) {
                const int lo = i < j ? i : j, hi = i < j ? j : i;
                const double rr = jacobi_pair_pad<GS, E>(base + lo * mp, base + hi * mp, sub, tol2, zero2, t2max);
                ratio = rr > ratio ? rr : ratio;
            }
        }
        __syncthreads();
    }
    return ratio;
}

#ifdef HTN_RING_PROF        // diagnostic build only (tools/ring_prof.py): per-workgroup 100 MHz tick sums per phase
__device__ long long g_ring_prof[256 * 16];
extern "C" int htn_ring_prof_dump(long long* out) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ring_prof), sizeof(long long) * 256 * 16));
    return 0;
}
#endif
struct RingArgs {
    double2* Vj;
    double2* G;
    double* S;
    const htn_svd_block* desc;
    const int* large_ids;
    const RingItem* items;
    const int* perm;
    const double* zero2;
    double2* mbox;
    unsigned* sync;              // [flags: 2 per workgroup | arrive: nl * max_sweeps | fail | pad | conv (u64): 2 x nl * max_sweeps,
                                 //  per block and sweep the largest squared cosine seen, then the largest tan^2 rotated by]
    int arrive_off, fail_off, conv_off;      // in 32-bit words (conv_off even)
    int xcc_off;                 // 32-bit words: one per workgroup, XCD id + 1 once the workgroup has started
    int max_sweeps;
    int two_partner;             // 1: two partner columns per cross step (HTN_RING_TWO_PARTNER=1, 16-lane form only)
    int staged_send;             // 1: the staged panel exchange (HTN_RING_STAGED_SEND=1: ring_send / ring_recv)
    double tol;
    int* info;
    int* sweeps_out;             // host-mapped, [nl]: outer sweeps of each block (0 = failed)
};

template <int GS, int E>
__device__ __forceinline__ void ring_run(const RingArgs A, const RingItem it, const htn_svd_block D, double2* lds, int* s_top, int* s_bot,
                         unsigned long long* s_rbits, int* s_ok, double* s_bnorm, int* s_local, unsigned* s_arr) {
    constexpr int mp = GS * E;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = it.P, k = it.k, w = it.w, n = it.n, m = D.m;
    double2* __restrict__ X = A.Vj + D.v_off;
    const int slot_elems = w * mp;
    double2* bufT = lds;
    double2* bufB = lds + slot_elems;
    unsigned* flags = A.sync;
    unsigned* fail = A.sync + A.fail_off;
    const double zero2 = A.zero2[it.li];
    const double tol2 = A.tol * A.tol;
    auto ncols = [&](int q) {
        const int c = n - q * w;
        return c < 0 ? 0 : (c > w ? w : c);
    };
    if (tid < P) {
        s_top[tid] = 2 * tid;
        s_bot[tid] = 2 * tid + 1;
    }
    if (tid == 0) {
        *s_ok = 1;
        s_arr[0] = s_arr[1] = 0u;
        // Which XCD is this?  The host places a block's workgroups at grid positions that the dispatcher has been SEEN to
        // deal to one XCD (position mod 8); nothing promises that, so every workgroup publishes the XCD id it reads from
        // the hardware register and the block takes the cheaper hand-off (plain stores kept in the shared L2) only if ALL
        // of its workgroups report the same id -- otherwise the placement-independent sc1 form, as before.  Every
        // workgroup of the block reads the same P words, so all take the same decision.
        int local = 0;
        if (P > 1 && A.xcc_off >= 0) {
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            xcc = (xcc & 0xfu) + 1u;
            unsigned* xw = A.sync + A.xcc_off + it.g0;
            __hip_atomic_store(xw + k, xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            local = 1;
            for (int q = 0; q < P && local >= 0; ++q) {
                if (!ring_wait_ge(xw + q, 1u, fail)) local = -1;
                else if (__hip_atomic_load(xw + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != xcc) local = local > 0 ? 0 : local;
            }
            if (local < 0) *s_ok = 0;
        }
        *s_local = local > 0 ? 1 : 0;
    }
    __syncthreads();
    const bool local = *s_local != 0;
    {   // resident panels <- X (written by the QR kernel before this launch: plain loads), re-padded from X's leading
        // dimension (the rule of the one-workgroup kernel) to mp rows; rows >= m are zero in both
        const int gsx = m <= 16 * JAC_MAXEL ? 16 : (m <= 32 * JAC_MAXEL ? 32 : 64);
        const int ldx = gsx * ((m + gsx - 1) / gsx);
        for (int side = 0; side < 2; ++side) {
            const int q = side ? s_bot[k] : s_top[k];
            double2* buf = side ? bufB : bufT;
            const int cnt = ncols(q) * mp;
            for (int idx = tid; idx < cnt; idx += RING_THREADS) {
                const int c = idx / mp, i = idx - c * mp;
                buf[idx] = i < m ? X[(int64_t)(q * w + c) * ldx + i] : make_double2(0.0, 0.0);
            }
        }
    }
    __syncthreads();
#ifdef HTN_RING_PROF
    // cross | send+drain | flags+wait | recv | intra | conv | total | sweeps,P | split of the cross steps (shader clock, see
    // ring_cross): LDS read, dot + sums, angle, update + write, barrier, steps, meetings | shader clock over the run.
    // Direct exchange: the mailbox stores are part of "cross" (its last step, which the step split does not count), "send+drain"
    // is the drain + barrier, "flags+wait" lane 0's flags and the wait of its half, "recv" that half's loads + the common barrier
    long long prof[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const long long prof_t0 = wall_clock64();
    long long prof_c0;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(prof_c0)::"memory");
#endif
    long long* split = nullptr;
#ifdef HTN_RING_STEP_PROF
    split = prof + 8;
#endif
    int sweeps = 0;
    bool done = n < 2, ok = *s_ok != 0;
    const int rounds = 2 * P - 1;
    const bool direct = A.staged_send == 0;                     // the direct exchange (see ring_send_col)
    double* const s_bscale = s_bnorm + RING_THREADS / 16;
    double* const s_tnorm = s_bnorm + 2 * (RING_THREADS / 16);
    while (!done && ok && sweeps < A.max_sweeps) {
        double ratio = 0.0, t2 = 0.0, sec2 = 1.0;      // sec2: 1 + tan^2 of the cross rotations, t2: tan^2 of those inside the panels
        for (int r = 0; r < rounds && ok; ++r) {
            const unsigned epoch = (unsigned)(sweeps * rounds + r + 1);
            const int par = (int)(epoch & 1u);
            const int nt = ncols(s_top[k]), nb = ncols(s_bot[k]);
            JAC_T(RING_PROF, p0);
            double2* box = A.mbox + it.mbox;                    // slot of workgroup kd, role, parity: ((kd * 2 + role) * 2 + par)
            // where this workgroup's panels go: top -> top of k + 1 (the first one's stays, the last one's becomes its bottom),
            // bottom -> bottom of k - 1 (the first one's -> top of 1)
            double2* const to_t = box + (int64_t)(((k + 1) * 2 + 0) * 2 + par) * slot_elems;
            double2* const to_b = k == 0 ? box + (int64_t)((1 * 2 + 0) * 2 + par) * slot_elems
                                         : box + (int64_t)(((k - 1) * 2 + 1) * 2 + par) * slot_elems;
            const bool send_t = k > 0 && k < P - 1;
            // a panel that came in through the direct receive brought its norms (not the first round of a sweep: the pairs
            // inside the panels have been rotated since)
            const bool have_t = direct && r > 0 && k > 0, have_b = direct && r > 0 && k < P - 1;
            const bool reg_send = direct && !(GS == 16 && A.two_partner) && P > 1 && nt > 0 && nb > 0;
            RingOut out;
            out.slot_t = __builtin_amdgcn_make_buffer_rsrc((void*)to_t, 0, (reg_send && send_t) ? nt * mp * 16 : 0, 0x00020000);
            out.slot_b = __builtin_amdgcn_make_buffer_rsrc((void*)to_b, 0, reg_send ? nb * mp * 16 : 0, 0x00020000);
            out.send_t = send_t, out.keep_t = !send_t, out.local = local;
            double rr = 0.0;
            if (reg_send) rr = ring_cross<GS, E, false, true>(bufT, bufB, nt, nb, tid, tol2, zero2, s_bnorm, s_bscale, s_tnorm, have_t, have_b, out, split, sec2);
            else if (GS == 16 && A.two_partner) {
                if constexpr (GS == 16)        // (64 lanes per column: the two rows of a pair would be two waves)
                    rr = ring_cross<GS, E, true, false>(bufT, bufB, nt, nb, tid, tol2, zero2, s_bnorm, s_bscale, s_tnorm, have_t, have_b, out, split, sec2);
            } else rr = ring_cross<GS, E, false, false>(bufT, bufB, nt, nb, tid, tol2, zero2, s_bnorm, s_bscale, s_tnorm, have_t, have_b, out, split, sec2);
            ratio = rr > ratio ? rr : ratio;
            JAC_T(RING_PROF, p1);
            JAC_ACC(RING_PROF, prof, 0, p0, p1);
            if (P < 2) continue;
            // ---- panels move one position: send (unless the last cross step has done it), drain, raise the flags ----
            if (!reg_send) {
                if (send_t) ring_send(bufT, to_t, nt * mp, tid, local);
                ring_send(bufB, to_b, nb * mp, tid, local);
            }
            // the panels that come in (the ids follow the same permutation in every workgroup of the block; lane 0 applies it
            // after the barrier)
            const int in_top = k == 0 ? s_top[0] : (k == 1 ? s_bot[0] : s_top[k - 1]);
            const int in_bot = k < P - 1 ? s_bot[k + 1] : s_top[P - 1];
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            JAC_T(RING_PROF, p2);
            JAC_ACC(RING_PROF, prof, 1, p1, p2);          // (direct exchange: drain + barrier only, the stores are part of the cross phase)
            // the direction a wave receives: 0 top, 1 bottom; a workgroup at an end of the ring has one direction for all waves
            const int half = k == 0 ? 1 : (k == P - 1 ? 0 : wave >> 2);
            const bool both = k > 0 && k < P - 1;
            if (tid == 0) {
                if (k == 0) ring_flag(flags + (it.g0 + 1) * 2 + 0, epoch, local);
                else {
                    if (k < P - 1) ring_flag(flags + (it.g0 + k + 1) * 2 + 0, epoch, local);
                    ring_flag(flags + (it.g0 + k - 1) * 2 + 1, epoch, local);
                }
                const int t_last = s_top[P - 1], b0 = s_bot[0];
                for (int q = P - 1; q >= 2; --q) s_top[q] = s_top[q - 1];
                s_top[1] = b0;
                for (int q = 0; q + 1 < P; ++q) s_bot[q] = s_bot[q + 1];
                s_bot[P - 1] = t_last;
                if (!direct) {
                    // ---- wait for what comes in ----
                    bool good = true;
                    if (k > 0) good = ring_wait_ge(flags + (it.g0 + k) * 2 + 0, epoch, fail);
                    if (good && k < P - 1) good = ring_wait_ge(flags + (it.g0 + k) * 2 + 1, epoch, fail);
                    if (!good) *s_ok = 0;
                }
            }
            if (k == P - 1) {           // the last workgroup's top panel becomes its bottom panel: swap the roles of the buffers
                double2* t = bufT;
                bufT = bufB;
                bufB = t;
            }
            if (!direct) {
                __syncthreads();
                JAC_T(RING_PROF, p3);
                JAC_ACC(RING_PROF, prof, 2, p2, p3);
                ok = *s_ok != 0;
                if (ok) {
                    const double2* mine = box + (int64_t)(k * 4) * slot_elems;
                    if (k > 0) ring_recv(bufT, mine + (int64_t)(0 * 2 + par) * slot_elems, ncols(s_top[k]) * mp, tid);
                    if (k < P - 1) ring_recv(bufB, mine + (int64_t)(1 * 2 + par) * slot_elems, ncols(s_bot[k]) * mp, tid);
                }
                __syncthreads();
                JAC_T(RING_PROF, p4);
                JAC_ACC(RING_PROF, prof, 3, p3, p4);
            } else {
                // ---- each direction on its own: one lane polls the flag (bounded, as every poll), tells its half through LDS
                // (epoch, or all ones: failed), the half loads; both halves meet at the barrier before the next round ----
                if (tid == (both ? half * (RING_THREADS / 2) : 0)) {
                    const bool good = ring_wait_ge(flags + (it.g0 + k) * 2 + half, epoch, fail);
                    if (!good) *s_ok = 0;
                    __hip_atomic_store(s_arr + half, good ? epoch : ~0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                unsigned seen;
                while ((seen = __hip_atomic_load(s_arr + half, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) < epoch)
                    __builtin_amdgcn_s_sleep(1);
                JAC_T(RING_PROF, p3);
                JAC_ACC(RING_PROF, prof, 2, p2, p3);      // (lane 0: flags + the wait of ITS half)
                if (seen != ~0u) {
                    const double2* mine = box + (int64_t)(k * 4 + half * 2 + par) * slot_elems;
                    const int ngt = RING_THREADS / GS, ng = both ? ngt / 2 : ngt, grp = tid / GS;
                    ring_recv_cols<GS, E>(half ? bufB : bufT, mine, ncols(half ? in_bot : in_top), both ? grp % ng : grp, ng, tid % GS,
                                          half ? s_bnorm : s_tnorm, half ? s_bscale : nullptr);
                }
                __syncthreads();
                JAC_T(RING_PROF, p4);
                JAC_ACC(RING_PROF, prof, 3, p3, p4);      // (lane 0: the loads of its half + the wait for the other half)
                ok = *s_ok != 0;
            }
        }
        if (!ok) break;
        JAC_T(RING_PROF, p5);
        {
            const double rr = ring_intra<GS, E>(bufT, ncols(s_top[k]), bufB, ncols(s_bot[k]), tid, tol2, zero2, t2);
            ratio = rr > ratio ? rr : ratio;
        }
        JAC_T(RING_PROF, p6);
        JAC_ACC(RING_PROF, prof, 4, p5, p6);
        // ---- block-wide maxima of the squared cosines this sweep SAW and of the tan^2 it rotated by (integer maxima on the
        //      bit patterns: any order gives the same bits): two returning atomic maxima + one arrival per workgroup ----
        if (tid == 0) s_rbits[0] = s_rbits[1] = 0ull;
        __syncthreads();
        {
            const unsigned long long key = wave_max_u64((unsigned long long)__double_as_longlong(ratio));
            const unsigned long long key2 = wave_max_u64((unsigned long long)__double_as_longlong(fmax(t2, sec2 - 1.0)));
            if (lane == 0 && key) atomicMax(s_rbits, key);
            if (lane == 0 && key2) atomicMax(s_rbits + 1, key2);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned long long* conv = (unsigned long long*)(A.sync + A.conv_off) + 2 * ((int64_t)it.li * A.max_sweeps + sweeps);
            unsigned* arrive = A.sync + A.arrive_off + it.li * A.max_sweeps + sweeps;
            unsigned long long mx = s_rbits[0], mt = s_rbits[1];
            if (P > 1) {
                const unsigned long long old = __hip_atomic_fetch_max(conv, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long old2 = __hip_atomic_fetch_max(conv + 1, mt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the maxima have been applied before this workgroup arrives
                (void)old;
                (void)old2;
                __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (ring_wait_ge(arrive, (unsigned)P, fail)) {
                    mx = __hip_atomic_load(conv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    mt = __hip_atomic_load(conv + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else *s_ok = 0;
            }
            s_rbits[0] = mx;
            s_rbits[1] = mt;
        }
        __syncthreads();
        ok = *s_ok != 0;
        ++sweeps;
        done = jacobi_last_sweep(__longlong_as_double((long long)s_rbits[0]), __longlong_as_double((long long)s_rbits[1]), A.tol);
        __syncthreads();
        JAC_T(RING_PROF, p7);
        JAC_ACC(RING_PROF, prof, 5, p6, p7);
    }
#ifdef HTN_RING_PROF
    if (tid == 0 && blockIdx.x < 256) {
        prof[6] = wall_clock64() - prof_t0;
        prof[7] = (local ? 1000000 : 0) + sweeps * 1000 + P;
        long long prof_c1;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(prof_c1)::"memory");
        prof[15] = prof_c1 - prof_c0;
        for (int q = 0; q < 16; ++q) g_ring_prof[blockIdx.x * 16 + q] = prof[q];
    }
#endif
    // ---- result: column norms -> S, columns (pivoting undone) -> G; the panels are wherever the tournament left them ----
    double2* __restrict__ g = A.G + D.g_off;
    const int* __restrict__ pc = A.perm + it.li * 64 * JAC_MAXEL;
    for (int side = 0; side < 2; ++side) {
        const double2* buf = side ? bufB : bufT;
        const int q = side ? s_bot[k] : s_top[k];
        const int nc = ncols(q);
        for (int c = wave; c < nc; c += RING_THREADS / 64) {
            const int col = q * w + c;
            double sn = 0.0;
            for (int i = lane; i < m; i += 64) {
                const double2 x = buf[c * mp + i];
                sn += x.x * x.x + x.y * x.y;
                g[(int64_t)col * m + pc[i]] = x;
            }
            sn = wave_sum(sn);
            if (lane == 0) A.S[D.s_off + col] = sqrt(sn);
        }
    }
    for (int col = n + k * (RING_THREADS / 64) + wave; col < D.n; col += P * (RING_THREADS / 64)) {      // columns beyond the rank: zero
        for (int i = lane; i < m; i += 64) g[(int64_t)col * m + i] = make_double2(0.0, 0.0);
        if (lane == 0) A.S[D.s_off + col] = 0.0;
    }
    if (k == 0 && tid == 0) {
        A.info[A.large_ids[it.li]] = (done && ok) ? sweeps : -(sweeps > 0 ? sweeps : 1);
        A.sweeps_out[it.li] = ok ? sweeps + ((local || P == 1) ? 1000 : 0) : 0;      // (+ 1000: hand-offs went through one XCD's L2)
        __threadfence_system();
    }
}

__global__ __launch_bounds__(RING_THREADS) void k_jacobi_ring(RingArgs A) {
    extern __shared__ double2 g_lds[];
    __shared__ int s_top[RING_MAX_P], s_bot[RING_MAX_P];
    __shared__ unsigned long long s_rbits[2];                // the sweep's largest squared cosine | largest tan^2, as bits
    __shared__ int s_ok, s_local;
    __shared__ double s_bnorm[3 * (RING_THREADS / 16)];      // tracked squared norms | scales of the bottom panel's columns | norms of a received top panel
    __shared__ unsigned s_arr[2];                            // direct receive: the epoch whose top / bottom panel has arrived
    const RingItem it = A.items[blockIdx.x];
    if (it.P <= 0) return;           // (a gap of the XCD-aware placement: see plan_ring)
    const htn_svd_block D = A.desc[A.large_ids[it.li]];
    const int m = D.m;
    const int gs = ring_gs(m), E = ring_e(m);
#define RING_CASE(GSV, EV) \
    case EV: ring_run<GSV, EV>(A, it, D, g_lds, s_top, s_bot, s_rbits, &s_ok, s_bnorm, &s_local, s_arr); break;
    if (gs == 16) {                  // m <= 256
        switch (E) {
            RING_CASE(16, 1) RING_CASE(16, 2) RING_CASE(16, 3) RING_CASE(16, 4) RING_CASE(16, 5) RING_CASE(16, 6) RING_CASE(16, 7)
            RING_CASE(16, 8) RING_CASE(16, 9) RING_CASE(16, 10) RING_CASE(16, 11) RING_CASE(16, 12) RING_CASE(16, 13)
            RING_CASE(16, 14) RING_CASE(16, 15)
            default: ring_run<16, 16>(A, it, D, g_lds, s_top, s_bot, s_rbits, &s_ok, s_bnorm, &s_local, s_arr);
        }
    } else {                         // 256 < m <= 512: E = 5 .. 8
        switch (E) {
            RING_CASE(64, 5) RING_CASE(64, 6) RING_CASE(64, 7)
            default: ring_run<64, 8>(A, it, D, g_lds, s_top, s_bot, s_rbits, &s_ok, s_bnorm, &s_local, s_arr);
        }
    }
#undef RING_CASE
}
