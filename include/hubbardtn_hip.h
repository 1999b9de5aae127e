/* hubbardtn_hip.h -- C ABI of libhubbardtn_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the two-site DMRG hot path that HubbardTN reaches through
 *     find_groundstate(psi0, H, IDMRG2(...))            src/HubbardFunctions.jl:1010
 * i.e. the work MPSKit 0.13.1 / TensorKit 0.14.6 / KrylovKit 0.9.5 do per bond update
 * (SURVEY.md section 8a rows a7-a10).  Those packages are not vendored under /root/reference;
 * each entry point below names the dependency routine it stands in for and the reference call
 * site that reaches it.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; sizes are element counts
 *   - complex128 = interleaved (re, im) doubles, exactly Julia's Vector{ComplexF64}
 *     (src/HubbardFunctions.jl:264 ff. build every TensorMap as ComplexF64)
 *   - matrices are column-major with an explicit leading dimension (TensorKit block layout)
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued, nothing synchronises
 *     unless stated
 *   - return value 0 = ok, otherwise htn_last_error() (thread-local) describes the failure
 *   - no exceptions cross the boundary; no global mutable state except the error string
 */
#ifndef HUBBARDTN_HIP_H
#define HUBBARDTN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HTN_ABI_VERSION 2
#define HTN_MAX_BUFS 8
#define HTN_TILE 32              /* output tile edge of the grouped GEMM */
/* grouped GEMM: one 4-wave workgroup per tile, several co-resident per CU; a tile of q = 1, 2 or 4 quadrants (16 x 16)
 * splits its K slabs 4 / q ways over its waves (htn_gemm.hip). */

/* operand ops */
#define HTN_OP_N 0               /* as stored                        */
#define HTN_OP_T 1               /* transposed                       */
#define HTN_OP_C 2               /* conjugate transposed             */
/* segment types */
#define HTN_SEG_GEMM 0           /* C += alpha * op(A) * op(B)       */
#define HTN_SEG_COPY 1           /* C += alpha * B  (B is m x n)     */

/* One output tile (<= 32 x 32) of an output block.  The tile owns segs[seg_begin .. +seg_count)
 * and is WRITTEN (not accumulated): a tile with no segments stores zeros.  Within that range all
 * GEMM segments come first and the last pad[0] entries are the COPY segments.  pad[1] = 1 promises that every
 * GEMM segment of the tile has k <= 16 (one K slab): the kernel then walks the list without reading it. */
typedef struct {
    int64_t c_off;      /* element offset of the BLOCK origin inside bufs[buf_c]   */
    int32_t buf_c;      /* index into the buffer table                              */
    int32_t ldc;
    int32_t m, n;       /* extent of this tile (1..32)                              */
    int32_t row0, col0; /* tile origin inside the block                             */
    int32_t seg_begin, seg_count;
    int32_t pad[2];
    /* split-K across workgroups (nparts > 1; 0 or 1 = the record is the whole tile): this record is part `part` of
     * `nparts` records that share one output tile and own consecutive ranges of its segment list (COPY segments in the
     * last part).  The parts meet through bufs[HTN_BUF_WS]: int32 tickets[HTN_WS_TICKET_ELEMS * 4] (zero before the
     * launch, reset by the kernel) followed by 32 x 32 complex128 slabs; the part drawing ticket nparts - 1 adds the
     * slabs ws_slot .. ws_slot + nparts - 1 in part order and writes the tile. */
    int32_t part, nparts;
    int32_t ws_slot;    /* first slab of this tile                                   */
    int32_t ticket;     /* index of this tile's ticket counter                       */
} htn_tile;             /* 64 bytes */
#define HTN_BUF_WS 7                 /* buffer-table slot of the split-K workspace   */
#define HTN_WS_TICKET_ELEMS 4096     /* complex128 elements reserved for the tickets (64 KiB = 16384 counters) */
/* workspace size in complex128 elements for a task list using n_slots slabs */
#define HTN_WS_ELEMS(n_slots) (HTN_WS_TICKET_ELEMS + (int64_t)(n_slots) * HTN_TILE * HTN_TILE)

/* One contribution  alpha * op(A)[block rows, 0:k] * op(B)[0:k, block cols]  to an output block.
 * op(A) is (block rows x k), op(B) is (k x block cols); offsets address element (0,0) of op(.). */
typedef struct {
    int64_t a_off, b_off;
    int32_t buf_a, buf_b;
    int32_t lda, ldb;
    int32_t k;
    int32_t op_a, op_b;
    int32_t type;
    double alpha_re, alpha_im;
} htn_seg;              /* 64 bytes */

const char* htn_last_error(void);
int htn_abi_version(void);

/* Binds the calling thread to a device and returns its properties (name buffer >= 256 bytes). */
int htn_device_init(int device, char* name_host, int* cu_count_host);

/* Grouped, segmented complex128 GEMM on v_mfma_f64_16x16x4_f64.
 * Stands in for: TensorKit block mul! (BLAS zgemm per coupled sector) + the TensorOperations /
 * Strided permutes around it, as executed inside MPSKit's AC2 effective-Hamiltonian apply and
 * environment transfers (reached from src/HubbardFunctions.jl:1010).
 * bufs_host: HTN_MAX_BUFS device base pointers (unused entries may be NULL). */
int htn_grouped_gemm_z(const void* const* bufs_host, const htn_tile* tiles, int32_t n_tiles,
                       const htn_seg* segs, void* stream);

/* Krylov vector algebra (stands in for VectorInterface inner/add!!/scale!! on TensorMaps as used
 * by KrylovKit.eigsolve(..., Lanczos)).  The reduced data are stored in the
 * Euclidean ("tilde") normalisation, so TensorKit's dim-weighted inner product is the plain dot.
 *   out[i]  = sum_j conj(V[i*ldv + j]) * w[j]        i < nvec      (deterministic 2-stage reduce)
 *   w[j]   += sign * sum_i coef[i] * V[i*ldv + j]
 * scratch must hold htn_dots_scratch_elems(nvec) complex128. */
int64_t htn_dots_scratch_elems(int32_t nvec);
int htn_dots_z(const void* V, int64_t ldv, int32_t nvec, const void* w, int64_t n,
               void* out, void* scratch, void* stream);
int htn_axpys_z(void* w, const void* V, int64_t ldv, int32_t nvec, const void* coef,
                double sign, int64_t n, void* stream);
/* dst[j] = src[j] / sqrt(Re(nrm2[0]))  (nrm2 on device; dst may alias src) */
int htn_scale_inv_sqrt_z(void* dst, const void* src, const void* nrm2, int64_t n, void* stream);

/* Device-resident Lanczos: lowest eigenpair of the Hermitian map y = H_eff x given as a short sequence of
 * grouped-GEMM launches (stage list; the buffer-table entries x_slot / y_slot are replaced by the current
 * Krylov vector / the output vector for every matvec).
 * Stands in for: KrylovKit.eigsolve(H_eff, x0, 1, :SR, Lanczos(krylovdim, tol, eager=true)) as called by
 * MPSKit's two-site update (reached from src/HubbardFunctions.jl:1010): orthonormal Krylov
 * basis kept in full, explicit two-pass reorthogonalisation, tridiagonal problem solved after every expansion,
 * stop when |beta_j y_j| < tol, restart from the Ritz vector at krylovdim (2 <= krylovdim <= 31).
 * V: (krylovdim + 2) * n complex128; on entry V[0:n] = start vector, on exit V[0:n] = normalised Ritz vector.
 * The scalar results are final on return; the kernels that write V[0:n] (and possibly one speculative step that writes
 * another row of V) may still be IN FLIGHT on `stream`: read V, free or reuse V, scratch and the stage buffers in stream
 * order or after a synchronisation.  n_matvec counts the matvec launches enqueued (HTN_LANCZOS_CLOSE=never|always|auto in
 * the environment decides which steps are followed by a speculative one: never the results, only this count).
 * exchange (may be NULL): called on the host after each matvec has been ENQUEUED, with the device pointer of y;
 * the multi-GPU host uses it to enqueue an RCCL all-reduce of y on the same stream (zero_y = 1 then clears y
 * before the local tiles are written).  The call synchronises the stream once per iteration (it needs
 * alpha_j, beta_j on the host). */
typedef struct {
    const void* bufs[HTN_MAX_BUFS];
    const htn_tile* tiles;
    const htn_seg* segs;
    int32_t n_tiles;
    int32_t pad;
} htn_gemm_launch;
typedef int (*htn_exchange2_fn)(void* y_dev, int64_t n, void* user);    /* != 0: failure, the solve is aborted */
int64_t htn_lanczos_scratch_elems(int32_t krylovdim);
int htn_lanczos_z(const htn_gemm_launch* stages_host, int32_t n_stages, int32_t x_slot, int32_t y_slot,
                  void* V, int64_t n, int32_t krylovdim, double tol, int32_t max_restart, void* scratch,
                  int32_t zero_y, htn_exchange2_fn exchange, void* user,
                  double* eig_host, int32_t* n_matvec_host, double* residual_host,
                  double* matvec_ms_host /* NULL, or receives the HIP-event time of all matvec launches */,
                  void* stream);
/* Lanczos with frozen rows: the lowest eigenpair of P H_eff P, P = 1 - Q Q^H, for n_frozen ORTHONORMAL device rows Q of
 * length n (row r at Q + r * n).  The start vector is projected first; every Krylov vector is orthogonalised against Q in
 * both passes of its step (the rows of a pass are Q followed by the Krylov rows); the Ritz vector is assembled from the
 * Krylov rows only and projected once more, so |Q^H x| stays at rounding.  This is a projection, not an energy penalty:
 * nothing to tune and the spectrum keeps its scale.  (Orthogonalised two-site DMRG for excited states; MPSKit reaches
 * excitations through the quasiparticle ansatz instead, src/HubbardFunctions.jl:1173-1299.)
 * The vector kernels keep one basis value per row in registers, 32 rows at most:
 *     krylovdim >= 2  and  krylovdim + n_frozen <= 31,      anything else is an error.
 * scratch: htn_lanczos_scratch_elems(krylovdim + n_frozen) elements; V and everything else as for htn_lanczos_z.
 * n_frozen = 0 (Q may be NULL) enqueues exactly what htn_lanczos_z enqueues: same bits, same matvec count. */
int htn_lanczos_orth_z(const htn_gemm_launch* stages_host, int32_t n_stages, int32_t x_slot, int32_t y_slot,
                       void* V, int64_t n, int32_t krylovdim, double tol, int32_t max_restart, void* scratch,
                       int32_t zero_y, htn_exchange2_fn exchange, void* user,
                       double* eig_host, int32_t* n_matvec_host, double* residual_host, double* matvec_ms_host,
                       const void* Q, int32_t n_frozen, void* stream);

/* Krylov exponential: x = exp(-i dt H) x0 for the Hermitian map given as stages (as for htn_lanczos_z), dt = dt_re + i dt_im
 * (dt = -i beta is imaginary time: exp(-beta H)).  Stands in for KrylovKit.exponentiate(H_eff, -i dt, x0, Lanczos(...)) as
 * MPSKit's TDVP2 calls it.  The orthonormal basis is built by the step kernels and the depth-1 pipeline of htn_lanczos_z; after
 * step m the host diagonalises the real tridiagonal T_m completely (implicit QL, m <= 31), forms c = exp(-i dt T_m) e_1 and
 * Saad's a-posteriori estimate est = beta_m |dt| |c_m|, and stops at the first m with est < tol, with beta_m < 1e-14 x (largest
 * |alpha| or beta seen: an invariant subspace, the result is exact), or at m = krylovdim.  Not converged at krylovdim: the
 * fraction s of the remaining time is halved until beta_m |s dt| |c_m(s dt)| < tol s (host work on the same T), that partial
 * step is applied and the basis is rebuilt from its result for the remaining time (the tolerance of later cycles is scaled by
 * the fraction that remains); at most max_restart restarts, then the call fails and the error names the fraction that remains.
 * Every step is applied by ONE launch, V[0] <- sum_i (c_i / |c|) V[i] in place (the basis is orthonormal, so the norm is known
 * on the host; the coefficients travel in the kernel arguments).  Nothing but the step records is read back.
 * V, scratch, krylovdim (2..31), zero_y, exchange: as for htn_lanczos_z.  On exit V[0:n] = x / |x|,
 * *growth_host = |x| / |x0| (1 to rounding for real dt), *alpha0_host = <x0|H|x0> / |x0|^2 (the first Lanczos alpha),
 * *err_host = the sum of the estimates of the steps applied, *n_matvec_host = matvecs enqueued (speculative ones included).
 * dt = 0: one matvec (alpha0), x = x0 / |x0|.  The CPU baseline library exports the symbol with host pointers and no kernels
 * (full two-pass reorthogonalisation, the same decisions). */
/* The combine launch of htn_krylov_expm_z on its own: V[0:n] <- sum_{i < nvec} coef[i] V[i * ldv : i * ldv + n] in place, nvec in
 * 1..32, coef_host = nvec complex128 (re, im pairs) in HOST memory, passed to the kernel by value: nothing is staged, the array may
 * be reused as soon as the call returns.  Rows 1.. are only read.  HIP library only. */
int htn_krylov_combine_z(void* V, int64_t ldv, int32_t nvec, const double* coef_host, int64_t n, void* stream);
int htn_krylov_expm_z(const htn_gemm_launch* stages_host, int32_t n_stages, int32_t x_slot, int32_t y_slot,
                      void* V, int64_t n, int32_t krylovdim, double dt_re, double dt_im, double tol,
                      int32_t max_restart, void* scratch, int32_t zero_y, htn_exchange2_fn exchange, void* user,
                      double* growth_host, double* alpha0_host, int32_t* n_matvec_host, double* err_host,
                      double* matvec_ms_host, void* stream);

/* Shifted linear solve (z - H) x = b for the Hermitian map given as stages (as for htn_lanczos_z), z = z_re + i z_im any finite
 * complex number (Im z < 0: the hole part of a Green's function), b = V[0:n], not normalised.  The correction-vector equation of
 * one frequency.  Method: minimal residual on the Lanczos basis (K(z - H, r) = K(H, r)), built by the step kernels and the
 * depth-1 pipeline of htn_lanczos_z.  After step m the host minimises | beta_0 e_1 - (z I~ - T~_{m+1,m}) y | by Givens rotations
 * on the (m + 1) x m complex tridiagonal matrix; the residual norm comes out of the rotations, no matvec is spent on it.  Stop at
 * |r| <= tol |b|, at beta_m < 1e-14 x (largest |alpha| or beta seen: an invariant subspace), or at m = krylovdim.  Not converged
 * there: x <- x + V_m y and the basis is rebuilt from r = V_{m+1} rho, rho = beta_0 e_1 - (z I~ - T~) y -- both updates in ONE
 * launch (htn_krylov_combine2_z); at most max_restart restarts, then the call fails and the error names the relative residual
 * that remains.  The restarted form converges for Im z != 0 (the field of values of z - H lies on the line Im = Im z); for real
 * z it may stagnate and then reports that.
 * use_guess != 0: X holds a start value x0; r0 = b - z x0 + H x0 costs one matvec and the solve is for the correction.
 * V, scratch, krylovdim (2..31), zero_y, exchange: as for htn_lanczos_z (V: at least krylovdim + 1 rows; the CPU baseline
 * library wants krylovdim + 2).  X: a caller buffer of n elements.  On exit X = x, V[0:n] = x / |x|, *norm_host = |x|,
 * *residual_host = the last relative residual |r| / |b| of the recurrence, *n_matvec_host = matvecs enqueued (the one of r0 and
 * speculative ones included).  Only step records and norms (32 bytes each) are read back.  The CPU baseline library exports the
 * symbol with host pointers and no kernels (full two-pass reorthogonalisation, the same decisions: htn_resolvent.h). */
int htn_krylov_solve_z(const htn_gemm_launch* stages_host, int32_t n_stages, int32_t x_slot, int32_t y_slot, void* V, int64_t n,
                       int32_t krylovdim, double z_re, double z_im, double tol, int32_t max_restart, void* X, int32_t use_guess,
                       void* scratch, int32_t zero_y, htn_exchange2_fn exchange, void* user, double* norm_host,
                       double* residual_host, int32_t* n_matvec_host, double* matvec_ms_host, void* stream);
/* The launch that ends a cycle of htn_krylov_solve_z on its own: X[0:n] <- (keep ? X : 0) + sum_{i < m} y[i] V[i * ldv : i * ldv + n]
 * and, with rho_host != NULL, V[0:n] <- sum_{i <= m} rho[i] V[i * ldv : ...] in place; m in 1..31, y_host = m and rho_host = m + 1
 * complex128 (re, im pairs) in HOST memory, passed to the kernel by value.  Rows 1.. are only read; without rho_host row 0 is only
 * read too.  HIP library only. */
int htn_krylov_combine2_z(void* V, int64_t ldv, int32_t m, const double* y_host, const double* rho_host, void* X, int32_t keep,
                          int64_t n, void* stream);

/* Batched one-sided Jacobi SVD of the coupled-sector blocks of a two-site tensor.
 * Stands in for: TensorKit tsvd!(t; alg=SVD()) -> LAPACK zgesvd per block (SURVEY.md 8a a9,
 * scheme chosen at src/HubbardFunctions.jl:1010 and :1363-1365).
 * For block i the m_i x n_i (column-major, ld = m_i) matrix at G + g_off[i] is overwritten by G*J
 * (mutually orthogonal columns = sigma_j u_j, UNSORTED; surplus columns of a wide block converge to 0),
 * the column norms go to S + s_off[i] and, if flags & HTN_SVD_ACCUMULATE, the n_i x n_i rotation J to
 * Vj + v_off[i] (ld = n_i).  The caller stages M or M^H (htn_batched_copy_z) so that the isometry the
 * sweep direction needs is the normalised G*J itself; the other factor is then a plain GEMM with M.
 * desc: device array of htn_svd_block, desc_host: the same array in host memory (may be NULL: then every block
 * runs on ONE CU; with it, QRCP blocks larger than one CU's LDS take the large-block path: panel-blocked pivoted QR
 * (helper workgroups share its trailing update from 160 columns on), then the ring block Jacobi -- all sweeps in ONE launch,
 * every block on several CUs whose LDS-resident column panels are handed round inside the launch (write-through stores +
 * epoch flags -- or stores kept in one XCD's L2 when all workgroups of the block read the same XCD id at run time; bounded
 * waits: a time-out is reported as an error of this call), convergence decided on the device; the
 * small blocks run beside it on an internal second stream that joins `stream` before the call returns; the call blocks
 * the host until everything has converged, results stay on the device.  Blocks the ring cannot take fall back to the
 * pair-visit block Jacobi of ABI 2 (one launch per tournament round; sweeps_hint bounds its speculative enqueue));
 * max_m_host = max_i max(m_i, pad_i).  A plain (non-QRCP) block with m_i > 512 ("tall") takes a multi-CU path: the same
 * pair-visit tournament with its columns streamed from global memory (Gram on MFMA over row chunks, fixed-order sums, U applied
 * chunk by chunk to X and, with HTN_SVD_ACCUMULATE, to J), one launch per round, sweeps_hint / sweeps_used / max_sweeps as
 * for the large blocks, no QR preconditioning (more outer sweeps); it runs on `stream` after the other blocks and needs
 * desc_host (without it m_i > 512 is an error).  Every other block must have max(m_i, pad_i) <= 512.
 * info_dev[i] receives the sweep count (<0: not converged).  A sweep ends the iteration when the largest squared
 * cosine it SAW before rotating was <= max(tol^2, 0.1 tol) (quadratic convergence: it leaves < tol^2 behind).  The blocks
 * that one workgroup takes whole (every block inside the LDS window, every block of a call without desc_host) also ask that
 * (largest tan^2 the sweep rotated by) x (that cosine^2) <= tol^2, unless nothing was rotated: inside a cluster of
 * singular values the angles are of order one and a sweep leaves the cosines it saw. */
#define HTN_SVD_ACCUMULATE 1      /* flags: also accumulate the rotation J (else Vj is not touched) */
#define HTN_SVD_QRCP 2            /* flags: the block at g_off is G0 (pad x m, ld = pad); pivoted-QR precondition it,
                                     run Jacobi on R^H (m x n, n = min(pad, m)) and write the m x n result
                                     (rows un-pivoted, ld = m) back to g_off; the v_off region (>= m*n) is scratch */
typedef struct {
    int64_t g_off, v_off, s_off;
    int32_t m, n;
    int32_t flags, pad;
} htn_svd_block;        /* 40 bytes */
/* Per-call options of htn_jacobi_svd_z (NULL = defaults); replaces the process-wide setters of ABI version 1 so
 * that two contexts on two host threads cannot see each other's settings.
 *   split_elems : blocks whose R^H (roundup(m) x n elements) exceeds it leave the one-workgroup kernel for the
 *                 large-block path (k_qr_large: panel-blocked pivoted QR; k_jacobi_pairs_gram: block Jacobi over many
 *                 CUs).  <= 0: the default ("does not fit one CU's LDS window", 9216 elements); larger values are
 *                 clamped to it.  Exists so that small problems can exercise the large-block path (tests); results
 *                 agree to the Jacobi tolerance either way.
 *   rank_cut    : rank-revealing stop of the large blocks' pivoted QR: once the squared Frobenius norm of the part
 *                 not yet factorised is below rank_cut^2 (it bounds every remaining singular value), the remaining
 *                 rows of R are dropped, the tournament runs on the rank found, and the dropped singular values are
 *                 reported as 0.  <= 0 = off (default).  Kept singular values then move by at most
 *                 rank_cut^2 / (2 sigma) (interlacing).
 *   sweeps_hint : outer sweeps the large-block path is expected to need (normally `*sweeps_used` of the previous call
 *                 for the same bond); the sweep expected to be the last is not followed by a speculatively enqueued
 *                 one.  <= 0: unknown, every sweep is enqueued one ahead of the host's knowledge.  Results do not
 *                 depend on it.
 *   sweeps_used : host pointer or NULL; receives the number of outer sweeps of the large-block path after which every
 *                 large block had converged (0 when no block took that path). */
typedef struct {
    int32_t split_elems;
    int32_t sweeps_hint;
    double rank_cut;
    int32_t* sweeps_used;
} htn_svd_opts;         /* 24 bytes */
int htn_jacobi_svd_z(void* G, void* Vj, double* S, const htn_svd_block* desc, const htn_svd_block* desc_host,
                     int32_t n_blocks, int32_t max_m_host, int32_t max_sweeps, double tol, int32_t* info_dev,
                     const htn_svd_opts* opts, void* stream);

/* dst(r x c, ldd) = op(src)(.., lds) with optional per-row / per-column real scaling:
 * generic batched strided copy used to (a) stage M or M^H into the Jacobi workspace and
 * (b) write the truncated isometries U[:, keep] / V^H[keep, :] and the centre S*V^H / U*S.
 * For each item: dst[i + j*ldd] = scale * f(src element), where
 *   op N: src[(i) + perm(j)*lds]      op C: conj(src[perm(j)... see htn_copy_item]). */
typedef struct {
    int64_t dst_off, src_off, idx_off, scl_off; /* idx/scl offsets into int32 / double side arrays; -1 = none */
    int32_t rows, cols;          /* extent of dst                                   */
    int32_t ldd, lds;
    int32_t op;                  /* HTN_OP_N: dst(i,j) = src(i, J) ; HTN_OP_C: dst(i,j) = conj(src(J', i))
                                    where the gathered index (idx side array) applies to dst's
                                    `gather_dim` (0 = rows, 1 = cols)                 */
    int32_t gather_dim;
    int32_t scale_dim;           /* 0: scale by scl[i], 1: scale by scl[j], -1: none  */
    int32_t inv_norm;            /* 1: divide by the gathered scale value instead     */
} htn_copy_item;        /* 64 bytes */
int htn_batched_copy_z(void* dst, const void* src, const int32_t* idx, const double* scl,
                       const htn_copy_item* items, int32_t n_items, double global_scale,
                       void* stream);

/* Batched unpivoted QR / LQ that FORMS the orthonormal factor: the gauge move of a one-site update (no pivoting, no
 * truncation).  Stands in for: TensorKit leftorth! / rightorth! (alg = QRpos / LQpos) per coupled sector as MPSKit's
 * one-site DMRG() calls them after each site update.
 * Block i is a strided view inside A, factorised IN PLACE (no staging copy):
 *   trans = 0 : the m x n view (m >= n, leading dimension ld) at A + offset is overwritten by Q (m x n, orthonormal
 *               columns); R (n x n upper triangular, strict lower part written as zeros) goes to Rbuf + r_offset, ld ldr.
 *   trans = 1 : the view is n x m (n rows, m >= n columns, leading dimension ld); its conjugate transpose is factorised,
 *               i.e. view = L Qr: the row-orthonormal factor Qr (n x m) goes in place, L (n x n lower triangular, strict
 *               upper part written as zeros) to Rbuf + r_offset.
 * Sign rule: the diagonal of R (of L) is real and non-negative.  A column whose remainder after projecting out the
 * columns before it falls below 1e-13 of its own norm is treated as dependent: its diagonal entry (and the rest of its
 * remainder) is an exact zero and Q is completed by a unit vector orthogonal to everything before it, so Q always has
 * orthonormal columns and Q R reproduces the view to rounding.
 * Method (HIP): left-looking, panels of HTN_QR_PANEL columns held in LDS; a panel is projected against the finished
 * columns (W = Q^H A_p, A_p -= Q W on v_mfma_f64_16x16x4_f64, Q read back through the L2) -- a second time when a column
 * lost more than half of its squared norm in the first projection --, then orthonormalised by Gram-Schmidt, always twice.  One workgroup per block, no workgroup waits for another; all sums are taken
 * in a fixed order, so the result is bit-reproducible.  m is limited by the LDS panel: m <= HTN_QR_MAX_M.
 * The CPU baseline library exports the same entry on host memory (Householder reflections, same conventions).
 * desc: device array; desc_host: the same array in host memory (needed: it sizes the launch). */
#define HTN_QR_PANEL 16          /* panel width while a panel of m rows fits the LDS (m <= 464); halved beyond, down to 1 */
#define HTN_QR_CHUNK 512         /* rows covered by one pass of the workgroup's row-owning loops (one row per thread)   */
#define HTN_QR_MAX_M 7664
typedef struct {
    int64_t offset;              /* element offset of the view inside A                   */
    int32_t m, n;                /* long and short extent, m >= n >= 1                    */
    int32_t ld, pad;
    int64_t r_offset;            /* element offset of R (L) inside Rbuf                   */
    int32_t ldr, trans;
} htn_qr_block;         /* 40 bytes */
int htn_qr_blocks_z(void* A, void* Rbuf, const htn_qr_block* desc, const htn_qr_block* desc_host, int32_t n_blocks,
                    void* stream);


/* Batched block trace-dots: the pairing of a left environment (blocks stored [n_bra x n_ket]) with right environments
 * (blocks stored [n_ket x n_bra]) that closes a two-point correlation function on a bond (htn_mps_correlator).  The sum
 * runs over A[r, c] * B[c, r]: one operand is read transposed and nothing is conjugated, which htn_dots_z cannot express.
 *   out[o] = sum over items with item.out == o, in list order, of
 *            w * sum_{r,c} A[a_off + r + c*lda] * B[b_off + c + r*ldb];       results with no item are written as 0
 * Two stages, no floating-point atomics: every item is cut into 32 x 32 tiles, the tiles are dealt to HTN_TRDOT_SLOTS
 * work units per item (one workgroup each, so a large block does not serialise the launch; the B tile goes through LDS so
 * that both operands are read along their contiguous direction), each unit adds its tiles in a fixed order; the second
 * stage adds the units of an item in slot order and the items of a result in list order.  Repeated calls are bit-identical.
 * Any sizes: blocks of one row or one column and blocks that are no multiple of the tile are fine; n_items = 0 writes zeros.
 * items: device array; scratch: htn_trdots_scratch_elems(n_items) complex128. */
#define HTN_TRDOT_SLOTS 16
typedef struct {
    int64_t a_off, b_off;       /* element offsets into A and B                                       */
    int32_t rows, cols;         /* A block: rows x cols, column-major, lda; B block: cols x rows, ldb */
    int32_t lda, ldb;
    int32_t out;                /* index of the result this item adds to                              */
    int32_t pad[3];             /* (pads the record to 64 bytes, the size of the other task records)  */
    double w_re, w_im;          /* weight                                                             */
} htn_trdot_item;               /* 64 bytes */
int64_t htn_trdots_scratch_elems(int32_t n_items);
int htn_block_trdots_z(const void* A, const void* B, const htn_trdot_item* items, int32_t n_items,
                       void* out, int32_t n_out, void* scratch, void* stream);


/* Block placement: builds a block-sparse tensor out of scaled blocks of another one (the site tensors of a state a local
 * operator was applied to: htn_mps_apply_op, htn_mps_transition).  Per item
 *   dst[dst_off + r + c*ldd] = coef * src[src_off + r + c*lds]   (0 <= r < rows, 0 <= c < cols),   or 0 when src_off = -1;
 * column-major complex128, coef real (one rounding per component).  htn_batched_copy_z has one scale per launch and cannot
 * zero-fill.  The items of a launch are expected to tile their destination exactly once, so no memset precedes it; nothing
 * outside the items' views is written.  Items are cut into 32 x 32 tiles that are dealt over the workgroups of the launch
 * (a large block is shared by all of them, many small ones share a workgroup); every element is written by exactly one
 * thread, no atomics, repeated calls are bit-identical.  n_items = 0 is a no-op.  items: device array. */
typedef struct {
    int64_t dst_off, src_off;   /* element offsets into dst and src; src_off = -1: write zeros        */
    int32_t rows, cols, ldd, lds;
    double coef;
    int32_t pad[6];             /* (pads the record to 64 bytes, the size of the other task records)  */
} htn_place_item;               /* 64 bytes */
int htn_block_place_z(void* dst, const void* src, const htn_place_item* items, int32_t n_items, void* stream);


/* Batched null-space projection: what is left of a block outside the range of an isometry, and how much was removed.  The
 * projected residuals of the two-site energy variance (htn_mps_variance): y (1 - A A^H) from the left, (1 - B^H B) from the right.
 * Per item R is an m x n view (column-major complex128, leading dimension ldr) inside `R`, Q a view inside `Q`:
 *   side 0 : Q is m x k with orthonormal columns (ldq >= m):  W = Q^H R,  R <- R - Q W
 *   side 1 : Q is k x n with orthonormal rows    (ldq >= k):  W = R Q^H,  R <- R - W Q
 * Every projection is applied TWICE (an isometry that is orthonormal to 1e-12 leaves that much of the removed part behind in
 * one pass; a residual of 1e-7 of the block would drown in it).  Per result o two real numbers, sums over the items with
 * item.out == o in list order:
 *   out[2 o]     = |W|_F^2 of the FIRST pass (the removed coefficients)
 *   out[2 o + 1] = |R|_F^2 after the second pass
 * results with no item are written as 0.  k = 0 is a pure norm (R is not written); m = 0 or n = 0 contributes nothing.
 * Work unit (HIP): (item, 16-column chunk of R) for side 0, (item, 16-row chunk) for side 1 -- HTN_NULLPROJ_UNITS per item --,
 * one workgroup each; units touch disjoint parts of R, so a large block spreads over the device and no workgroup waits for
 * another.  Inside a unit Q is taken in rounds of 64 columns (rows): the four waves form their shares of W over a quarter of
 * the long dimension each on v_mfma_f64_16x16x4_f64, the shares are added in wave order in LDS, then every wave updates 16-row
 * tiles of the chunk with the same instruction; any k >= 0.  No floating-point atomics: every unit stores its two partial
 * sums, a second launch adds the units of an item in unit order and the items of a result in list order.  Repeated calls are
 * bit-identical; nothing outside the R views is written.
 * items: device array; items_host: the same array in host memory (needed: it sizes the launch); scratch: 2 x (sum of
 * HTN_NULLPROJ_UNITS over the items) doubles.  The CPU baseline library exports the same entry on host memory (plain loops,
 * the same two passes and outputs; items and scratch may be NULL there). */
#define HTN_NULLPROJ_UNITS(m, n, side) ((m) <= 0 || (n) <= 0 ? 0 : (((side) ? (m) : (n)) + 15) / 16)
typedef struct {
    int64_t r_off, q_off;       /* element offsets of the views inside R and Q                        */
    int32_t m, n, k;            /* R: m x n; Q: m x k (side 0) or k x n (side 1)                      */
    int32_t ldr, ldq;
    int32_t side;
    int32_t out;                /* index of the result this item adds to                              */
    int32_t pad[5];             /* (pads the record to 64 bytes, the size of the other task records)  */
} htn_nullproj_item;            /* 64 bytes */
int htn_block_nullproj_z(void* R, const void* Q, const htn_nullproj_item* items, const htn_nullproj_item* items_host,
                         int32_t n_items, double* out, int32_t n_out, void* scratch, void* stream);


/* One site of perfect sampling (Ferris, Vidal, Phys. Rev. B 85, 165146) for a batch of samples: the step htn_mps_sample takes per
 * site.  Every sample b carries a bond density matrix: one n_c x n_c column-major block (ld n_c) per sector c
 * of the site's left bond, sample b at rho + b * rho_stride.  Per item -- one stored sub-block A[(l, s); r] of the site tensor,
 * an n_l x n_r view (ld lda) inside `A`, shared by all samples -- and sample three launches do
 *   probe    T = rho_l A                                  (n_l x n_r, ld n_l, at T + b * t_stride + t_off) and, per work unit,
 *            the partial sum of Re<A, T> = Re sum conj(A[i, j]) T[i, j];
 *   choose   p(s) = sum over the items with that s, in list order, of coef x (the item's units in unit order), P = sum_s p(s) in
 *            the order s = 0 .. n_site - 1;  measure != 0: s* = the smallest s with p(s) > 0 whose cumulative sum p(0) + .. + p(s)
 *            is >= u[b] P (the last s with p(s) > 0 if rounding leaves none), choice[b] = s*, logp[b] += log(p(s*) / P),
 *            scale = 1 / p(s*);  measure == 0 (the site is traced): choice[b] = -1, logp[b] is left alone, scale = 1 / P;
 *   close    rho'_r = scale x sum over the run of items with that out_off, in list order, of coef A^H T  (n_r x n_r, ld n_r, at
 *            rho_next + b * rho_next_stride + out_off), items with s != s* left out when the site is measured.  A run no item of
 *            which is taken is written as zeros; what no run covers is not written.
 * Items with the same out_off must follow one another (the first of a run owns its close units).  probe_unit0 / close_unit0 are
 * the running sums of HTN_SAMPLE_UNITS(n_l, n_r) over the items and of HTN_SAMPLE_UNITS(n_r, n_r) over the first items of the
 * runs (every later item of a run carries the value of the next run's first item); the entry checks them against items_host.
 * Work unit = 64 rows x 16 columns of one output block of one sample = one workgroup of four waves, each a 16 x 16 tile on
 * v_mfma_f64_16x16x4_f64 with operands read through the L2 (the site tensor is shared by the batch); grid = units x samples.
 * No floating-point atomics, every sum in a fixed order: a sample's result does not depend on the batch it runs in and
 * repeated calls are bit-identical.  Nothing synchronises with the host; nothing outside the T, rho' views, choice[0 .. n_samples)
 * and logp[0 .. n_samples) is written.  u, choice, logp: device arrays of n_samples entries; items: device array, items_host
 * the same array in host memory (it sizes the launches); scratch: HTN_SAMPLE_SCRATCH_DOUBLES doubles; n_site <= HTN_MAX_SITE,
 * n_samples <= 65535.  HIP library only. */
#define HTN_SAMPLE_UNITS(m, n) ((m) <= 0 || (n) <= 0 ? 0 : (((m) + 63) / 64) * (((n) + 15) / 16))
#define HTN_SAMPLE_SCRATCH_DOUBLES(probe_units, n_samples) (((int64_t)(probe_units) + 1) * (int64_t)(n_samples))
typedef struct {
    int64_t rho_off;            /* rho_l inside a sample's rho                                         */
    int64_t a_off;              /* the sub-block inside A                                              */
    int64_t t_off;              /* T_s of this sub-block inside a sample's T                           */
    int64_t out_off;            /* rho'_r inside a sample's next rho                                   */
    int32_t n_l, n_r, lda;
    int32_t s;                  /* site multiplet of the sub-block, 0 .. n_site - 1                    */
    int32_t probe_unit0;        /* number of the item's first probe unit                               */
    int32_t close_unit0;        /* number of the first close unit of the item's run                    */
    double coef;                /* coefficient of the identity on this sub-block in a left-environment step */
} htn_sample_item;              /* 64 bytes */
int htn_sample_step_z(void* rho_next, const void* rho, const void* A, void* T, const htn_sample_item* items,
                      const htn_sample_item* items_host, int32_t n_items, int32_t n_site, int32_t n_samples,
                      int64_t rho_stride, int64_t rho_next_stride, int64_t t_stride, const double* u, int32_t measure,
                      int32_t* choice, double* logp, void* scratch, void* stream);


/* =====================================================================================================
 * Bond-update / sweep level (ABI 2): what sits behind
 *     find_groundstate(psi0, H, IDMRG2(; trscheme, tol))          src/HubbardFunctions.jl:1010
 * i.e. MPSKit's two-site sweep body.  The Hamiltonian builder
 * (hamiltonian(), src:386-472, 811-910) and initialize_mps (src:917-959) stay on the host-language side, exactly as
 * in the reference; they hand over
 *   - the MPO as tables: per site the (dN, 2k) labels of its left / right virtual levels and a list of
 *     (left level, right level, site-operator id, coefficient) entries; site operators as reduced matrix elements;
 *   - the MPS as TensorKit-shaped data: one flat ComplexF64 vector per site + a table of sub-blocks
 *     (left sector, site multiplet, right sector, offset, leading dimension) -- TensorKit's per-fusion-tree views --
 *     and per bond the int32 sector labels (N, 2S) with their int32 multiplet counts (htn_sector).
 * Everything below that -- sector layouts, recoupling coefficients (closed-form 9j), task lists, theta formation,
 * Lanczos, per-sector SVD, the global truncation rule, write-back, environment transfer, the sweep loop -- runs
 * inside the library (C++ planner + HIP kernels; one host thread per context).
 * Host pointers end in _host; everything is copied at the call, the caller keeps ownership of its buffers.
 * ===================================================================================================== */
typedef struct htn_ctx htn_ctx;
typedef struct htn_mpo htn_mpo;
typedef struct htn_mps htn_mps;

/* Symmetry of the reduced tensors (src:245-382).  Sector label = (N, j):
 *   HTN_SYM_SU2_U1 : fZ2 x SU(2) x U(1) (src:250): N = particle number (parity = N mod 2), j = 2S, spins couple
 *   HTN_SYM_U1_U1  : fZ2 x U(1) x U(1)  (src:247): N = particle number, j = 2 Sz (additive, may be negative)
 *   HTN_SYM_SU2    : fZ2 x SU(2)        (src:341): N = parity (mod 2), j = 2S
 * site_N / site_j: labels of the n_site site multiplets (3 or 4). */
#define HTN_SYM_SU2_U1 0
#define HTN_SYM_U1_U1 1
#define HTN_SYM_SU2 2
#define HTN_MAX_SITE 4
typedef struct {
    int32_t kind;
    int32_t n_site;
    int32_t site_N[HTN_MAX_SITE];
    int32_t site_j[HTN_MAX_SITE];
} htn_symmetry;

/* reduced site operator: irreducible tensor of rank k/2 (SU(2) kinds; U1_U1: k = change of 2Sz) changing N by dN;
 * red[out * HTN_MAX_SITE + in] = reduced matrix element <out || O || in> in the convention of src:281-293
 * (isometric fusion tensors: c+ has 1 and sqrt(2)). */
typedef struct {
    int32_t k, dN;
    double red[HTN_MAX_SITE * HTN_MAX_SITE];
} htn_site_op;

typedef struct {
    int32_t wl, wr;          /* level on the left / right MPO bond of this site */
    int32_t op;              /* index into the site-operator table             */
    int32_t pad;
    double coef_re, coef_im;
} htn_mpo_entry;

/* one sub-block of a site tensor inside the caller's flat vector: A[(l, s) ; r] as an n_l x n_r column-major
 * matrix at data[off] with leading dimension ld (TensorKit fusion-tree view) */
typedef struct {
    int32_t lN, lj, s, rN, rj;
    int32_t ld;
    int64_t off;
} htn_subblock;

typedef struct {
    int32_t N, j, count;
} htn_sector;

/* truncation + solver settings of one bond update / sweep */
typedef struct {
    int32_t chi_full;          /* truncdim(D), src:1363-1365, in TensorKit dim units (sum (2S+1) n); <= 0: off      */
    int32_t weighting;         /* order at the truncdim cut: 0 = sqrt(2S+1) x Schmidt value, 1 = Schmidt value       */
    double cutoff;             /* truncbelow(eta), src:1007-1010: keep Schmidt values > eta; 0: off                  */
    int32_t krylovdim;         /* 30 (KrylovKit / MPSKit default)                                                    */
    int32_t maxrestart;
    double lanczos_tol;
    double jacobi_tol;         /* 1e-14 */
    int32_t jacobi_max_sweeps; /* 40 */
    int32_t svd_split_elems;   /* htn_svd_opts.split_elems; 0 = default */
    double rank_cut;           /* 0 = off (parity-exact); see DESIGN.md section 4 */
    int32_t profile;           /* 1: synchronise around the stages so that the t_* fields are GPU-inclusive          */
    int32_t pad;
} htn_sweep_opts;

typedef struct {
    int32_t bond, direction;
    int32_t n_matvec, jacobi_sweeps;
    int32_t chi_full, multiplets;
    int32_t n_tiles, n_segs;
    int64_t theta_size;
    int64_t apply_flops, apply_bytes, svd_flops;
    double energy, residual, trunc_weight;
    double t_plan, t_lanczos, t_svd, t_env, t_total;   /* host wall seconds per stage */
    double matvec_ms;                                    /* HIP-event time of the H_eff apply launches (if timed) */
} htn_bond_stats;

/* context: one device, one stream (NULL: the library creates its own), one host thread at a time.
 * backend: HTN_BACKEND_HIP is the product.  libhubbardtn_cpu.so (built from oracle/cpu_backend, the CPU baseline of
 * SURVEY 8d) exports the same ABI with HTN_BACKEND_CPU; neither library contains the other's backend and nothing
 * falls back. */
#define HTN_BACKEND_CPU 0
#define HTN_BACKEND_HIP 1
int htn_ctx_create(int32_t backend, int32_t device, void* stream, htn_ctx** out);
void htn_ctx_destroy(htn_ctx* ctx);
int htn_ctx_backend(const htn_ctx* ctx);
/* record HIP events around every H_eff apply launch (htn_bond_stats.matvec_ms); costs two event records per matvec */
int htn_ctx_set_timing(htn_ctx* ctx, int32_t on);

/* sector-parallel effective-H apply: rank r of `world` computes output tiles r, r + world, ... of every
 * apply and the partial results are summed by ONE all-reduce per matvec on the context's stream.
 *  - htn_comm_unique_id + htn_ctx_set_comm: RCCL over xGMI, called from inside the library (HIP backend);
 *    the 128-byte id is created on rank 0 and distributed by the caller (torch.distributed, MPI, a file, ...)
 *  - htn_ctx_set_exchange: caller-supplied reduction (host callback, invoked after each matvec has been enqueued
 *    with the device pointer of y); a non-zero return aborts the solve.  Used by the gloo/CPU rehearsal tests. */
#define HTN_COMM_ID_BYTES 128
int htn_comm_unique_id(void* id_host);
int htn_ctx_set_comm(htn_ctx* ctx, int32_t rank, int32_t world, const void* id_host);
int htn_ctx_set_exchange(htn_ctx* ctx, int32_t rank, int32_t world, htn_exchange2_fn fn, void* user);

/* MPO of a chain of nsites sites.  level_ptr[nsites + 2]: levels (dN, k pairs) of bond b (between site b-1 and b,
 * b = 0 .. nsites) are levels[2 * level_ptr[b] .. 2 * level_ptr[b + 1]); entry_ptr[nsites + 1]: entries of site i.
 * Level 0 of an interior bond is the identity "nothing applied yet", the last level "term complete" (Jordan form,
 * SURVEY App. A.3); the boundary bonds hold exactly one level. */
int htn_mpo_create(htn_ctx* ctx, const htn_symmetry* sym, int32_t nsites, const htn_site_op* ops_host, int32_t n_ops,
                   const int32_t* level_ptr_host, const int32_t* levels_host, const int32_t* entry_ptr_host,
                   const htn_mpo_entry* entries_host, htn_mpo** out);
void htn_mpo_destroy(htn_mpo* mpo);

/* MPS + environments of a finite chain (or of an iDMRG window between two blocks).  bond_ptr[nsites + 2]: sectors of
 * bond b are sectors[bond_ptr[b] .. bond_ptr[b + 1]).  Site tensors must be right-canonical for sites >= 1 (site 0
 * carries the centre), "tilde" normalised.  sub_ptr[nsites + 1] indexes `subs`; data_ptr[nsites
 * + 1] (element offsets) indexes data_host, sub-block offsets are relative to their site's start.
 * left_env / right_env (may be NULL = open end): the boundary environments in the library's block order
 * (htn_mps_env_size / htn_mps_get_env of the engine they come from). */
int htn_mps_create(htn_ctx* ctx, const htn_mpo* mpo, int32_t nsites, const int32_t* bond_ptr_host,
                   const htn_sector* sectors_host, const int32_t* sub_ptr_host, const htn_subblock* subs_host,
                   const int64_t* data_ptr_host, const void* data_host, const void* left_env_host,
                   const void* right_env_host, htn_mps** out);
void htn_mps_destroy(htn_mps* mps);

/* one two-site update of sites (i, i+1) (0-based): form theta, lowest eigenpair of H_eff (optimise = 1) or
 * <theta|H|theta> only (optimise = 0: the centre is moved without optimisation), per-sector SVD + global truncation,
 * write back (placement 0 'right': A_i = U, centre S V^H on i+1; 1 'left': centre U S on i, B_{i+1} = V^H) and
 * move the environment.  stats may be NULL. */
int htn_bond_update(htn_mps* mps, int32_t i, int32_t direction, int32_t placement, int32_t optimise,
                    const htn_sweep_opts* opts, htn_bond_stats* stats_host);
/* one sweep in MPSKit's DMRG2 order: bonds 1..L-1 rightwards, L-2..1 leftwards (2L-3 updates);
 * stats_host: 2L-3 records or NULL; energy_host receives the last eigenvalue */
int htn_dmrg2_sweep(htn_mps* mps, const htn_sweep_opts* opts, htn_bond_stats* stats_host, double* energy_host);

/* One-site DMRG at FIXED bond tables (MPSKit's DMRG(); the "re-optimise variationally at that dimension" step of
 * TruncState scheme 0, src:1351-1367): grow the bonds with two-site sweeps, converge with these.
 * htn_site_update: the centre must be on site i (htn_mps_centre).  optimise = 1: lowest eigenpair of the one-site
 * effective Hamiltonian GL W_i GR by htn_lanczos_z, the Lanczos vector being the site's stored data (re-laid to left
 * layout for direction +1, to right layout for -1); optimise = 0: <x|H_eff|x> only.  direction +1: QR per right sector
 * (htn_qr_blocks_z), site i becomes the left isometry Q, site i+1 <- R B_{i+1}, the left environment moves; -1: LQ per
 * left sector, A_{i-1} <- A_{i-1} L, the right environment moves; 0: the centre stays.  Bond tables never change; a
 * sector block with fewer rows than columns (possible only in a state no two-site sweep has shaped) is an error that
 * says "run a two-site sweep first".  Nothing is truncated, so the eigenvalue IS <psi|H|psi> of the stored state.
 * stats (may be NULL): bond = the bond crossed, t_svd = the QR + absorption, jacobi_sweeps = trunc_weight = 0.
 * htn_mps_spectrum keeps the Schmidt values of the last TWO-SITE update of a bond: one-site updates do not refresh it.
 * Refused (not verified): states with attached orthogonal states, contexts with a communicator or an exchange hook.
 * htn_dmrg1_sweep: sites 0..L-2 rightwards, then L-1..1 leftwards (2L-2 updates, stats_host: 2L-2 records or NULL);
 * the centre ends on site 0, the convention every other call expects after a sweep; energy_host: the last eigenvalue. */
int htn_site_update(htn_mps* mps, int32_t i, int32_t direction, int32_t optimise, const htn_sweep_opts* opts,
                    htn_bond_stats* stats_host);
int htn_dmrg1_sweep(htn_mps* mps, const htn_sweep_opts* opts, htn_bond_stats* stats_host, double* energy_host);
/* site that carries the centre (0 after htn_mps_create and after every sweep) */
int32_t htn_mps_centre(const htn_mps* mps);
/* y = H_eff(site i) x on host vectors in the stored layout of site i (size htn_mps_site_theta_size = htn_mps_site_size;
 * sub-block table: htn_mps_get_site); the centre must be on site i.  Tests and Hermiticity checks. */
int64_t htn_mps_site_theta_size(htn_mps* mps, int32_t i);
int htn_heff1_apply(htn_mps* mps, int32_t i, const void* x_host, void* y_host);

/* Time evolution of a finite chain: two-site TDVP (Haegeman et al., Phys. Rev. B 94, 165116; MPSKit's TDVP2).  dt = dt_re + i dt_im
 * travels as arguments (htn_sweep_opts keeps its layout); dt = -i beta evolves in imaginary time.  From opts: the truncation,
 * krylovdim (2..31), lanczos_tol (the tolerance of htn_krylov_expm_z), maxrestart, the SVD settings.
 * htn_bond_evolve: htn_bond_update with the eigen-solve replaced by theta <- exp(-i dt H_eff2) theta; SVD, truncation by opts,
 *   write-back (placement as there) and environment move are the same, the centre is renormalised after the truncation.
 *   stats: energy = <theta|H_eff2|theta> BEFORE the step (the first Lanczos alpha), residual = the error estimate, n_matvec,
 *   trunc_weight.  The norm change |x| / |x0| of the exponential is NOT returned by htn_bond_evolve / htn_site_evolve (the state is
 *   renormalised and htn_bond_stats has no field for it): a caller who needs it -- imaginary time -- uses htn_tdvp2_sweep, whose
 *   log_norm_host sums it over the sweep.
 * htn_site_evolve: the centre must be on site i; exp(-i dt H_eff1) on the stored site vector in place (the one-site stages of
 *   htn_site_update with direction 0): no QR, the centre stays.
 * htn_tdvp2_sweep: one symmetric second-order step of length dt.  Rightwards i = 0 .. L-2: bond_evolve(i, dt/2) placement right,
 *   then (i < L-2) site_evolve(i+1, -dt/2); leftwards i = L-2 .. 0: bond_evolve(i, dt/2) placement left, then (i > 0)
 *   site_evolve(i, -dt/2).  The centre must be on site 0 and ends there.  stats_host: 2L-2 records or NULL, the n_matvec of a
 *   record includes the backward site step that follows it; energy_host = the last record's energy; log_norm_host (may be
 *   NULL) = the sum of log(|x| / |x0|) over all solves of the sweep (the state itself stays normalised; 0 to rounding for real dt).
 * htn_mps_set_mpo: swaps the Hamiltonian of an existing state (a quench).  Same context, symmetry, chain length and site
 *   multiplets; the centre on site 0; open ends (no boundary environments).  The right environments are rebuilt on the device as
 *   htn_mps_create builds them and the plan cache is dropped; the state's tensors are not touched.  If building them fails the
 *   call returns the error and the state keeps its old Hamiltonian, environments and plans.  The state holds a counted
 *   reference to the new MPO and drops the one to the old.
 * Refused: contexts with a communicator or an exchange hook, states with attached orthogonal states, iDMRG windows,
 * krylovdim outside 2..31. */
int htn_bond_evolve(htn_mps* mps, int32_t i, int32_t direction, int32_t placement, double dt_re, double dt_im,
                    const htn_sweep_opts* opts, htn_bond_stats* stats_host);
int htn_site_evolve(htn_mps* mps, int32_t i, double dt_re, double dt_im, const htn_sweep_opts* opts, htn_bond_stats* stats_host);
int htn_tdvp2_sweep(htn_mps* mps, double dt_re, double dt_im, const htn_sweep_opts* opts, htn_bond_stats* stats_host,
                    double* energy_host, double* log_norm_host);
int htn_mps_set_mpo(htn_mps* mps, const htn_mpo* mpo);

/* Time evolution at FIXED bond tables: one-site TDVP (Haegeman et al., as above; MPSKit's TDVP() beside TDVP2()).  Nothing is
 * truncated: the norm and, for real dt, the energy are conserved to the tolerance of the Krylov solves and a step is exactly
 * reversible; the bond tables and the Schmidt spectra of htn_mps_spectrum stay as the last two-site update left them.
 * htn_site_evolve_move: the centre must be on site i.  site <- exp(-i fwd H_eff1) site (the solve of htn_site_evolve, in left
 *   layout for direction +1, right layout for -1), then the QR / LQ of htn_site_update: Q stays on site i, the environment moves
 *   across it, and the triangular factor C is evolved by exp(-i back H_eff0) on the bond it sits on -- H_eff0(C) = sum_w GL_w C
 *   GR_w with the environment that already holds Q (htn_heff0_apply) -- before it is absorbed into the neighbour, the new centre.
 *   direction 0 is refused (htn_site_evolve is that call).  stats (may be NULL): bond = the bond crossed, energy = the first
 *   Lanczos alpha of the site solve (<psi|H|psi> before the move), residual = its error estimate, n_matvec = site + bond
 *   matvecs, n_tiles / theta_size / apply_flops of the site apply, jacobi_sweeps = trunc_weight = 0.
 * htn_tdvp1_sweep: one symmetric second-order step of length dt.  Rightwards i = 0 .. L-2: site_evolve_move(i, +1, dt/2, -dt/2);
 *   leftwards i = L-1 .. 1: site_evolve_move(i, -1, dt/2, -dt/2), where site L-1 takes its two forward half steps as one solve
 *   of length dt; then site_evolve(0, dt/2).  The centre must be on site 0 (else an error, the state untouched) and ends there.
 *   stats_host: 2L-2 records or NULL (the last one includes the closing step on site 0); energy_host = the first alpha of that
 *   closing step; log_norm_host as for htn_tdvp2_sweep.
 * Refused: what htn_site_update and htn_tdvp2_sweep refuse (communicator or exchange hook, attached states, iDMRG windows,
 * krylovdim outside 2..31, a sector block with fewer rows than columns: "run a two-site sweep first").
 * htn_mps_bond_size: elements of a vector in BOND layout on bond b (0..L) -- one n_c x n_c column-major matrix per sector c of
 *   the bond, in the order of htn_mps_bond: the layout of the triangular factors of a gauge move.
 * htn_heff0_apply: y = H_eff0(bond b) x on host vectors in bond layout; 1 <= b <= L-1, the centre on site b-1 or b and both
 *   environments of bond b present on its table (after a gauge move across b they are).  Tests and Hermiticity checks. */
int htn_site_evolve_move(htn_mps* mps, int32_t i, int32_t direction, double fwd_re, double fwd_im, double back_re, double back_im,
                         const htn_sweep_opts* opts, htn_bond_stats* stats_host);
int htn_tdvp1_sweep(htn_mps* mps, double dt_re, double dt_im, const htn_sweep_opts* opts, htn_bond_stats* stats_host,
                    double* energy_host, double* log_norm_host);
int64_t htn_mps_bond_size(htn_mps* mps, int32_t b);
int htn_heff0_apply(htn_mps* mps, int32_t b, const void* x_host, void* y_host);

/* Frequency-space Green's functions: correction-vector sweeps.  For one z the state x is swept towards the solution of
 * (z - H) |x> = |b>, b the ONE state attached by htn_mps_set_orthogonal(x, &b, 1) (read as the right-hand side, e.g. the result
 * of htn_mps_apply_op); then <O_x' psi0|x> of all sites by htn_mps_transition.  z = E0 + omega + i eta gives the particle part;
 * the hole part solves with z = E0 - omega - i eta (Im z < 0) and flips the overall sign.
 * htn_bond_solve: htn_bond_update with the eigen-solve replaced by htn_krylov_solve_z for (z - H_eff2) theta = p, where
 *   p = amplitude(b) x O_L theta_b O_R is the row the attached-state machinery forms, BEFORE orthonormalisation, and the start
 *   value is the current theta times the state's amplitude.  theta formation, per-sector SVD, truncation by opts, write-back and
 *   the move of the H and overlap environments are those of htn_bond_update.  The stored tensors stay normalised, as in TDVP2;
 *   the norm |theta_new| of the last solve is the state's AMPLITUDE: the state is amplitude x (stored tensors), the factor
 *   htn_mps_apply_op introduced, which htn_mps_overlap and htn_mps_transition apply.  *amp_host = that amplitude,
 *   bx_host[0..1] = <p|theta_new> = <b|x> before truncation.  stats: residual = the relative residual of the solve,
 *   energy = Im <p|theta_new> (the spectral weight, the quantity DDMRG converges), the rest as for a bond update.  opts:
 *   krylovdim (2..31), lanczos_tol (the tolerance of the solve), maxrestart, truncation and SVD settings.
 * htn_cv_sweep: bonds 0 .. L-2 rightwards (placement right), then L-2 .. 0 leftwards (placement left), 2L-2 records; the centre
 *   must be on site 0 and ends there.  amp_host / bx_host: those of the last bond.
 * Refused: no attached state or more than one; a context with a communicator or an exchange hook; iDMRG windows; krylovdim
 * outside 2..31.  An optimising htn_bond_update or a TDVP step on such a state does what it did before. */
int htn_bond_solve(htn_mps* x, int32_t i, int32_t direction, int32_t placement, double z_re, double z_im, const htn_sweep_opts* opts,
                   htn_bond_stats* stats_host, double* amp_host, double* bx_host);
int htn_cv_sweep(htn_mps* x, double z_re, double z_im, const htn_sweep_opts* opts, htn_bond_stats* stats_host, double* amp_host,
                 double* bx_host);

/* Excited states inside one sector: orthogonalised two-site DMRG.  After htn_mps_set_orthogonal(mps, others, n) every
 * OPTIMISING bond update of `mps` finds the lowest eigenpair of H_eff inside the orthogonal complement of the n attached
 * states: per attached state phi_k the overlap environments <mps|phi_k> of every bond are built at the call and moved with
 * the H environment by every update (non-optimising moves included); per update p_k = O_L theta_phi O_R is formed in the
 * state's theta layout (<p_k, theta> = <phi_k|psi>), the p_k are orthonormalised (a row whose remainder is below 1e-12 of
 * its norm is dropped) and the solve is htn_lanczos_orth_z's.  krylovdim + n <= 31, else the update fails.
 * The attached states must live in the same context and have the same symmetry, chain length and total sector (end
 * bonds of one sector, dimension 1); any centre position; they must not be updated while attached (attach again after
 * changing one).  References are counted: an attached state stays alive until it is detached.  n = 0 detaches; a state
 * without attached states takes exactly the code path it took before this call existed.  At most 8 states.  Not available
 * on a context with a communicator (htn_ctx_set_comm / htn_ctx_set_exchange with world > 1). */
int htn_mps_set_orthogonal(htn_mps* mps, const htn_mps* const* others_host, int32_t n);
/* -> number of attached states; dropped_host (may be NULL): projector rows dropped as dependent in the last update */
int32_t htn_mps_orthogonal_count(const htn_mps* mps, int32_t* dropped_host);
/* out_host[0..1] = <a|b> (re, im) by a transfer pass on the device; 0 for states in different total sectors */
int htn_mps_overlap(htn_mps* a, const htn_mps* b, double* out_host);

/* Two-point correlation functions of a finite chain, measured on the device without touching the state.  One call gives one
 * CHANNEL for all pairs i <= j: `open` acts on site i, `pass` on the sites strictly between (the Jordan-Wigner string of a
 * fermionic channel, else the identity), `close` on site j; `onsite` (has_onsite) is the one-site product for i == j.  The
 * operators are reduced site operators in the conventions of htn_site_op, exactly what an MPO channel of htn_mpo_create
 * carries: <close . pass ... pass . open> is what the Hamiltonian term with these three operators and coefficient 1 measures.
 * Method: a left pass carries the norm environment and forms, per site i, the environment with `open` (and `onsite`) applied
 * on i; a right pass carries the right norm environment plus one open level per closing site j (all levels of a site in the
 * two grouped-GEMM launches of one plan); on every bond the halves meet in ONE htn_block_trdots_z launch, block weight
 * (2S_bra + 1) / (2S_ket + 1) (1 in the abelian kind).  Nothing synchronises inside the pass; the table is downloaded once.
 * The norm environments are carried explicitly, so the centre may sit anywhere and the state is not re-gauged.
 * out_host: L*L complex128, row-major, entry [i*L + j] for i <= j (i == j only with has_onsite), everything else 0;
 * already divided by <psi|psi>, which is also returned in norm_host (may be NULL).  The state is not modified.
 * Errors: `open` and `close` charges that do not add up to zero, a `pass` (or `onsite`) operator that carries a charge, a
 * chain with boundary environments (an iDMRG window), a context with a communicator or an exchange hook (not verified). */
typedef struct {
    htn_site_op open, pass, close;  /* on site i, on the sites between, on site j  (i < j)               */
    htn_site_op onsite;             /* the one-site product for i == j; used only if has_onsite          */
    int32_t has_onsite, pad;
} htn_corr_channel;                 /* 552 bytes */
int htn_mps_correlator(htn_mps* mps, const htn_corr_channel* ch, void* out_host, double* norm_host);

/* Correlation functions of two nearest-neighbour BOND operators (four-point functions: bond order, bond pair field, dimer),
 * measured like htn_mps_correlator.  One call gives one channel for all i, j with j >= i + 2: open[0] acts on site i, open[1] on
 * site i + 1, `pass` on the sites i + 2 .. j - 1, close[0] on site j and close[1] on site j + 1 (n_close = 2; the bonds (i, i+1)
 * and (j, j+1) are disjoint).  The value is what an MPO path with these entries, coefficient 1 and the intermediate levels
 *   (open[0].dN, open[0].k) -> (open_dN, open_k) -> .. -> (-close[1].dN, close[1].k) -> scalar
 * measures (U1_U1: the k of a level is the sum of the operators' k to its left): open_dN / open_k name the level the open pair
 * couples to, in the SU(2) kinds one of the ranks |k0 - k1| .. k0 + k1; the level between the close operators is fixed by
 * close[1].  n_close = 1 is the variant with a one-site close: close[0] on site j takes the level (open_dN, open_k) to the
 * scalar, close[1] is ignored (it is neither read nor part of the plan-cache key; `pad` likewise) and j runs up to L - 1; it
 * measures products on three adjacent sites (j = i + 2) among others.
 * Method: the left probe carries the levels [norm, half, open] (norm -> half by open[0], half -> open by open[1]), the right
 * probe [norm, halfR, open_j ..] (halfR <- norm by close[1], open_j <- halfR by close[0], open_j <- open_j by `pass`); the
 * halves meet on bond i + 2 in ONE htn_block_trdots_z launch per bond with the block weight of htn_mps_correlator.  Nothing
 * synchronises inside the pass, the table is downloaded once, the state is only read (any gauge, any centre position).
 * out_host: L*L complex128, row-major, entry [i*L + j] for j >= i + 2 (j <= L - 2 with n_close = 2), everything else 0; already
 * divided by <psi|psi>, which is also returned in norm_host (may be NULL).
 * Errors: charges of the open pair and of the close operators that do not add up to zero; an (open_dN, open_k) the two open
 * operators cannot couple to; a `pass` that carries a charge; fewer than 4 sites (3 with n_close = 1); n_close outside 1..2; a
 * chain with boundary environments (an iDMRG window); a context with a communicator or an exchange hook. */
typedef struct {
    htn_site_op open[2];            /* on sites i, i + 1                                                  */
    htn_site_op close[2];           /* on sites j, j + 1 (n_close = 1: close[0] on site j alone)          */
    htn_site_op pass;               /* on sites i + 2 .. j - 1                                            */
    int32_t open_dN, open_k;        /* charge / rank of the level after open[1]: what the pair couples to */
    int32_t n_close, pad;
} htn_corr_channel2;                /* 696 bytes */
int htn_mps_correlator2(htn_mps* mps, const htn_corr_channel2* ch, void* out_host, double* norm_host);

/* A reduced site operator O (rank k, charge dN) applied to site `site` of a finite open chain: *out is a NEW state
 * O_site |src> in the total sector fused with (dN, k), on the same context and MPO; src is only read.  The operator's charge
 * leaves through the right end: bonds right of the site are re-labelled by fusion with (dN, k) (an old sector contributes its
 * multiplets to every new sector it couples to, in the sorted order of the old sectors; pairs nothing reaches are left out),
 * the site's tensor is opened with the reduced elements, the tensors right of it are passed through with 6j recoupling
 * coefficients; a fermionic operator carries its Jordan-Wigner string to the left, (-1)^(N_left dN).
 * The centre of src must be on `site`; the result has its centre there too, is canonical, and is NOT normalised:
 *   <O_x psi|O_y psi> = sum_q <psi| O+_{x,q} O_{y,q} |psi>   (sum over the components of the operator's multiplet)
 * in the units of htn_mps_overlap; norm2_host (may be NULL) receives <out|out>.  A result of norm 0 is returned as it is.
 * Host work: bond tables, layouts and one place-item list per site (cached by tables + operator); device work: one
 * htn_block_place_z launch per site from `site` on, copies left of it, the H environments of the new tables.
 * Errors: centre elsewhere; site out of range; SU(2) kinds: a source of total spin > 0 with an operator of rank > 0 (the result's
 * sector would not be unique); a chain with boundary environments; a context with a communicator or an exchange hook; a
 * state with attached orthogonal states; an operator that maps two site states onto one. */
int htn_mps_apply_op(const htn_mps* src, int32_t site, const htn_site_op* op, htn_mps** out, double* norm2_host);
/* out_host[x] = <O_x bra|ket> for all sites x (L complex128) in one pass: left of x the bra's own tensors (one left overlap
 * pass), right of x the passed tensors, which do not depend on x (one right overlap pass), per site one step with the opened
 * tensor and one htn_block_trdots_z launch: about 3L overlap steps instead of L^2.  bra may be in any gauge and is not
 * modified; nothing synchronises inside the pass.  Sites the sector tables admit no contribution for give exact zeros.
 * Errors: different contexts, lengths or symmetries; the total sector of ket is not that of bra fused with (dN, k); the
 * limits of htn_mps_apply_op (for the bra). */
int htn_mps_transition(htn_mps* bra, const htn_site_op* op, const htn_mps* ket, void* out_host);

/* Two-site energy variance of a finite open chain (Hubig, Haegeman, Schollwoeck, Phys. Rev. B 97, 045125): the squared norms of
 * (H - E)|psi> projected onto the one-site and the two-site tangent complements.  A sum of squared norms: no cancellation, no
 * <H^2> environments, no SVD of its own.  EXACT (= <H^2> - <H>^2 of the normalised state) for an MPO of range 1 (nearest-
 * neighbour terms only), a LOWER BOUND for longer range.  With the centre carried from site 0 to L-1, M_i the centre on site i,
 * A_i the left isometry of M_i, B_{i+1} the stored right-canonical tensor, theta = M_i B_{i+1} and y = H_eff2 theta:
 *   bond_host[i] = |(1 - A_i A_i^H) y (1 - B_{i+1}^H B_{i+1})|^2        i = 0 .. L-2
 *   site_host[i] = |(1 - A_i A_i^H) y B_{i+1}^H|^2                      i = 0 .. L-2   (the left-null part of H_eff1(M_i))
 *   site_host[L-1] = |H_eff1(M) - <M|H_eff1(M)> M|^2                    M the centre on the last site, formed by subtraction
 *   *energy_host = <theta|y>;   the variance is sum(site) + sum(bond).
 * In the tilde normalisation all of these are plain per-sector products and Frobenius norms.  Device work:
 * per bond one theta, one H_eff2 apply, one non-optimising move (htn_bond_update with optimise = 0, no dimension limit, no
 * cutoff: only singular values below 1e-14 of the largest go) that yields A_i, two htn_block_nullproj_z launches; one H_eff1 apply
 * and one launch on the last site; ONE download of the results.  The centre may be anywhere: it is carried to site 0 first by
 * the same moves.  No update writes into a buffer the state holds, so the state is kept by its handles and put back when the
 * call returns (errors included): tensors, environments, centre, stored energy, spectra and hints are bit for bit what they
 * were, and nothing is carried back.  Only the plan cache grows; the item lists are cached under keys of their own.
 * A state that carries its norm beside its tensors (htn_mps_apply_op) reports the variance of the NORMALISED state.
 * site_host: L doubles, bond_host: L-1 doubles, energy_host: one; each may be NULL.  split_host (may be NULL): three doubles, host
 * wall seconds of [theta + applies, projections, moves], every lap closed by a stream sync (a timed call is slower).
 * Refused: a chain with boundary environments (an iDMRG window), a context with a communicator or an exchange hook, a state
 * with attached orthogonal states, a state of norm 0. */
int htn_mps_variance(htn_mps* mps, double* site_host, double* bond_host, double* energy_host, double* split_host);

/* Perfect sampling of a finite open chain (Ferris, Vidal, Phys. Rev. B 85, 165146): n_samples independent configurations of
 * site multiplets, each drawn with its exact probability <psi|prod_i P_{s_i}|psi> / <psi|psi>, site by site from the left.
 * The centre must be on site 0 with every other site right-canonical (the state after every sweep); the state is only read.
 * Every sample carries a bond density matrix rho (one block per sector, trace 1); per site the batch takes one
 * Backend::sample_step (htn_sample_step_z above: the rule of the draw, the order of every sum).  In the tilde normalisation the
 * coefficient of every sub-block is 1 and a level closes against the right-canonical remainder with the identity, weight 1, in
 * every sector: probabilities are plain sums.
 *   u_host        n_samples x L uniforms in [0, 1), sample-major: u_host[b * L + i] draws site i of sample b
 *   measure_host  L flags (NULL: all 1); a site with flag 0 is traced: nothing is drawn there, its output is -1
 *   batch         samples that advance through a site together (<= 0: the default, 256); results do not depend on it
 *   out_host      n_samples x L multiplet indices (the site multiplets of the symmetry, in its order), -1 = traced
 *   logp_host     n_samples logarithms of the probability of the drawn configuration (of its measured sites)
 *   split_host    NULL or two doubles: host wall seconds of [planning, device passes including the downloads]
 * Nothing synchronises inside a pass: choices and log-probabilities are downloaded once per batch.  The per-site item lists are
 * cached under keys of their own (a sweep after the call plans what it plans without one).  A state that carries its norm
 * beside its tensors (htn_mps_apply_op) is sampled as the normalised state.
 * Refused: a centre that is not on site 0; a chain with boundary environments (an iDMRG window); a context with a communicator
 * or an exchange hook; a state with attached orthogonal states; a state of norm 0. */
int htn_mps_sample(htn_mps* mps, int32_t n_samples, const double* u_host, const int32_t* measure_host, int32_t batch,
                   int32_t* out_host, double* logp_host, double* split_host);

/* y = H_eff(bond i, i+1) x on host vectors in the library's theta layout (size htn_mps_theta_size); tests and
 * Hermiticity checks.  x and y are complex128 host arrays. */
int64_t htn_mps_theta_size(htn_mps* mps, int32_t i);
int htn_heff2_apply(htn_mps* mps, int32_t i, const void* x_host, void* y_host);
/* theta of sites (i, i+1) as currently stored (host, theta layout) */
int htn_mps_get_theta(htn_mps* mps, int32_t i, void* theta_host);

/* queries (two-call pattern: a NULL output pointer returns the count only) */
int32_t htn_mps_nsites(const htn_mps* mps);
int32_t htn_mps_bond(const htn_mps* mps, int32_t b, htn_sector* sectors_host);              /* -> number of sectors  */
int64_t htn_mps_spectrum(const htn_mps* mps, int32_t b, htn_sector* sectors_host, double* values_host);
                                        /* Schmidt values of the last update of bond b, per sector descending;
                                           sectors[k].count values each; returns the total number of values */
int64_t htn_mps_site_size(const htn_mps* mps, int32_t i, int32_t* kind_host);               /* kind: 'L' or 'R'      */
int32_t htn_mps_get_site(const htn_mps* mps, int32_t i, htn_subblock* subs_host, void* data_host);  /* -> #sub-blocks */
int64_t htn_mps_env_size(const htn_mps* mps, int32_t side, int32_t b);                      /* side 0 = left, 1 = right */
int htn_mps_get_env(const htn_mps* mps, int32_t side, int32_t b, void* data_host);
/* block table of an environment (htn_mps_env_blocks): one record per stored block */
typedef struct {
    int32_t aN, aj, w, bN, bj;     /* left env: (bra, w, ket) stored [n_bra x n_ket]; right env: (ket, w, bra) [n_ket x n_bra] */
    int32_t rows, cols;
    int32_t pad;
    int64_t off;
} htn_env_block;
int32_t htn_mps_env_blocks(const htn_mps* mps, int32_t side, int32_t b, htn_env_block* blocks_host);
/* the bond table an environment was built on.  It is the table of bond b AT THE TIME the environment was formed: the
 * left environment of bond b dates from the last rightward update of that bond, the right one from the last leftward
 * update, and a truncation by dimension may have kept different counts in between.  -> number of sectors */
int32_t htn_mps_env_bond(const htn_mps* mps, int32_t side, int32_t b, htn_sector* sectors_host);
/* planner introspection (tests): the task lists of the H_eff apply on bond i as the kernels receive them.
 * stage 0 = Z stage (may be empty), 1 = Y stage.  Returns counts through n_tiles / n_segs; tiles / segs may be NULL. */
int htn_plan_apply_dump(htn_mps* mps, int32_t i, int32_t stage, int32_t* n_tiles, htn_tile* tiles_host, int32_t* n_segs,
                        htn_seg* segs_host, int64_t* z_size, int64_t* flops);
/* the launch load-balancing pass the engine applies to every task list before upload (HIP backend): long tiles of 2 or 4
 * quadrants (16 x 16) are cut into one-quadrant tiles sharing their segment list, tiles still longer than a CU's fair
 * share into split-K parts (htn_tile.part / nparts / ws_slot / ticket); the records are then dealt in layers of n_cus,
 * longest to the least loaded CU, XCD-aware.  Returns the number of workspace slabs the balanced list needs (bufs[HTN_BUF_WS]
 * must then hold HTN_WS_ELEMS(slabs) elements with the ticket region zeroed), -1 on error; *n_out = number of records
 * (out may be NULL to query it). */
int32_t htn_balance_tiles(const htn_tile* tiles_host, int32_t n_tiles, int32_t n_cus, htn_tile* out_host, int32_t out_cap,
                          int32_t* n_out);
/* plan-cache statistics: hits, misses (host planner invocations) */
int htn_mps_cache_stats(const htn_mps* mps, int64_t* hits, int64_t* misses);

/* =====================================================================================================
 * Infinite chain: step-wise IDMRG2 driver (McCulloch's growing window, arXiv:0804.2509), what sits behind
 *     find_groundstate(psi0::InfiniteMPS, H, IDMRG2(; trscheme, tol))        src/HubbardFunctions.jl:1010
 * A window of 2T sites (window_mpo, full-width MPO bonds at both ends) is optimised by two-site sweeps between two
 * boundary environments; its halves are then absorbed into the boundaries (the environments at the centre bond; the
 * right one relabelled N -> N + window_dN) and the next window is predicted from the previous one's halves.  Boundary
 * environments and site tensors stay on the device from one step to the next.
 * The host supplies random windows (initialize_mps stays on the host side): a step whose previous step returned
 * needs_window = 1 (and the first step) must be given one, built between the tables htn_idmrg_boundary reports.
 * Handles are reference counted like htn_mps: the driver keeps its context and MPO alive; htn_idmrg_window hands out a
 * new reference to the current window (release it with htn_mps_destroy), valid after htn_idmrg_destroy.
 * ===================================================================================================== */
typedef struct htn_idmrg htn_idmrg;
typedef struct {
    htn_sweep_opts sweep;      /* truncation + solver of every window update                                          */
    int32_t cell_sites;        /* T: the window MPO holds 2T sites                                                    */
    int32_t window_dN;         /* particles per window, 2T P / Q (HTN_SYM_SU2: its parity)                            */
    double tol;                /* stop when the change of the centre spectrum delta < tol ...                         */
    int32_t min_steps;         /* ... after at least min_steps steps                                                  */
    int32_t maxiter;           /* or after maxiter steps                                                              */
    int32_t sweeps_per_step;   /* window sweeps per step (at most; early exit when the energy has settled)            */
    int32_t warm_start;        /* 1: McCulloch prediction from the third window on; 0: every window from the host     */
} htn_idmrg_opts;              /* 96 bytes */
typedef struct {
    int32_t step;              /* 0-based index of the step just run                                                  */
    int32_t sweeps;            /* window sweeps of this step                                                          */
    int32_t converged;         /* delta < tol after at least min_steps steps                                          */
    int32_t finished;          /* converged or maxiter reached: no further step (the window stays as its sweeps left it) */
    int32_t needs_window;      /* the next step must be given a window from the host                                  */
    int32_t chi_full;          /* TensorKit dim of the centre bond                                                    */
    double energy;             /* <psi|H|psi> of the grown system (all absorbed sites + the window)                   */
    double energy_per_site;    /* (energy - previous energy) / 2T; NaN on step 0                                      */
    double delta;              /* qdim-weighted distance of the centre spectra of this and the previous step; inf on step 0 */
} htn_idmrg_stats;             /* 48 bytes */
int htn_idmrg_create(htn_ctx* ctx, const htn_mpo* window_mpo, const htn_idmrg_opts* opts, htn_idmrg** out);
void htn_idmrg_destroy(htn_idmrg* idmrg);
/* bond table the next window must have at its left (side 0) / right (side 1) end; two-call pattern (NULL: count only).
 * -> number of sectors, -1 on a bad argument */
int32_t htn_idmrg_boundary(const htn_idmrg* idmrg, int32_t side, htn_sector* sectors_host);
/* one growth step.  Window tables as in htn_mps_create (bond_ptr ... data, 2T sites); all NULL = start from the driver's
 * prediction (allowed only when the previous step returned needs_window = 0).  stats_host may be NULL. */
int htn_idmrg_step(htn_idmrg* idmrg, const int32_t* bond_ptr_host, const htn_sector* sectors_host,
                   const int32_t* sub_ptr_host, const htn_subblock* subs_host, const int64_t* data_ptr_host,
                   const void* data_host, htn_idmrg_stats* stats_host);
/* the current window as an htn_mps (a new reference: release it with htn_mps_destroy) */
int htn_idmrg_window(htn_idmrg* idmrg, htn_mps** out);

#ifdef __cplusplus
}
#endif
#endif
