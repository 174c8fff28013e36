/* hifir_amd.h -- C ABI of the MI355X-native HIFIR preconditioner-apply path.
 *
 * Plain C, plain pointers and sizes, no C++/torch types.  This is the drop-in boundary for the
 * reference's hot path: the reference keeps factorizing on the host, hands each level of its
 * hif::Precs list to this library once (hifamd_add_level / hifamd_set_dense, the field set of
 * hif::Prec::export_sparse_data + inquire_or_export_dense), and from then on every
 * HIF::solve / HIF::hifir / lhf?Solve / lhf?Apply(LHF_S) call is served from HBM by hand-written
 * gfx950 kernels.  INTEGRATION.md shows the reference-side binding.
 *
 * All file:line citations are relative to the reference tree (HIFIR v0.2.0).
 *
 * Conventions
 *   - every function returns a HifAmdStatus (values mirror LhfStatus, libhifir/include/libhifir.h:148-154);
 *     the message of the last failure on the calling thread is returned by hifamd_last_error()
 *     (cf. lhfGetErrorMsg, libhifir.h:255).
 *   - value type: double (HIFAMD_D) or double complex (HIFAMD_Z, C99 layout == std::complex<double>);
 *     index type int32 (LhfInt), pointer type int64 (LhfIndPtr = ptrdiff_t), libhifir.h:47-83.
 *   - a handle is NOT thread-safe (same rule as the reference: HIF::solve mutates `mutable _prec_work`,
 *     src/hif/builder.hpp:579); distinct handles may be used from distinct threads.
 *   - multi-RHS blocks are row-interleaved [n][nrhs] with an explicit row stride (ld, in elements),
 *     i.e. the layout of hif::Array<std::array<T,Nrhs>> (src/hif/ds/CompressedStorage.hpp:2127).
 *   - there is no CPU fallback: without a usable HIP device every compute entry point fails with
 *     HIFAMD_HIFIR_ERROR.
 */
#ifndef HIFIR_AMD_H
#define HIFIR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum HifAmdStatus {
  HIFAMD_SUCCESS = 0,      /* LHF_SUCCESS */
  HIFAMD_NULL_OBJ,         /* LHF_NULL_OBJ */
  HIFAMD_MISMATCHED_SIZES, /* LHF_MISMATCHED_SIZES */
  HIFAMD_BAD_PREC,         /* LHF_BAD_PREC */
  HIFAMD_HIFIR_ERROR       /* LHF_HIFIR_ERROR */
} HifAmdStatus;

typedef enum HifAmdValueType { HIFAMD_D = 0, HIFAMD_Z = 1 } HifAmdValueType;

/* operator tags of lhf?Apply (LhfOperationType, libhifir/include/libhifir.h:159-164), same values */
typedef enum HifAmdOp {
  HIFAMD_S = 0, /* x = M^{-1} b   (prec_solve,      alg/prec_solve.hpp:332-412) */
  HIFAMD_SH,    /* x = M^{-H} b   (prec_solve_tran, alg/prec_solve.hpp:542-612) */
  HIFAMD_M,     /* x = M b        (prec_prod,       alg/prec_prod.hpp:55-147)  */
  HIFAMD_MH     /* x = M^H b      (prec_prod_tran,  alg/prec_prod.hpp:148-235) */
} HifAmdOp;

typedef struct HifAmdPrec *HifAmdHdl; /* opaque: one multilevel preconditioner resident in HBM */

/* ---- library ------------------------------------------------------------------------------ */
const char *hifamd_version(void);
/* message of the last error on this thread, or NULL; cleared by the call (libhifir.cpp:224-229) */
const char *hifamd_last_error(void);
/* number of visible HIP devices (0 without a GPU; never fails) */
int hifamd_device_count(void);

/* ---- lifecycle ---------------------------------------------------------------------------- */
/* replaces `new HIF<>` in lhf?Create (libhifir.cpp:383-396); device = HIP ordinal, -1 = current */
HifAmdStatus hifamd_create(HifAmdValueType vt, int device, HifAmdHdl *out);
HifAmdStatus hifamd_destroy(HifAmdHdl h); /* NULL-safe, frees HBM (cf. lhf?Destroy, libhifir.h:619) */

/* ---- hierarchy import (host pointers; data is copied) ------------------------------------- */
/* One call per hif::Prec, in list order (src/hif/alg/Prec.hpp:309-323).  The four matrices are
 * CCS exactly as the reference stores them (Prec::mat_type = ccs_type, Prec.hpp:86,90):
 *   L_B, U_B : m x m strict triangles, implicit unit diagonal, sorted row indices
 *   E        : (n-m) x m,   F : m x F_ncols (F_ncols == n-m, or 0 when absent; prec_solve.hpp:395)
 * d: m values; s,t: n REAL scalings (Prec.hpp:96-99); p, q_inv: n 0-based permutations.
 * p_inv and q are only needed by HIFAMD_SH / HIFAMD_M / HIFAMD_MH and may be NULL otherwise (with q the plain solve
 * also writes its output permutation from inside the last triangular kernel instead of a separate pass). */
HifAmdStatus hifamd_add_level(HifAmdHdl h, int64_t m, int64_t n,
                              const int64_t *L_colptr, const int32_t *L_rowind, const void *L_vals,
                              const int64_t *U_colptr, const int32_t *U_rowind, const void *U_vals,
                              const int64_t *E_colptr, const int32_t *E_rowind, const void *E_vals,
                              int64_t F_ncols,
                              const int64_t *F_colptr, const int32_t *F_rowind, const void *F_vals,
                              const void *d, const double *s, const double *t,
                              const int32_t *p, const int32_t *p_inv,
                              const int32_t *q, const int32_t *q_inv);
/* The UNFACTORED column-major nd x nd Schur complement of the last level, as
 * Prec::inquire_or_export_dense hands it out (Prec.hpp:275-293).  Factorized here on the host by
 * QR with column pivoting + rank determination (QRCP::factorize, small_scale/QRCP.hpp:107-179);
 * rrqr_cond <= 0 selects the reference default eps^(-2/3) (QRCP.hpp:110-117). */
HifAmdStatus hifamd_set_dense(HifAmdHdl h, int64_t nd, const void *mat_colmajor, double rrqr_cond);
/* The same block of a hierarchy that the reference factorized with is_symm (symm_level_factorize,
 * alg/symm_factor.hpp:654-657 fills Prec::symm_dense_solver instead of dense_solver; the export is the
 * symmetric branch of Prec::inquire_or_export_dense, Prec.hpp:294-303).  Factorized here on the host by a
 * symmetric / Hermitian eigendecomposition with the truncation rules of SYEIG::factorize
 * (small_scale/SYEIG.hpp:107-175): spd > 0 positive definite, < 0 negative definite, 0 indefinite
 * (Options::spd).  Only the lower triangle is read.  Solve, conjugate-transpose solve and product follow
 * SYEIG::solve / multiply (SYEIG.hpp:181-200, 256-273), incl. the run-time `rank` argument. */
HifAmdStatus hifamd_set_dense_symm(HifAmdHdl h, int64_t nd, const void *mat_colmajor, int spd);
/* The same block when the reference was built with HIF_DENSE_MODE=0 (macros.hpp:100-105, small_scale/solver.hpp:49):
 * its last level is then LU with partial pivoting (small_scale/LUP.hpp).  Factorized here on the host
 * (?getrf semantics, LUP::factorize :100-119) and applied as one product with the explicit inverse; the `rank`
 * argument is ignored as in LUP::solve (:141), the conjugate-transpose apply passes 'T' to the solve and 'C' to the
 * product exactly like LUP.hpp:150,187.  An exactly singular block is refused (HIFAMD_BAD_PREC). */
HifAmdStatus hifamd_set_dense_lup(HifAmdHdl h, int64_t nd, const void *mat_colmajor);
/* Converts CCS -> schedule-ordered CSR, level-schedules the triangular factors, ships everything to
 * HBM and sizes the work arena for batches of up to max_nrhs (the reference sizes its work buffer
 * on first use only, builder.hpp:414-416 -- not replicated). */
HifAmdStatus hifamd_finalize(HifAmdHdl h, int64_t max_nrhs);
/* Complex handles only, and only before the first hifamd_add_level (the flags are planner options: they shape the
 * analysis of every level).  Real handles form two explicit operators at hifamd_finalize that complex handles do not
 * have by default: the closed top of every L / U triangle pair as one dense product, and the tail of the hierarchy (from
 * the first level of at most 4,096 rows through the dense block) as one dense product, guarded by the finalize-time
 * probe of hifamd_stats_ext slots 7-11.  The flags ask for them on this handle; their products run on the f64 matrix
 * cores as two real products per complex one.  Opt-in because the kernel families a default complex handle launches
 * are pinned by the test suite; a handle created without this call plans, launches and answers as before.
 * Refusals, in this order: NULL handle HIFAMD_NULL_OBJ; flags outside 0 ... 3 HIFAMD_MISMATCHED_SIZES; a real handle
 * with flags != 0 HIFAMD_BAD_PREC (it has both operators already); a handle that has a level or is finalized
 * HIFAMD_BAD_PREC.  Flags 0 is a no-op.  hifamd_save(_ex) does not store the flags: pass them to hifamd_load_ex. */
#define HIFAMD_ZOP_TAIL 1 /* tail of the hierarchy as one operator */
#define HIFAMD_ZOP_TOP 2  /* closed top of every triangle pair as one operator */
HifAmdStatus hifamd_set_complex_operators(HifAmdHdl h, int flags);

/* ---- on-disk form of an imported hierarchy ---------------------------------- */
/* hifamd_save writes exactly what hifamd_add_level / hifamd_set_dense received (before or after
 * hifamd_finalize); hifamd_load creates a handle and replays those calls -- the caller then calls
 * hifamd_finalize.  Lets a hierarchy factorized once on a host that has the reference be applied on
 * GPU nodes that do not.  Format (little-endian): "HIFAMD1\0", int64 value type, int64 #levels, int64
 * has_dense; per level int64 {m, n, F_ncols}, the four CCS matrices as int64 {nrows, ncols} + three
 * counted arrays (int64 count, data, zero padding to 8 bytes), then d, s, t, p, p_inv, q, q_inv as
 * counted arrays; the dense block as int64 nd, double rrqr_cond and a counted column-major array. */
HifAmdStatus hifamd_save(HifAmdHdl h, const char *path);
HifAmdStatus hifamd_load(const char *path, int device, HifAmdHdl *out);
/* hifamd_load with hifamd_set_complex_operators(h, complex_operators) applied between the creation of the handle and
 * the replayed hifamd_add_level calls; hifamd_load is this call with 0.  An analysis trailer written under other flags
 * does not fit the planner options in force and is ignored: the levels are analyzed afresh. */
HifAmdStatus hifamd_load_ex(const char *path, int device, int complex_operators, HifAmdHdl *out);
/* hifamd_save with options.  HIFAMD_SAVE_ANALYSIS appends the ANALYSIS of every level (wavefront schedules, band plans,
 * slot-ordered triangles: what hifamd_add_level derives on the host, e.g. 24 s of the 45 s between load and first apply
 * on a 256^3 grid) as a checksummed trailer behind the records above.  hifamd_load adopts it when it was made with the
 * planner options in force (HIFIR_AMD_* environment) and fits the factors' sparsity pattern (it holds no matrix values),
 * verifies every size and index range first, and analyzes as usual otherwise (also with HIFIR_AMD_LOAD_ANALYSIS=0): a trailer changes how long a load
 * takes, never its result -- hifamd_stats_ext slot 12 tells how many levels came from it.  A reader that does not know
 * the trailer ignores it.  No reference counterpart. */
#define HIFAMD_SAVE_ANALYSIS 1
HifAmdStatus hifamd_save_ex(HifAmdHdl h, const char *path, int flags);

/* ---- queries (cf. lhf?GetLevels/GetNnz/GetSchurSize/GetSchurRank, libhifir.h:722-740) ------ */
int hifamd_value_type(HifAmdHdl h);     /* HIFAMD_D / HIFAMD_Z of the handle (what hifamd_load found in the file); -1 for NULL */
int hifamd_device(HifAmdHdl h);         /* HIP ordinal the handle is bound to (after hifamd_finalize; before: as created, -1 = current) */
int64_t hifamd_nrows(HifAmdHdl h);
int64_t hifamd_levels(HifAmdHdl h);     /* counts the dense block as a level (builder.hpp:141-147) */
int64_t hifamd_nnz(HifAmdHdl h);        /* Prec::nnz summed (Prec.hpp:170-176) */
int64_t hifamd_schur_size(HifAmdHdl h);
int64_t hifamd_schur_rank(HifAmdHdl h);
/* stats[0..15]: 0 sum n_l, 1 sum m_l, 2 nnz(L)+nnz(U), 3 nnz(E)+nnz(F), 4 dense n, 5 B_mat bytes,
 * 6 B_vec bytes per RHS (SURVEY 8d formula), 7 #wavefronts L (all levels), 8 #wavefronts U,
 * 9 kernel launches per apply at the last captured batch width, 10 sparse levels, 11 bands (L+U, all
 * levels), 12 band workgroups, 13 seconds spent in hifamd_finalize, 14 bytes of explicit operators resident in HBM
 * (block inverses + combined top operators + the tail operator), 15 milliseconds of the last hipGraph capture */
HifAmdStatus hifamd_stats(HifAmdHdl h, double *stats16);
/* Set-up and operator accounting (additive, no reference counterpart); returns the number of values it knows, writes
 * min(cap, that) of them: 0 finalize seconds, 1 last graph capture ms, 2 bytes of block inverses, 3 bytes of combined top
 * operators, 4 bytes of the tail operator, 5 rows of the tail operator (0: the recursion runs), 6 its first level,
 * 7 relative difference product vs recursion on the finalize-time probe, 8 max |entry| of the tail operator, 9 why it
 * was rejected (0 not, 1 not finite, 2 growth, 3 probe, 4 an error while it was formed), 10 / 11 the probe and growth
 * limits in force (HIFIR_AMD_TAIL_PROBE_TOL, HIFIR_AMD_TAIL_GROWTH), 12 levels whose analysis came from the trailer of the
 * file the handle was loaded from (hifamd_save_ex), 13 host seconds spent analyzing the levels (or adopting their
 * analysis), 14 bytes of the work arena (w + v of every level), 15 its width in columns (this build: always 64 -- the
 * fast kernels address a 64-column arena; max_nrhs bounds the batch width a call may pass, not the arena), 16 bytes of
 * the component bands' coefficient tiles, 17 bytes of the factors with their plan arrays, 18 max_nrhs of hifamd_finalize,
 * 19 / 20 rows (all levels) whose L / U result the FIRST solve of a level does not store because nothing reads it from
 * memory (real handles, sparse-own levels; HIFIR_AMD_SKIP_ROWS=0: none), 21 arrays of the host copy that hifamd_finalize found
 * changed since hifamd_add_level -- not by this library -- and rebuilt from the imported arrays (a warning names them on stderr;
 * anything it cannot rebuild is refused), 22 bytes of the null-space bases resident in HBM (hifamd_set_nsp_basis, both ops),
 * 23 / 24 rows of sparse-own L bands that are streamed as sources / kept in LDS as dependent rows (kernel k_band_ls), 25 rows
 * of that kernel's source chunk (0: no band runs through it),
 * 26 components of all component bands (L and U, every level), 27 workgroups of those bands that own more than one
 * component (the planner chains components once a band has more than 8 * HIFIR_AMD_BAND_WGS of them, and bags small
 * ones), 28 the largest number of source chunks per component of any band that runs through k_band_ls, 29 the flags of
 * hifamd_set_complex_operators in force (real handles: 0).  Slots 3-11 are filled for complex handles as for real ones.
 * -1 for a NULL handle. */
int hifamd_stats_ext(HifAmdHdl h, double *out, int cap);
/* Per-level sizes (what the SURVEY 8(d) byte formula needs level by level): 0 m, 1 n, 2 nnz(L_B), 3 nnz(U_B), 4 nnz(E),
 * 5 nnz(F), 6 / 7 wavefronts of L / U, 8 / 9 launches ("bands") of the L / U plan, 10 rows of the combined top operator.
 * Returns the number of values it knows (-1: NULL handle or no such level). */
int hifamd_level_stats(HifAmdHdl h, int level, double *out, int cap);
/* Which level and stage every kernel launch of the LAST batched apply belongs to, in launch order (for attributing a
 * kernel trace): out[i] = 16 * level + stage, stage 1 S1 gather, 2 first LDU solve (with the fused S1), 3 S3 product with
 * E, 4 dense block / tail operator, 5 S5 product with F, 6 second LDU solve (with the fused S5 / S7), 7 S7 scatter
 * (prec_solve.hpp:359-411).  Returns the number of launches; writes min(cap, that). */
int hifamd_launch_map(HifAmdHdl h, int32_t *out, int cap);
/* Which kernels the LAST batched apply launched, by kernel family (for tests: does a shape or a setting reach the kernel it
 * is meant to reach?).  Host-side bookkeeping at the launch sites, kept with the graph of the shape like the launch map and
 * summed over the lanes of a batch wider than 64 columns; of the forward or the adjoint apply, whichever ran last.
 * out[f] = launches of family f on every level, out[N + f] = those of them on a level >= 1 (the tail operator counts for
 * the first level it replaces), f < N; hifamd_kernel_family_name(f) names the families in order ("band_ct1", "band_ct2",
 * ..., NULL from f = N on).  A family is what the dispatch distinguishes: a kernel, and where the planner or a
 * HIFIR_AMD_* switch chooses between instantiations, the instantiation (two exceptions: bit 2048 of HIFIR_AMD_CD_DBG picks the
 * other form of k_band_ct's tile loop, which makes the same sums in the same order -- both count as band_ct1 / 2 / 4; bit
 * 4096 picks the former group loop and epilogue of k_spmm_tile / k_spmm_tile4 -- both count as spmm_tile[4]_rb1 / 2).
 * Returns 2 N (writes min(cap, that)); 0 before
 * hifamd_finalize, -1 for a NULL handle. */
int hifamd_kernel_census(HifAmdHdl h, int32_t *out, int cap);
const char *hifamd_kernel_family_name(int family);
/* level schedule of one triangular factor (host-side analysis; usable without a GPU):
 * which = 0 (L_B) / 1 (U_B).  *nwf = number of wavefronts; if order != NULL it receives the m row
 * ids in processing order and wf_ptr (nwf+1 entries) the wavefront boundaries into it. */
HifAmdStatus hifamd_level_schedule(HifAmdHdl h, int level, int which, int64_t *nwf,
                                   int32_t *order, int64_t *wf_ptr);

/* ---- apply: x = M^{-1} b ------------------------------------------------------------------ */
/* rank: 0 = numerical rank of the dense level, <0 or > size = full (QRCP.hpp:376-377) */
/* HIF::solve (builder.hpp:409-423) / lhf?Solve (libhifir.h:698): host pointers, one RHS */
HifAmdStatus hifamd_solve(HifAmdHdl h, const void *b, void *x, int64_t rank);
/* batched, HOST pointers: B, X are [n][nrhs] row-interleaved with row strides ldb, ldx */
HifAmdStatus hifamd_solve_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx,
                                int64_t nrhs, int64_t rank);
/* batched, DEVICE pointers on the handle's device; enqueued on `stream` (a hipStream_t, NULL = the
 * handle's own stream) and NOT synchronized.  B and X must not alias (libhifir Ownership note). */
HifAmdStatus hifamd_solve_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx,
                                    int64_t nrhs, int64_t rank, void *stream);

/* ---- outer matrix, SpMV and iterative refinement ------------------------------------------ */
/* user matrix A in CRS (copied to HBM): what lhf?Setup borrows for IR (libhifir.cpp:413);
 * 0- or 1-based like the reference (builder.hpp:311-329) */
HifAmdStatus hifamd_set_matrix(HifAmdHdl h, int64_t n, const int64_t *indptr, const int32_t *indices,
                               const void *vals);
/* Y = A X, row dot-products in CRS order (CRS::multiply_nt_low, CompressedStorage.hpp:1109-1127;
 * mt::multiply_nt, utils/mt_mv.hpp:58-73); device pointers, [n][nrhs] */
HifAmdStatus hifamd_spmv_batch_dev(HifAmdHdl h, const void *dX, int64_t ldx, void *dY, int64_t ldy,
                                   int64_t nrhs, void *stream);
/* HIF::hifir (builder.hpp:459-489, alg/IterRefine.hpp:77-165) for nrhs columns at once; host
 * pointers.  betas == NULL: fixed nirs sweeps.  betas = {lower, upper}: per-column relative
 * residual test; ir_status (2*nrhs ints, may be NULL) gets {iterations, flag} per column with
 * flag 0 converged / 1 diverged / -1 reached nirs (IterRefine.hpp:119-120). */
HifAmdStatus hifamd_hifir_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx,
                                int64_t nrhs, int nirs, const double *betas, int64_t rank,
                                int *ir_status);
/* same with device pointers for B and X (ir_status stays a host array) */
HifAmdStatus hifamd_hifir_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx,
                                    int64_t nrhs, int nirs, const double *betas, int64_t rank,
                                    int *ir_status);

/* ---- null-space filter (HIF::nsp / HIF::nsp_tran, builder.hpp:419-422, 491-492) --------------- */
/* Constant mode (NspFilter::set_nsp_const, NspFilter.hpp:118-125): after every HIFAMD_S (op = HIFAMD_S)
 * or HIFAMD_SH (op = HIFAMD_SH) apply -- inside iterative refinement and GMRES too -- each column loses
 * the mean of its rows [start, end); end < 0 means "to the last row"; start > end >= 0 removes the
 * filter.  Unlike the reference (builder.hpp:439) batched applies are filtered as well.  Needs a
 * finalized handle. */
HifAmdStatus hifamd_set_nsp_const(HifAmdHdl h, HifAmdOp op, int64_t start, int64_t end);
/* Basis mode (the device form of the reference's user filter, NspFilter.hpp USER_OR / USER_CB: a host callback cannot
 * run inside a device-resident Krylov loop, so the caller hands over vectors that span the null space): after every
 * HIFAMD_S (op = HIFAMD_S) or HIFAMD_SH (op = HIFAMD_SH) apply -- inside iterative refinement, GMRES / FGMRES and
 * BiCGSTAB too -- every column x becomes x - Q (Q^H x), Q an orthonormal basis of span(V).  V: host pointer, [n][k]
 * row-interleaved with row stride ldv (the multi-RHS layout), 1 <= k <= HIFAMD_NSP_MAX, of the handle's value type;
 * copied, orthonormalized on the host (modified Gram-Schmidt in the caller's order, twice, Hermitian inner products)
 * and shipped to HBM.  k = 0 (V may be NULL) removes the basis.  One filter per op: setting a basis replaces a
 * constant-mode filter on that op, and switching a constant-mode filter on replaces a basis.  Needs a finalized handle.
 * Refusals, in this order: NULL handle HIFAMD_NULL_OBJ; op not HIFAMD_S / HIFAMD_SH, k < 0, k > HIFAMD_NSP_MAX, k > 0
 * with V NULL or ldv < k HIFAMD_MISMATCHED_SIZES; handle not finalized HIFAMD_BAD_PREC; a non-finite entry, a zero
 * vector or a vector that depends numerically on its predecessors (norm after orthogonalization <= eps^(2/3) of the
 * norm before, the rank criterion of the dense level, QRCP.hpp:110-117) HIFAMD_BAD_PREC, the message naming the
 * vector's index.  A column's filtered bits do not depend on the batch it travels in.
 * Krylov drivers: GMRES / FGMRES and BiCGSTAB keep their semantics, the filter acts on their applies only -- a caller
 * who wants a consistent right-hand side calls hifamd_nsp_filter_batch on it first.  PCG and symmetric QMR with a basis
 * on HIFAMD_S run projected (see hifamd_pcg_batch, hifamd_sqmr_batch). */
#define HIFAMD_NSP_MAX 16
HifAmdStatus hifamd_set_nsp_basis(HifAmdHdl h, HifAmdOp op, int64_t k, const void *V, int64_t ldv);
/* vectors of the basis filter in force on op (0: none or constant mode; -1: NULL handle) */
int64_t hifamd_nsp_dim(HifAmdHdl h, HifAmdOp op);
/* The filter in force on op (basis or constant mode) alone, in place, on [n][nrhs] blocks (what a caller uses to make b
 * consistent or to project a start vector).  No filter set: the block is left as it is.  Host pointers (returns when
 * done) / device pointers, enqueued on `stream` (NULL = the handle's own) and not synchronized, like
 * hifamd_apply_batch_dev. */
HifAmdStatus hifamd_nsp_filter_batch(HifAmdHdl h, HifAmdOp op, void *X, int64_t ldx, int64_t nrhs);
HifAmdStatus hifamd_nsp_filter_batch_dev(HifAmdHdl h, HifAmdOp op, void *dX, int64_t ldx, int64_t nrhs, void *stream);
/* FIND the null space of a singular system on the device, for the caller who knows THAT A is singular, not what its
 * null space is.  op = HIFAMD_S: null(A); op = HIFAMD_SH: null(A^H) (runs on the adjoint engine, built on first use).
 * Method: for a block X0 of always HIFAMD_NSP_MAX = 16 probe columns (a 16-column batch costs what one column costs,
 * and the spare columns tell "nullity = kmax" from "more than kmax"), B = -A X0 lies in range(A), so A D = B is
 * consistent; D = hifamd_gmres_batch_dev on the 16 columns (x0 = 0, restart, rtol, maxit, rank as there); V = X0 + D
 * has ||A v_j|| <= rtol ||A x0_j|| and numerical rank = nullity.  V is ordered and orthonormalized through 16 x 16
 * matrices: G = V^H V (fixed-order device reduction), Hermitian eigendecomposition on the host, eigenvalues descending,
 * V <- V E diag(w)^{-1/2}; then twice the order-preserving step G = V^H V = R^H R (Cholesky), V <- V R^{-1}.  A column
 * whose eigenvalue or Cholesky pivot is not positive and finite is dropped with every column behind it (not an error: a
 * nonsingular A with a near-exact M gives V ~ 0).  Accepted by the definition, not by the spectrum: q_j is a numerical
 * null vector when res_j = ||A q_j||_2 <= tol ||A||_inf (||A||_inf the largest row sum of |a_ij|, of A^H for
 * HIFAMD_SH); *found = length of the LEADING PREFIX of accepted columns, at most kmax.
 * How rtol and tol relate: for a random probe ||v|| ~ ||x0|| sqrt(k / n) (k the nullity), so the null columns reach
 * res / ||A|| <~ rtol sqrt(n / k), while every unit column orthogonal to the null space has res >= sigma_min+(A), the
 * smallest nonzero singular value: tol has to lie between the two (e.g. rtol = 1e-10, tol = 1e-7 up to 1M rows).  A
 * matrix with sigma_min+ < tol ||A||_inf has, by this definition, a larger numerical null space.
 * X0 != NULL: host [n][16] probes of the handle's value type, row stride ldx0 >= 16.  X0 == NULL: generated on the
 * device from `seed` by a counter-based generator: entry (i, j) is f(16 i + j + 1), the imaginary part of a complex
 * entry f(16 (n + i) + j + 1), where f(c): z = seed + 0x9E3779B97F4A7C15 c (mod 2^64); z = (z ^ (z >> 30))
 * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) 0x94D049BB133111EB; z = z ^ (z >> 31) (the splitmix64 finalizer);
 * u = (z >> 11) 2^-53; f = 2 u - 1.
 * The filter in force on op (basis or constant) is suspended for the duration of the search and restored on every
 * exit, error exits included.  install != 0 and *found > 0: the first *found columns become the basis filter of op
 * (as hifamd_set_nsp_basis would set them, without a host round trip; a constant-mode filter on op is replaced);
 * *found == 0 leaves the filter in force as it was.  Q (host, may be NULL, row stride ldq >= kmax) receives the
 * *found columns [n][*found]; resid16 (may be NULL) the 16 values res_j / ||A||_inf in column order, +infinity for a
 * dropped column; info4 (may be NULL) = {probe columns whose GMRES did not converge, largest GMRES iteration count,
 * 1 if a column beyond kmax also passed or *found == 16 ("there may be more"), 1 if anything non-finite was met (then
 * *found = 0)}.  Same inputs, same bits.  Needs hifamd_set_matrix; the 16-column batch passes the
 * width check of hifamd_gmres_batch.
 * Refusals, in this order: NULL handle HIFAMD_NULL_OBJ; op not HIFAMD_S / HIFAMD_SH, kmax < 1, kmax > 16, tol <= 0,
 * rtol <= 0, restart < 1, maxit < 1, X0 given with ldx0 < 16, Q given with ldq < kmax, found NULL
 * HIFAMD_MISMATCHED_SIZES; handle not finalized or no matrix HIFAMD_BAD_PREC. */
HifAmdStatus hifamd_nsp_find(HifAmdHdl h, HifAmdOp op, int64_t kmax, double tol, double rtol, int restart, int maxit,
                             int64_t rank, const void *X0, int64_t ldx0, uint64_t seed, int install, int64_t *found, void *Q,
                             int64_t ldq, double *resid16, int *info4);
/* the orthonormal basis in force on op, [n][k] into Q (host, row stride ldq >= k); returns k, 0 when there is none or
 * the filter is in constant mode, -1 for a NULL handle, a NULL Q or ldq too small */
int64_t hifamd_nsp_get_basis(HifAmdHdl h, HifAmdOp op, void *Q, int64_t ldq);

/* ---- lhf?Apply with an operator tag (libhifir.h:685, libhifir.cpp:447-472), batched ----------- */
/* op = HIFAMD_S / HIFAMD_SH: nirs <= 1 direct apply (ir_status, if given, gets {1, -1} per column);
 * nirs > 1: iterative refinement with A (HIFAMD_S) or A^H (HIFAMD_SH, IterRefine.hpp:93-96).
 * op = HIFAMD_M / HIFAMD_MH: the multilevel product (HIF::mmultiply, builder.hpp:503-513), always direct.
 * rank = -2 (LHF_DEFAULT_RANK) -> full rank for products and when refining, numerical rank otherwise
 * (libhifir.cpp:453-455).
 * The adjoint hierarchy (U^H, L^H, F^H, E^H, conj(d), (t,q) in, (s,p_inv) out, A^H solve on the dense
 * block) is analysed and shipped to HBM on the first HIFAMD_SH call; it needs the q and p_inv arrays
 * in hifamd_add_level (so do the product operators).  Host pointers. */
HifAmdStatus hifamd_apply_batch(HifAmdHdl h, HifAmdOp op, const void *B, int64_t ldb, void *X, int64_t ldx,
                                int64_t nrhs, int nirs, const double *betas, int64_t rank, int *ir_status);
/* direct apply with device pointers, enqueued on `stream` and not synchronized */
HifAmdStatus hifamd_apply_batch_dev(HifAmdHdl h, HifAmdOp op, const void *dB, int64_t ldb, void *dX, int64_t ldx,
                                    int64_t nrhs, int64_t rank, void *stream);

/* ---- right-preconditioned restarted GMRES, batched (the caller of the hot path) ------------- */
/* The reference's driver gmres_hif (examples/advanced/gmres.hpp:19-123: x0 = 0, modified Gram-Schmidt,
 * Givens rotations, stop on |y_{j+1}| / ||b|| <= rtol) for nrhs columns in lock step; all vectors
 * stay in HBM -- and so do the Hessenberg columns, rotations, residuals and per-column iteration state;
 * one batched apply, one SpMM and j + 2 fused axpy/dot passes per inner step serve every column, and the host
 * reads back three integers per step.  Needs hifamd_set_matrix.  Real and complex handles: the Hessenberg
 * entries are Hermitian products sum conj(q_i) v_i (for real data that IS the example's hif::inner; for
 * complex data the example's sum conj(v_i) q_i is the conjugate and would not orthogonalize), the rotations
 * follow gmres.hpp:75-83 with their conjugates.  rank: 0 numerical rank (the example's default),
 * -1 full.  Per column: flags[c] = 0 converged / 1 stagnated / 2 reached maxit, iters[c] = inner
 * iterations (either may be NULL).  Host pointers; the _dev variant takes device pointers for B, X. */
HifAmdStatus hifamd_gmres_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs,
                                int restart, double rtol, int maxit, int64_t rank, int *flags, int *iters);
HifAmdStatus hifamd_gmres_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs,
                                    int restart, double rtol, int maxit, int64_t rank, int *flags, int *iters);

/* The flexible variant fgmres_hifir (examples/advanced/gmres.hpp:127-231): the preconditioner of outer cycle
 * k is iterative refinement with 2^k sweeps (HIF::hifir), the preconditioned basis is kept and x is updated
 * from it.  sweeps[c] (may be NULL) = refinement sweeps spent on column c (the driver's num_mv). */
HifAmdStatus hifamd_fgmres_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs,
                                 int restart, double rtol, int maxit, int64_t rank, int *flags, int *iters,
                                 int *sweeps);

/* ---- extra-precise residuals: compensated b - A x, refinement and GMRES-IR -------------------- */
/* How the handle's drivers form r = b - A x.  HIFAMD_RESID_WORKING (the default): tmp = 0; tmp += a x; r = b - tmp in
 * working precision, rounding error about eps sum |a||x| per row.  HIFAMD_RESID_COMPENSATED: every row's sum is carried
 * as an unevaluated pair, as if in twice the working precision (TwoProd by fused multiply-add, TwoSum; Dot2 of Ogita,
 * Rump and Oishi with b_i as the first term), error eps |r| + gamma^2 (|b| + sum |a||x|): what lets refinement reach a
 * forward error of eps instead of cond(A) eps.  x, the applies and the Krylov kernels stay in working precision.  The
 * operations per row and column, in CRS order:
 *   s = b_i; c = 0; per nonzero: p = (-a) x; e = fma(-a, x, -p); t = s + p; z = t - s; q = (s - (t - z)) + (p - z);
 *   s = t; c = c + (q + e); finally r_i = s + c.
 * Complex: two independent real sums started from Re b and Im b; per nonzero the real part takes (-ar xr) then (+ai xi),
 * the imaginary part (-ar xi) then (-ai xr).  A column's bits depend neither on the batch width nor on its neighbours.
 * The mode is followed by both branches of hifamd_hifir_batch and hifamd_apply_batch (HIFAMD_S and HIFAMD_SH: the
 * adjoint engine holds A^H as a CRS of its own), by the restart residuals of GMRES / FGMRES and by FGMRES's inner
 * refinement; the null-space search always works in working precision.  The default is read from HIFIR_AMD_RESIDUAL
 * (0 / 1) when the handle is created.  Finalized or not; a mode outside 0..1: HIFAMD_MISMATCHED_SIZES. */
#define HIFAMD_RESID_WORKING 0
#define HIFAMD_RESID_COMPENSATED 1
HifAmdStatus hifamd_set_residual_precision(HifAmdHdl h, int mode);
/* the mode in force; -1 for a NULL handle */
int hifamd_residual_precision(HifAmdHdl h);
/* R = B - A X (op = HIFAMD_S) or B - A^H X (op = HIFAMD_SH, the adjoint engine, built on first use as for
 * hifamd_apply_batch) on [n][nrhs] blocks with row strides ldb, ldx, ldr; mode HIFAMD_RESID_WORKING /
 * HIFAMD_RESID_COMPENSATED, or -1 for the handle's.  Needs hifamd_set_matrix; any width (64 columns per launch).
 * Refusals, in this order: NULL handle HIFAMD_NULL_OBJ; another op, a mode outside -1..1 HIFAMD_MISMATCHED_SIZES; handle
 * not finalized or no matrix HIFAMD_BAD_PREC; a NULL block HIFAMD_NULL_OBJ; nrhs < 1 or a row stride below nrhs
 * HIFAMD_MISMATCHED_SIZES; R aliasing B or X HIFAMD_BAD_PREC.  Host pointers (returns when done) / device pointers,
 * enqueued on `stream` (NULL = the handle's own) and not synchronized. */
HifAmdStatus hifamd_residual_batch(HifAmdHdl h, HifAmdOp op, const void *B, int64_t ldb, const void *X, int64_t ldx,
                                   void *R, int64_t ldr, int64_t nrhs, int mode);
HifAmdStatus hifamd_residual_batch_dev(HifAmdHdl h, HifAmdOp op, const void *dB, int64_t ldb, const void *dX, int64_t ldx,
                                       void *dR, int64_t ldr, int64_t nrhs, int mode, void *stream);
/* GMRES-based iterative refinement (Carson and Higham's GMRES-IR) for nrhs columns, 64 in lock step: x = 0; per outer
 * step k = 0, 1, ...: r = b - A x, ALWAYS compensated (k = 0: r = b); res = ||r|| / ||b||; res <= rtol: flag 0;
 * k > 0 and res not below the step before: flag 1 (stagnated), the column gets back the iterate of the step before;
 * k == max_outer: flag 2; otherwise d = hifamd_gmres_batch_dev on A d = r (x0 = 0, restart, inner_rtol relative to
 * ||r||, inner_maxit, rank; its restart residuals follow the handle's mode) and x += d.  A column that has stopped is
 * frozen: its later bits do not depend on its neighbours.  The residual and the correction are kept in blocks as wide as
 * the widest tile the handle takes (64 columns, or the max_nrhs of hifamd_finalize where the arena is narrower), so a
 * column's x and relres do not depend on the width of the batch either -- and a narrow batch costs the memory and the
 * vector passes of a full tile.  A zero column: x = 0, flag 0, 0 steps; a column whose norm or
 * residual is not finite: flag 1 at once.  Per column (each array may be NULL): flags[c]; outer[c] = corrections that
 * the returned x contains; iters[c] = inner GMRES iterations spent; relres[c] = the compensated ||r|| / ||b|| of the
 * returned x, a certificate that holds below 1e-13 where a working-precision residual is noise.  Refusals as for
 * hifamd_gmres_batch (inner_maxit for maxit), plus inner_rtol outside (0, 1) or max_outer < 1
 * HIFAMD_MISMATCHED_SIZES.  Host pointers; the _dev variant takes device pointers for B, X (the other arrays stay
 * host arrays) and returns when the solve is done. */
HifAmdStatus hifamd_gmres_ir_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs,
                                   int restart, double rtol, double inner_rtol, int max_outer, int inner_maxit,
                                   int64_t rank, int *flags, int *outer, int *iters, double *relres);
HifAmdStatus hifamd_gmres_ir_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs,
                                       int restart, double rtol, double inner_rtol, int max_outer, int inner_maxit,
                                       int64_t rank, int *flags, int *outer, int *iters, double *relres);

/* ---- preconditioned CG for a Hermitian positive-definite pair (A, M), batched --------------- */
/* 1 when M^{-1} of the imported hierarchy is Hermitian, 0 when not, -1 for a NULL handle.  Exact test on the host
 * copy, every sparse level: U_B == L_B^H (same pattern, equal values), F == E^H (F absent only if E is empty),
 * s == t, p == q, Im d == 0; the last level absent or imported with hifamd_set_dense_symm (a QRCP or LUP block fails).
 * This is what a hierarchy factorized with is_symm satisfies; a nonsymmetric factorization of a symmetric matrix does
 * not.  Computed once per imported hierarchy; works before hifamd_finalize and without a GPU.  On 0, hifamd_last_error()
 * names the first violation ("level <l>: <what>"). */
int hifamd_hermitian(HifAmdHdl h);
/* Standard preconditioned CG with x0 = 0 for nrhs columns in lock step: q = A p, alpha = rho / p^H q, x += alpha p,
 * r -= alpha q, stop on ||r|| / ||b|| <= rtol, z = M^{-1} r, rho' = r^H z, p = z + (rho' / rho) p.  All vectors and the
 * per-column scalars stay in HBM (four work vectors r, z, p, q per 64-column tile, no restarts); one batched apply, one
 * SpMM and four fused vector passes serve every column per step, and the host reads back one integer per step.
 * Inner products are Hermitian (sum conj(a_i) b_i) and their summation order depends on n only, so a column's result
 * does not depend on the batch it is solved in.  Needs hifamd_set_matrix and a Hermitian M^{-1} (hifamd_hermitian; the
 * HIFAMD_BAD_PREC message names the level and the array of the first violation); a constant-mode null-space filter on
 * HIFAMD_S (hifamd_set_nsp_const) is not supported and refused with HIFAMD_BAD_PREC.  With a BASIS filter on HIFAMD_S
 * (hifamd_set_nsp_basis, P = I - Q Q^H) PCG runs projected, on the complement of span(Q): r0 = P b, ||b|| in the
 * stopping test is ||P b||, every z is P M^{-1} r; when Q spans the null space of a Hermitian positive semi-definite A
 * the operator PCG sees is P M^{-1} P, Hermitian with M^{-1}, and x is the solution without a component in span(Q).
 * The inconsistent part of b, (I - P) b, is DROPPED: the result solves A x = P b, i.e. it is the filtered
 * representative of the least-squares solutions only when Q spans null(A); if Q is not a null space of A the
 * breakdown flag or maxit report it.  P b = 0 is the zero column.  maxit < 1 or rtol <= 0:
 * HIFAMD_MISMATCHED_SIZES.  rank: 0 numerical rank, -1 full.  Per column: flags[c] = 0 converged / 1 breakdown (p^H A p
 * or r^H M^{-1} r not positive or not finite: A or M is not positive definite on that column) / 2 reached maxit,
 * iters[c] = iterations (a zero column: x = 0, flag 0, 0 iterations); either may be NULL.  Host pointers; the _dev
 * variant takes device pointers for B, X (flags, iters stay host arrays) and returns when the solve is done. */
HifAmdStatus hifamd_pcg_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs,
                              double rtol, int maxit, int64_t rank, int *flags, int *iters);
HifAmdStatus hifamd_pcg_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs,
                                  double rtol, int maxit, int64_t rank, int *flags, int *iters);

/* ---- breakdown-free block CG for a Hermitian positive-definite pair (A, M) -------------------- */
/* Block CG with x0 = 0 (Dubrulle's BCGrQ, preconditioned): the batch is cut into tiles of `block` <= 64 columns, and the
 * columns of a tile share ONE block Krylov space -- every column is minimised over the directions generated by all of them,
 * where hifamd_pcg_batch runs 64 independent spaces in lock step.  The block residual is kept factored, R = Q C with
 * Q^H M^{-1} Q = I, and rank loss (dependent, duplicate or zero columns, directions that converge before the others)
 * shrinks the block through a pivoted Cholesky instead of breaking down:
 *   start: beta_j = ||b_j||; R = B diag(1 / beta); Z = M^{-1} R; G = R^H Z = S^H S, the upper Cholesky factor by the
 *     largest remaining diagonal (ties: the lowest index), stopped when that diagonal is <= deftol * max diag G: rank r,
 *     S is r x s; E = I[:, piv] inv(S[:, piv]); Q = R E; P = Z E; C = S
 *   per step: T = A P; alpha = (P^H T)^{-1} by an unpivoted Cholesky; X += P alpha C diag(beta); Q -= T alpha;
 *     relres_j = sqrt(c_j^H (Q^H Q) c_j) = ||r_j|| / ||b_j||; stop when every column is <= rtol; W = M^{-1} Q;
 *     G = Q^H W = S^H S (pivoted as above, rank r'); Q <- Q E; P <- W E + P S^H; C <- S C; r = r'
 * A STEP is one batched M^{-1} apply plus one SpMM on the block, the unit of the PCG iteration count; on top of these
 * it costs two Gram products and two row-local [n][block] x [block][block] products on the f64 matrix cores and three
 * one-workgroup kernels on the small matrices.  Everything stays in HBM (four work vectors Q, W, P, T per tile); the host
 * reads back one integer per step.  Sums run in a fixed order: the same tile with the same inputs gives the same bits,
 * but -- unlike every other driver here -- a column's result DOES depend on the columns it shares a tile with.
 * Needs hifamd_set_matrix and a Hermitian M^{-1}, and treats the filters as hifamd_pcg_batch does: a constant-mode
 * filter on HIFAMD_S is refused with HIFAMD_BAD_PREC, with a basis filter the iteration runs projected (R = P B,
 * beta = ||P b||, every apply filtered).  maxit < 1, rtol <= 0, block outside [1, 64] or deftol outside (0, 1):
 * HIFAMD_MISMATCHED_SIZES.  deftol: 1e-12 sits two decades above the rounding of a 64-column Gram.  rank: 0 numerical
 * rank, -1 full.  Per column: flags[c] = 0 converged / 1 breakdown / 2 reached maxit; iters[c] = the steps of its tile,
 * the same for all its columns.  A zero column: x = 0, flag 0, 0 iterations.  A column whose ||b||^2 is not finite is
 * excluded: x = 0, flag 1, 0 iterations; it enters the block as an exact zero and does not touch its neighbours.  A
 * breakdown (P^H A P not positive definite: a pivot <= 0 or not finite; a Gram with a non-finite entry or a leftover
 * diagonal below -deftol * max diag; r' = 0 with columns still unconverged) ends the tile: every column that was not
 * <= rtol at its last test gets flag 1, iters = completed steps.  ranks (may be NULL): int[2 * ceil(nrhs / block)], per
 * tile its rank after the start and during its last step.  flags and iters may be NULL.  Host pointers; the _dev variant
 * takes device pointers for B, X (flags, iters, ranks stay host arrays) and returns when the solve is done. */
HifAmdStatus hifamd_bcg_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs, int block,
                              double rtol, double deftol, int maxit, int64_t rank, int *flags, int *iters, int *ranks);
HifAmdStatus hifamd_bcg_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs, int block,
                                  double rtol, double deftol, int maxit, int64_t rank, int *flags, int *iters, int *ranks);

/* ---- LOBPCG: the smallest eigenpairs of a Hermitian pair (A, M) -------------------------------- */
/* Knyazev's locally optimal block preconditioned CG for the nev smallest eigenvalues of the Hermitian matrix given to
 * hifamd_set_matrix and their eigenvectors, with the hierarchy as preconditioner.  A block of k <= 16 candidates gives the
 * basis S = [X W P] of s = 3 k <= 48 columns; columns nev .. k - 1 are guard columns, which sharpen convergence and never
 * hold the solve up.  ||A||_inf is the largest row sum of |a_ij|.
 *   start: X = X0 ([n][k], row stride ldx0), or, for X0 == NULL, entry (i, j) from counter 16 i + j + 1 of the probe stream
 *     of `seed` (the imaginary part from counter 16 (n + i) + j + 1; hifamd_nsp_find states the generator); with a basis
 *     filter on HIFAMD_S in force X <- (I - Q Q^H) X; G = X^H X = S^H S, the pivoted upper Cholesky factor of
 *     hifamd_bcg_batch stopped at deftol; X <- X I[:, piv] inv(S[:, piv]); AX = A X; X^H AX = V Theta V^H (ascending),
 *     X <- X V, AX <- AX V, lambda = Theta, P = AP = 0
 *   loop: R = AX - X diag(lambda); res_j = ||r_j||_2 / ||A||_inf (||x_j|| = 1 by construction); conv_j = res_j <= tol;
 *     every j < nev converged, or steps == maxit: end.  W = M^{-1} R on the columns that are not converged (filtered like
 *     every apply; a converged column of W is an exact zero: soft locking); AW = A W; steps += 1;
 *     GB = S^H S, GA = S^H [AX AW AP] (Hermitian parts); D = diag(GB)^(-1/2) (0 where the diagonal is not positive);
 *     D GB D = T^H T pivoted as above, rank r; E = D I[:, piv] inv(T[:, piv]); E^H GA E = V Theta V^H by a cyclic Jacobi
 *     method (ascending; equal values in index order); C = E V[:, :k]; lambda = Theta[:k]; Cp = C with its first k rows
 *     zero; X <- S C, AX <- AS C, P <- S Cp, AP <- AS Cp
 * A step is one batched M^{-1} apply plus one SpMM on k columns, one pass for both Grams and one row-local
 * [n][48] x [48][32] product on the f64 matrix cores, and the small matrices in one workgroup; the host reads back one
 * integer per step.  Sums run in a fixed order: the same inputs give the same bits.  The eigenvectors come back
 * orthonormal; their phase (sign) is not fixed.  Smallest eigenvalues of A only: no largest or interior ones; the
 * generalized problem A x = lambda B x is hifamd_lobpcg_gen's, more than k - guard eigenpairs are hifamd_eigs's.  The pair has to be definite for the iteration to converge; on an indefinite pair it runs to maxit
 * (flag 2), which is not refused.
 * Refusals, in this order: a NULL handle (HIFAMD_NULL_OBJ); k outside [1, 16], nev outside [1, k], tol <= 0, maxit < 1,
 * deftol outside (0, 1), a row stride below k (HIFAMD_MISMATCHED_SIZES); a handle that is not finalized (HIFAMD_BAD_PREC;
 * one finalized with max_nrhs < k: HIFAMD_MISMATCHED_SIZES), no matrix, a hierarchy that is not Hermitian, a constant-mode
 * filter on HIFAMD_S (HIFAMD_BAD_PREC, as hifamd_pcg_batch; with a basis filter the iteration runs on the complement of
 * span(Q) and returns the smallest eigenvalues there); a start block that is rank deficient (a Cholesky rank below k) or
 * not finite, or whose X^H A X is not finite (HIFAMD_BAD_PREC).
 * Out: lambda[k], X ([n][k], row stride ldx), res[k] (the last res_j), flags[k] -- per column by its own last res_j:
 * 0 converged, 2 not converged at maxit, 1 breakdown (a non-finite Gram, a basis of rank below k, a Jacobi method that has
 * not ended after 30 sweeps: lambda and X of the last completed step are returned) -- and info3 = {steps, rank of the
 * basis in the last step, largest Jacobi sweep count}; lambda, res, flags, info3 may be NULL.  rank: 0 numerical rank,
 * -1 full.  Host pointers; the _dev variant takes device pointers for X0 and X (the other arrays stay host arrays) and
 * returns when the solve is done. */
HifAmdStatus hifamd_lobpcg(HifAmdHdl h, int64_t k, int64_t nev, const void *X0, int64_t ldx0, uint64_t seed, double tol,
                           double deftol, int maxit, int64_t rank, double *lambda, void *X, int64_t ldx, double *res,
                           int *flags, int *info3);
HifAmdStatus hifamd_lobpcg_dev(HifAmdHdl h, int64_t k, int64_t nev, const void *dX0, int64_t ldx0, uint64_t seed, double tol,
                               double deftol, int maxit, int64_t rank, double *lambda, void *dX, int64_t ldx, double *res,
                               int *flags, int *info3);

/* ---- generalized LOBPCG: the smallest eigenpairs of A x = lambda B x ---------------------------- */
/* The mass matrix B in CRS (copied to HBM as a second matrix of the handle): arguments, index bases, checks and refusal
 * codes of hifamd_set_matrix.  It serves hifamd_lobpcg_gen only: it is not given to the adjoint engine, hifamd_save does not
 * write it, and like A it is NOT checked for being Hermitian or positive definite -- a B that is not shows as a refused start
 * block or as a breakdown.  ||B||_inf is the largest row sum of |b_ij|. */
HifAmdStatus hifamd_set_mass_matrix(HifAmdHdl h, int64_t n, const int64_t *indptr, const int32_t *indices,
                                    const void *vals);
/* hifamd_lobpcg for the nev smallest eigenvalues of the Hermitian definite pencil (A, B), B Hermitian positive definite: the
 * iteration, its arguments and its outputs with a third block BS = [BX BW BP] carried beside S and AS = [AX AW AP]:
 *   start: X as hifamd_lobpcg generates or takes it; BX = B X; G = X^H BX = S^H S (pivoted Cholesky stopped at deftol);
 *     X, BX <- . I[:, piv] inv(S[:, piv]); AX = A X; X^H AX = V Theta V^H, X, AX, BX <- . V, lambda = Theta, P = AP = BP = 0
 *   loop: R = AX - BX diag(lambda); res_j = ||r_j||_2 / ((||A||_inf + |lambda_j| ||B||_inf) ||x_j||_2), the normwise
 *     backward error of the pair (lambda_j, x_j) -- the vectors are B-normalized, so ||x_j||_2 is not 1 and belongs in the
 *     scale, and the test does not depend on how B is scaled; conv_j = res_j <= tol; every j < nev converged, or
 *     steps == maxit: end.  W = M^{-1} R (exact zeros in converged columns); AW = A W; BW = B W; steps += 1; GB = S^H BS,
 *     GA = S^H AS; the Rayleigh-Ritz step of hifamd_lobpcg on (GB, GA) unchanged; X, P <- S [C Cp], AX, AP <- AS [C Cp],
 *     BX, BP <- BS [C Cp]
 * A step costs one more SpMM on k columns than hifamd_lobpcg's, and its row passes read and move a third block.  The
 * orders of summation are hifamd_lobpcg's: with an explicit identity as B the iterates are that driver's, bit for bit,
 * until the two stopping tests decide differently.  Out: lambda ascending, X with X^H B X = I, res, flags, info3 as
 * hifamd_lobpcg.  Not done here: largest or interior eigenvalues; a null-space basis under B (the B-orthogonal projector) and more
 * eigenpairs than one block of k <= 16 holds are hifamd_eigs's: the null space goes into its constraint block Y.
 * Refusals in hifamd_lobpcg's order, with: no mass matrix (hifamd_set_mass_matrix; HIFAMD_BAD_PREC) directly after no
 * matrix; after the Hermitian check ANY null-space filter on HIFAMD_S, the constant-mode one and a basis filter alike
 * (HIFAMD_BAD_PREC): the Euclidean projector I - Q Q^H would solve the pencil (A, P B P), and the B-orthogonal projector
 * I - Q (Q^H B Q)^{-1} Q^H B is not implemented; a start block whose X^H B X is not finite, or has a Cholesky rank below k
 * -- a rank-deficient block, or a B that is not positive definite: the message names both -- or whose X^H A X is not
 * finite (HIFAMD_BAD_PREC). */
HifAmdStatus hifamd_lobpcg_gen(HifAmdHdl h, int64_t k, int64_t nev, const void *X0, int64_t ldx0, uint64_t seed, double tol,
                               double deftol, int maxit, int64_t rank, double *lambda, void *X, int64_t ldx, double *res,
                               int *flags, int *info3);
HifAmdStatus hifamd_lobpcg_gen_dev(HifAmdHdl h, int64_t k, int64_t nev, const void *dX0, int64_t ldx0, uint64_t seed, double tol,
                                   double deftol, int maxit, int64_t rank, double *lambda, void *dX, int64_t ldx, double *res,
                                   int *flags, int *info3);

/* ---- locked LOBPCG sweeps: up to 128 eigenpairs, constraints under B ------------------------------ */
/* The B-orthogonal projector alone: W <- W - Y C, C = (BY)^H W, for Y ([n][m], 1 <= m <= 128, row stride ldy) with
 * B-orthonormal columns and W ([n][kw], 1 <= kw <= 16, row stride ldw), in place.  gen == 0: B = I (BY is Y, no copy);
 * gen != 0: B is the mass matrix and BY = B Y is formed here, 64 columns a product.  C is summed in a fixed order on the f64
 * matrix cores (the same inputs give the same bits); a column of W that is exactly zero keeps its bits, and no column of W
 * reads another.  Y is NOT checked for orthonormality here.  Refusals, in this order: a NULL handle; m outside [1, 128], kw
 * outside [1, 16], a row stride below its block (HIFAMD_MISMATCHED_SIZES); a handle that is not finalized, gen without a
 * mass matrix (HIFAMD_BAD_PREC); a NULL block (HIFAMD_NULL_OBJ).  The _dev variant takes device pointers and returns when
 * the projection is done. */
HifAmdStatus hifamd_eig_project(HifAmdHdl h, int gen, int64_t m, const void *Y, int64_t ldy, int64_t kw, void *W, int64_t ldw);
HifAmdStatus hifamd_eig_project_dev(HifAmdHdl h, int gen, int64_t m, const void *dY, int64_t ldy, int64_t kw, void *dW,
                                    int64_t ldw);
/* The nev smallest eigenpairs of A (gen == 0) or of the pencil (A, B) (gen != 0), m0 + nev <= 128, by sweeps of
 * hifamd_lobpcg / hifamd_lobpcg_gen on blocks of k <= 16 candidates, `guard` of them guard columns (0 <= guard < k), under
 * the constraint block Y of locked, B-orthonormal vectors: hard locking plus constraints.
 *   Y = the caller's m0 >= 0 columns ([n][m0], row stride ldy; NULL with m0 = 0), BY = B Y; L = 0;
 *   X0 = the caller's block ([n][k]) or the generated one of `seed`, as hifamd_lobpcg takes or generates it
 *   sweep t = 0, 1, ...: want = min(nev - L, k - guard); the iteration of hifamd_lobpcg(_gen) with (k, nev = want, tol,
 *     deftol, maxit PER SWEEP) and two more operations: X <- X - Y (BY)^H X once, directly behind the start block (and the
 *     basis filter of the standard problem) and in front of BX = B X, and W <- W - Y (BY)^H W once per step, directly
 *     behind W = M^{-1} R and in front of AW = A W (converged columns of W stay exact zeros);
 *     p = the length of the leading run of flag-0 columns among the first `want`; p == 0: end;
 *     X_c = X[:, :p], projected once more, is appended to Y (generalized: B X_c is recomputed, appended to BY); L += p;
 *     L == nev: end; the next X0 = [X[:, p:k] | p columns generated from seed + t + 1] (P is dropped)
 * With m0 = 0 and nev <= k - guard this is one sweep without a projector launch: the bits of hifamd_lobpcg(_gen) with
 * (k, nev).  Y and BY live in two [n][128] buffers of the handle, allocated at the first call that needs them.
 * Out: lambda[nev] in lock order (ascending up to the tolerance), X ([n][nev], row stride ldx; X^H B X = I, Y^H B X = 0),
 * res[nev], flags[nev]: 0 locked, 1 breakdown, 2 not converged -- the columns the last sweep asked for and did not lock
 * carry its candidates with its flag (a converged one behind an unconverged one counts as 2), the columns never reached
 * are zero with lambda = res = NaN and flag 2 -- and info4 = {total steps, sweeps, locked, smallest basis rank seen};
 * lambda, res, flags, info4 may be NULL.  hifamd_eigs_sweeps returns the sweeps' (want, locked, steps).
 * Refusals, in this order: a NULL handle; hifamd_lobpcg's argument checks with nev = want of the first sweep; guard outside
 * [0, k), nev < 1, m0 < 0 or m0 + nev > 128, a row stride below its block (HIFAMD_MISMATCHED_SIZES); Y == NULL with m0 > 0
 * (HIFAMD_NULL_OBJ); the handle checks of hifamd_lobpcg / hifamd_lobpcg_gen in their order -- with gen every null-space
 * filter stays refused (the constraint block is how a null space is deflated there), on the standard problem a basis
 * filter keeps working; a Y with max |Y^H B Y - I| > 1e-10 (HIFAMD_BAD_PREC: orthonormalizing Y is the caller's job); a
 * sweep's start block that hifamd_lobpcg refuses.
 * Not done here: largest or interior eigenvalues, orthonormalizing Y, more than 128 locked vectors.  Host pointers; the
 * _dev variant takes device pointers for Y, X0 and X. */
HifAmdStatus hifamd_eigs(HifAmdHdl h, int gen, int64_t nev, int64_t k, int64_t guard, const void *Y, int64_t ldy, int64_t m0,
                         const void *X0, int64_t ldx0, uint64_t seed, double tol, double deftol, int maxit, int64_t rank,
                         double *lambda, void *X, int64_t ldx, double *res, int *flags, int *info4);
HifAmdStatus hifamd_eigs_dev(HifAmdHdl h, int gen, int64_t nev, int64_t k, int64_t guard, const void *dY, int64_t ldy, int64_t m0,
                             const void *dX0, int64_t ldx0, uint64_t seed, double tol, double deftol, int maxit, int64_t rank,
                             double *lambda, void *dX, int64_t ldx, double *res, int *flags, int *info4);
/* (want, locked, steps) of every sweep of the handle's last hifamd_eigs(_dev) call: at most cap triples into out (may be
 * NULL) -> the number of sweeps, -1 for a NULL handle */
int hifamd_eigs_sweeps(HifAmdHdl h, int *out, int cap);

/* ---- restarted block GCR for a general pair (A, M): a shared block space without conditions ---- */
/* Restarted block GCR with x0 = 0: in exact arithmetic block GMRES(restart) with right preconditioning, flexible by
 * construction.  The batch is cut into tiles of `block` <= 64 columns, and the columns of a tile share ONE block Krylov
 * space, as in hifamd_bcg_batch -- but nothing is asked of the hierarchy: no Hermitian M^{-1}, no definite A.  The
 * residual is kept factored and rank-revealed, relative residual = Rh C with Rh^H Rh = I:
 *   beta_j = ||b_j||; X = 0; steps = 0; mu_prev = inf
 *   cycle c = 0, 1, ...:
 *     R = B - A X in the handle's residual precision (c = 0: R = B); rho_j = ||R_j||; t_j = rho_j / beta_j
 *     all t_j <= rtol: flags 0, end.  steps == maxit: flag 0 / 2 by t_j, end.
 *     mu = max_j t_j; c > 0 and not mu < mu_prev: flag 0 / 1 (stagnated) by t_j, end.  mu_prev = mu
 *     Rn = R diag(1 / rho); G = Rn^H Rn = S^H S, the upper Cholesky factor by the largest remaining diagonal (ties: the
 *       lowest index), stopped when that diagonal is <= deftol * max diag G: rank r, S is r x s;
 *       Rh = Rn I[:, piv] inv(S[:, piv]); C = S diag(rho / beta).  r == 0 or a bad Gram: flag 0 / 1 by t_j, end.
 *     for j = 0 .. restart - 1:
 *       Z = M^{-1} Rh; W = A Z; steps += 1
 *       C_i = Q_i^H W for every stored i < j (all from the same W); W -= sum Q_i C_i; Z -= sum P_i C_i
 *       W^H W = S1^H S1 (pivoted as above, rank q; q == 0 ends the cycle); E = I[:, piv] inv(S1[:, piv]);
 *       Q_j = W E; P_j = Z E   (A P_j = Q_j, Q_j^H Q_i = delta_ij I)
 *       D = Q_j^H Rh; X += P_j D C diag(beta); Rh -= Q_j D; H = Rh^H Rh; rel_j = sqrt(max(0, c_j^H H c_j))
 *       all rel_j <= rtol, steps == maxit or j == restart - 1: the cycle ends, before H is factored
 *       H = S^H S (pivoted, rank r'; r' == 0 ends the cycle); Rh <- Rh I[:, piv] inv(S[:, piv]); C <- S C; r = r'
 * A STEP is one batched M^{-1} apply plus one SpMM on the block, the unit of every other driver here: maxit caps steps and
 * iters[c] is the step count of the column's tile.  EVERY FLAG 0 IS DECIDED ON A TRUE RESIDUAL b - A x formed at a
 * cycle's start; the recurrence's rel_j only ends a cycle early, and what a pivoted Cholesky drops is therefore looked at
 * again at the next cycle's start: a drop cannot make a column pass.  A converged column stays in the block and leaves
 * through the rank, as in block CG.  A column's bits depend on the columns it shares a tile with; the same tile with the
 * same inputs gives the same bits (fixed summation orders, no atomics); tiles do not see each other.  The filters are
 * treated as hifamd_bicgstab_batch treats them: every M^{-1} apply is filtered, nothing else, and a constant-mode filter
 * is allowed.  On top of the apply and the SpMM a step costs the stacked Gram against the cycle's blocks, one fused
 * projection pass, two more Grams, the update pass and two in-place [n][block] x [block][block] products on the f64
 * matrix cores, three one-workgroup kernels, and one integer read back; a cycle's start costs a residual, a Gram and a
 * second read-back.  Memory: 2 * restart + 1 blocks of [n][block] on the device plus restart + 4 matrices of 64 x 64.
 * Refusals as hifamd_bicgstab_batch, then block outside [1, 64], restart outside [1, HIFAMD_BGCR_MAX_RESTART] or deftol
 * outside (0, 1): HIFAMD_MISMATCHED_SIZES.  rank: 0 numerical rank, -1 full.  flags[c] = 0 converged / 1 stagnated, a bad
 * Gram (a non-finite entry, a leftover diagonal below -deftol * max diag) or excluded / 2 reached maxit.  A zero column:
 * x = 0, flag 0, 0 steps.  A column whose ||b||^2 is not finite is excluded as in hifamd_bcg_batch: x = 0, flag 1, 0 steps;
 * it enters the block as an exact zero and does not touch its neighbours.  ranks (may be NULL):
 * int[2 * ceil(nrhs / block)], per tile its rank after the start of its first cycle and the rank of Rh during its last
 * step.  flags and iters may be NULL.  Host pointers; the _dev variant takes device pointers for B, X (flags, iters, ranks
 * stay host arrays) and returns when the solve is done. */
#define HIFAMD_BGCR_MAX_RESTART 64
HifAmdStatus hifamd_bgcr_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs, int block,
                               int restart, double rtol, double deftol, int maxit, int64_t rank, int *flags, int *iters,
                               int *ranks);
HifAmdStatus hifamd_bgcr_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs, int block,
                                   int restart, double rtol, double deftol, int maxit, int64_t rank, int *flags, int *iters,
                                   int *ranks);

/* ---- right-preconditioned BiCGSTAB for a general (non-Hermitian) pair (A, M), batched --------- */
/* BiCGSTAB with x0 = 0 and shadow residual r^ = b for nrhs columns in lock step: r = b, rho = (r^, r), p = r; per
 * iteration y = M^{-1} p, v = A y, alpha = rho / (r^, v), x += alpha y, r -= alpha v, test; y = M^{-1} r, t = A y,
 * omega = (t, r) / (t, t), x += omega y, r -= omega t, test; rho' = (r^, r), beta = (rho' / rho)(alpha / omega),
 * p = r + beta (p - omega v).  The test is ||r|| / ||b|| <= rtol.  A STEP is one M^{-1} apply plus one SpMM (the unit
 * of the GMRES and PCG iteration counts): maxit caps steps, and iters[c] reports steps, so a column may stop on an odd
 * count (converged, or maxit reached, after the first half of an iteration).  All vectors and the per-column scalars
 * stay in HBM (five work vectors r, p, v, y, t per 64-column tile; r^ is B itself, read in place; no restarts); the
 * host reads back one integer after each of the two tests of an iteration.  Inner products are Hermitian
 * (sum conj(a_i) b_i) and their summation order depends on n only, so a column's result does not depend on the batch
 * it is solved in.  A null-space filter on HIFAMD_S (hifamd_set_nsp_const / hifamd_set_nsp_basis) filters every
 * M^{-1} apply, as in GMRES, and nothing else: b is taken as it is (hifamd_nsp_filter_batch makes it consistent);
 * M^{-1} need not be Hermitian.  Needs hifamd_set_matrix (else HIFAMD_BAD_PREC, as for a handle not finalized);
 * maxit < 1 or rtol <= 0: HIFAMD_MISMATCHED_SIZES.  rank: 0 numerical rank, -1 full.  Per column: flags[c] = 0
 * converged / 1 breakdown ((r^, v), (t, t), omega, rho' or the initial rho exactly zero or not finite; x keeps its last
 * completed update) / 2 reached maxit, iters[c] = steps taken (a zero column: x = 0, flag 0, 0 steps; a non-finite
 * column: flag 1, 0 steps); either may be NULL.  Host pointers; the _dev variant takes device pointers for B, X
 * (flags, iters stay host arrays), writes X in place and returns when the solve is done. */
HifAmdStatus hifamd_bicgstab_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs,
                                   double rtol, int maxit, int64_t rank, int *flags, int *iters);
HifAmdStatus hifamd_bicgstab_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs,
                                       double rtol, int maxit, int64_t rank, int *flags, int *iters);

/* ---- right-preconditioned IDR(s) for a general (non-Hermitian) pair (A, M), batched ------------ */
/* IDR(s) with biorthogonalization (van Gijzen and Sonneveld, ACM TOMS 38(1), 2011) and its "maintaining convergence"
 * choice of omega (kappa = 0.7), x0 = 0, for nrhs columns in lock step.  P is the [n][s] shadow block, (a, b) = sum
 * conj(a_i) b_i:
 *   r = b; G = U = 0 (n x s each); M = I_s; omega = 1
 *   cycle: f = P^H r
 *     for k = 0 .. s-1:  c_k .. c_{s-1} by forward substitution on the lower triangle M[k:, k:] c = f[k:];
 *       v = r - sum_{i>=k} c_i g_i; v^ = M^{-1} v; u = omega v^ + sum_{i>=k} c_i u_i; g = A u   (a step); raw = P^H g;
 *       alpha_i = (raw_i - sum_{l<i} alpha_l M[i,l]) / M[i,i] (i < k); M[i,k] = raw_i - sum_{l<k} alpha_l M[i,l] (i >= k);
 *       g_k = g - sum_{l<k} alpha_l g_l; u_k = u - sum_{l<k} alpha_l u_l; beta = f_k / M[k,k]; r -= beta g_k;
 *       x += beta u_k; test; f_i = 0 (i <= k); f_i -= beta M[i,k] (i > k)
 *     v^ = M^{-1} r; t = A v^   (a step); omega = (t, r) / (t, t); rho = |(t, r)| / (||t|| ||r||);
 *     rho < kappa: omega *= kappa / rho; r -= omega t; x += omega v^; test
 * The test is ||r|| / ||b|| <= rtol, r by recurrence (the residual precision of the handle plays no part).  A STEP is
 * one M^{-1} apply plus one SpMM, the unit of a BiCGSTAB step: maxit caps steps and iters[c] reports them.  Short
 * recurrences, 2 s + 4 work vectors per 64-column tile (r, v, v^, t, G, U) and the per-column scalars in HBM; the host
 * reads back one integer per step.  All columns of a tile share k; a column that stops is frozen.  The summation order
 * of every inner product depends on n only, so a column's x, flag and steps depend on neither the batch width nor its
 * neighbours.  s: 1 .. HIFAMD_IDRS_MAX.  P: a HOST pointer in both variants, [n][s] of the handle's value type,
 * row-interleaved with row stride ldp >= s, one block for all columns, used exactly as given (not orthonormalized); or
 * NULL: the block is generated on the device from seed, entry (i, j) = probe_value(seed, 16 i + j + 1), the imaginary
 * part of a complex entry probe_value(seed, 16 (n + i) + j + 1) -- the first s columns of the block hifamd_nsp_find
 * draws from the same seed (the generator is specified there), not orthonormalized either.  A null-space filter on
 * HIFAMD_S (hifamd_set_nsp_const / hifamd_set_nsp_basis) filters every M^{-1} apply and nothing else, as in BiCGSTAB.
 * Refusals as hifamd_bicgstab_batch, in its order (needs hifamd_set_matrix: HIFAMD_BAD_PREC; maxit < 1 or rtol <= 0:
 * HIFAMD_MISMATCHED_SIZES), then s < 1, s > HIFAMD_IDRS_MAX or P given with ldp < s: HIFAMD_MISMATCHED_SIZES, then a
 * non-finite entry of P: HIFAMD_BAD_PREC.  rank: 0 numerical rank, -1 full.  Per column: flags[c] = 0 converged /
 * 1 breakdown (M[k,k], (t, t) or (t, r) exactly zero or not finite; x keeps its last completed update) / 2 reached maxit,
 * iters[c] = steps taken (a zero column: x = 0, flag 0, 0 steps; a non-finite column: flag 1, 0 steps); either may be
 * NULL.  Host pointers; the _dev variant takes device pointers for B, X (P, flags, iters stay host arrays), writes X in
 * place and returns when the solve is done. */
#define HIFAMD_IDRS_MAX 8
HifAmdStatus hifamd_idrs_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs, int s,
                               const void *P, int64_t ldp, uint64_t seed, double rtol, int maxit, int64_t rank,
                               int *flags, int *iters);
HifAmdStatus hifamd_idrs_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs, int s,
                                   const void *P, int64_t ldp, uint64_t seed, double rtol, int maxit, int64_t rank,
                                   int *flags, int *iters);

/* ---- symmetric QMR for a Hermitian INDEFINITE pair (A, M), batched ---------------------------- */
/* The symmetric QMR of Freund and Nachtigal with x0 = 0 for nrhs columns in lock step: PCG's coupled two-term
 * recurrence without the positivity requirement (A M^{-1} is self-adjoint in the indefinite form induced by M^{-1}),
 * plus a quasi-minimal-residual smoothing of the iterates:
 *   r = b; s = b; tau = ||b||; theta = 0; d = g = 0; z = M^{-1} r; rho = (r, z); p = z
 *   per iteration: q = A p; sigma = (p, q); alpha = rho / sigma; r -= alpha q;
 *     theta' = ||r|| / tau; c2 = 1 / (1 + theta'^2); tau = tau theta' sqrt(c2); eta = c2 theta^2; zeta = c2 alpha;
 *     theta = theta'; d = eta d + zeta p; g = eta g + zeta q; x += d; s -= g;
 *     stop on ||s|| / ||b|| <= rtol; z = M^{-1} r; rho' = (r, z); p = z + (rho' / rho) p; rho = rho'
 * s is the residual b - A x of the smoothed iterate, by recurrence; the raw residual r underneath may be erratic.  An
 * ITERATION is one M^{-1} apply plus one SpMM, the unit of the PCG iteration count and of a BiCGSTAB step.  All vectors
 * and the per-column scalars stay in HBM (seven work vectors r, z, p, q, d, g, s per 64-column tile, no restarts); the
 * host reads back one integer per iteration.  Inner products are Hermitian (sum conj(a_i) b_i) and their summation
 * order depends on n only, so a column's result does not depend on the batch it is solved in.  Needs
 * hifamd_set_matrix and a Hermitian M^{-1} (hifamd_hermitian; the HIFAMD_BAD_PREC message names the level and the array
 * of the first violation and points to is_symm, GMRES and BiCGSTAB); M^{-1} and A may be indefinite (a positive-definite
 * pair is a valid input too).  A constant-mode null-space filter on HIFAMD_S (hifamd_set_nsp_const) is refused with
 * HIFAMD_BAD_PREC.  With a BASIS filter on HIFAMD_S (hifamd_set_nsp_basis, P = I - Q Q^H) the iteration runs projected
 * exactly as hifamd_pcg_batch does: r0 = s0 = P b, ||b|| in the stopping test is ||P b||, every z is P M^{-1} r, and
 * P b = 0 is the zero column.  maxit < 1 or rtol <= 0: HIFAMD_MISMATCHED_SIZES.  rank: 0 numerical rank, -1 full.  Per
 * column: flags[c] = 0 converged / 1 breakdown (rho = (r, z) or sigma = (p, A p) exactly zero or not finite, no sign
 * test; x keeps its last update) / 2 reached maxit, iters[c] = iterations (a zero column: x = 0, flag 0, 0 iterations;
 * a non-finite column: flag 1, 0 iterations); either may be NULL.  Host pointers; the _dev variant takes device
 * pointers for B, X (flags, iters stay host arrays) and returns when the solve is done. */
HifAmdStatus hifamd_sqmr_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs,
                               double rtol, int maxit, int64_t rank, int *flags, int *iters);
HifAmdStatus hifamd_sqmr_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs,
                                   double rtol, int maxit, int64_t rank, int *flags, int *iters);

/* ---- instrumentation ---------------------------------------------------------------------- */
/* Average device time (ms) of the last `hifamd_solve_batch_dev`-shaped graph over `reps` replays,
 * measured with HIP events on the handle's stream (the stream the kernels run on). */
HifAmdStatus hifamd_time_apply(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx,
                               int64_t nrhs, int64_t rank, int warmup, int reps, double *ms_avg);
HifAmdStatus hifamd_sync(HifAmdHdl h);
/* Stream-ordered copy of an [n][ncols] block (device memory of the handle's device, row stride lds) into the columns
 * [col0, col0 + ncols) of dst (row stride ldd; device memory of ANY device of the process: a peer copy), enqueued on
 * the handle's own stream behind whatever was enqueued there with stream = NULL -- the gather of an RHS-sharded batch
 *  without a host round trip.  Not synchronized (hifamd_sync). */
HifAmdStatus hifamd_copy_columns_dev(HifAmdHdl h, const void *src, int64_t lds, int64_t ncols, void *dst, int64_t ldd,
                                     int64_t col0);
/* development aid: checksums of the device-resident arrays of a finalized handle (per level: the nine
 * arrays of L, U, E, F, then d, s, t, p, q_inv; finally Q^H, R^{-1}, jpvt and the rank); returns how many */
int hifamd_debug_checksums(HifAmdHdl h, uint64_t *out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* HIFIR_AMD_H */
