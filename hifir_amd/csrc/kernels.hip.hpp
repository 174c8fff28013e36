// kernels.hip.hpp -- hand-written gfx950 (CDNA4, wave64) kernels of the HIFIR apply path.
//
// Vector layout everywhere: row-interleaved [n][R], R = 2^logR <= 64 right-hand sides per row
// (the layout of hif::Array<std::array<T,Nrhs>>, ds/CompressedStorage.hpp:2127).  A wave64 is split
// into G = 64/R row groups of R lanes: lane = g*R + c handles RHS column c of the g-th row the wave
// currently owns.  R = 64: one wave per row, one coalesced 512-B access per touched row;
// R = 1: one lane per row.  Inside a row every lane walks the nonzeros SEQUENTIALLY in the
// reference's accumulation order with separate multiply and subtract/add (the TU is compiled with
// -ffp-contract=off), so every sparse stage is bit-identical to the reference's scalar loops for
// every batch width.
//
// Reference loops restated as row gathers (file:line relative to the reference tree):
//   k_trsv_*  L: CCS::solve_as_strict_lower   ds/CompressedStorage.hpp:2268-2279 (+ mrhs :2287)
//             D: y[i] /= d[i]                 alg/prec_solve.hpp:219 (fused into the first U kernel that touches a row)
//             U: CCS::solve_as_strict_upper   ds/CompressedStorage.hpp:2357-2369 (+ mrhs :2377)
//   k_trsv_band_p the band form at R = 64 (trsv_band_r64): next row's head behind the last gathers, one poll per item,
//                 carried prefixes of the next band on the idle compute units (host.hpp finish_band_plan)
//   k_spmm_epi    CCS::multiply_nt_low :2079 fused with  y = s[p]*b[p] - y  prec_solve.hpp:366-368,397-399
//                 (R = 64: spmm_stream_r64, the same item/batch pipeline)
//   k_gather_scale   work[i] = s[p[i]]*b[p[i]]           alg/prec_solve.hpp:359,402
//   k_scatter_scale  y[i] = t[i]*work[q_inv[i]]          alg/prec_solve.hpp:411
//   k_dense_gemm     QRCP::_solve_nt (ormqr, trsv, perm) small_scale/QRCP.hpp:371-411 on f64 MFMA
//   k_crs_spmm       CRS::multiply_nt_low(x,istart,len,y) ds/CompressedStorage.hpp:1109-1127
//   k_thin_update + k_tri_gemm_d   the thin tail of a triangle in block-dense form (host.hpp plan_dense_blocks)
//   k_gather_div / k_prod_rows / k_spmm_prod / k_scatter_div   prec_prod, alg/prec_prod.hpp:55-147
//   k_zcombine       complex products as two real MFMA products
//   k_top_gemm_z / k_top_reduce_z   top and tail operators of a complex handle (hifamd_set_complex_operators): both real
//                    products in one kernel, combined across neighbouring lanes
//   k_gm_step / k_gm_finish / k_gm_backsolve / k_gm_combine / k_gm_colop   device-resident Arnoldi process of GMRES
//   k_cg_dot / k_cg_xr / k_cg_p / k_cg_finish   device-resident preconditioned CG (batch-width-independent reductions)
//   k_bs_tr / k_bs_xr_full / k_bs_p / k_bs_finish   device-resident BiCGSTAB (same reductions; with k_cg_dot and k_cg_xr)
//   k_qm_r / k_qm_ds / k_qm_finish   device-resident symmetric QMR for Hermitian indefinite pairs (same reductions;
//                    with k_cg_dot and k_cg_p)
//   k_idr_comb / k_idr_gu / k_idr_finish / k_idr_pfill   device-resident IDR(s) (same reductions; with k_cg_dot, k_cg_xr,
//                    k_bs_tr and, for P^H x, k_nsp_coef / k_nsp_finish)
//   k_bcg_gram / k_bcg_sum / k_bcg_xq / k_bcg_qp / k_bcg_small / k_bcg_beta / k_bcg_norm   device-resident block CG: Grams and
//                    row-local products on the f64 matrix cores, the small matrices in one workgroup (blockcg_small.hpp)
//   k_bgcr_gram / k_bgcr_sum / k_bgcr_proj / k_bgcr_rmul / k_bgcr_rho / k_bgcr_small   device-resident restarted block GCR: the
//                    stacked Gram, the fused block Gram-Schmidt pass, in-place right-multiplication, decisions (blockgcr_small.hpp)
//   k_lob_gram / k_lob_update / k_lob_resid / k_lob_lock / k_lob_small   device-resident LOBPCG: both Grams of the basis
//                    [X W P] in one pass, the row-local update, the Rayleigh-Ritz step in one workgroup (lobpcg_small.hpp);
//                    instantiated with a third block [BX BW BP] for the generalized problem A x = lambda B x
//   k_colsum_partial / k_sub_colmean   null-space-filter BLAS-1
//   k_nsp_coef / k_nsp_finish / k_nsp_sub   basis mode of the null-space filter: x -= Q (Q^H x)
//   k_probe_fill / k_blk_rmul   null-space search: counter-based probe block, V <- V C for a 16 x 16 C
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "band_lds.hpp"
#include "blockcg_small.hpp"
#include "blockgcr_small.hpp"
#include "lobpcg_small.hpp"

namespace hifamd {

struct cplx {
  double x, y;
};
typedef double v4f64 __attribute__((ext_vector_type(4)));  // accumulator tile of v_mfma_f64_16x16x4_f64

// ---- value-type arithmetic, spelled out so that no contraction / reassociation can happen ------
__device__ __forceinline__ double vzero(double) { return 0.0; }
__device__ __forceinline__ cplx vzero(cplx) { return cplx{0.0, 0.0}; }
__device__ __forceinline__ double vmul(double a, double b) { return a * b; }
__device__ __forceinline__ cplx vmul(cplx a, cplx b) {
  return cplx{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
}
__device__ __forceinline__ double vsub(double a, double b) { return a - b; }
__device__ __forceinline__ cplx vsub(cplx a, cplx b) { return cplx{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ double vadd(double a, double b) { return a + b; }
__device__ __forceinline__ cplx vadd(cplx a, cplx b) { return cplx{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ double vscale(double s, double a) { return s * a; }
__device__ __forceinline__ cplx vscale(double s, cplx a) { return cplx{s * a.x, s * a.y}; }
__device__ __forceinline__ double vdiv(double a, double b) { return a / b; }
__device__ __forceinline__ cplx vdiv(cplx a, cplx b) {
  // Smith's algorithm (robust against overflow like libgcc's __divdc3; tolerance-level parity)
  if (fabs(b.x) >= fabs(b.y)) {
    const double r = b.y / b.x, den = b.x + b.y * r;
    return cplx{(a.x + a.y * r) / den, (a.y - a.x * r) / den};
  }
  const double r = b.x / b.y, den = b.x * r + b.y;
  return cplx{(a.x * r + a.y) / den, (a.y * r - a.x) / den};
}

// Workgroups are dealt round-robin to the 8 XCDs (each with its own L2).  Rows that are neighbours in
// the matrix share most of the vector rows they gather, so the streaming kernels renumber their
// workgroups such that every XCD walks ONE contiguous window of rows (a gathered row is then fetched
// into one L2 instead of up to eight).
__device__ int g_xcd_remap = 1;
__device__ __forceinline__ unsigned xcd_block() {
  const unsigned g = gridDim.x, b = blockIdx.x;
  if (!g_xcd_remap) return b;
  const unsigned q = g >> 3, r = g & 7u, x = b & 7u;
  return x * q + (x < r ? x : r) + (b >> 3);
}

__device__ __forceinline__ double vdivr(double a, double r) { return a / r; }
__device__ __forceinline__ cplx vdivr(cplx a, double r) { return cplx{a.x / r, a.y / r}; }

// lane decomposition
struct LaneMap {
  int g, c, G;
};
__device__ __forceinline__ LaneMap lane_map(int logR) {
  const int lane = threadIdx.x & 63;
  LaneMap m;
  m.g = lane >> logR;
  m.c = lane & ((1 << logR) - 1);
  m.G = 64 >> logR;
  return m;
}

// A caller-owned vector block as a kernel argument: either a plain pointer, or a pointer that the kernel
// reads from a device slot at run time (+ a column offset).  The latter lets ONE captured hipGraph serve
// every (B, X) pair of a given shape: the slot is rewritten before each replay instead of re-capturing
// the ~550 nodes whenever a Krylov solver hands over a different pair of vectors.
template <class T>
struct IoPtr {
  T *direct;
  T *const *slot;
  int64_t off;
  __device__ __forceinline__ T *get() const { return slot ? (*slot + off) : direct; }
};

// S1 fused into the triangular solve: the kernel that touches a row of L FIRST takes its right-hand side straight from
// the level's input, rhs[i] = s[p[i]] * b[p[i]] (prec_solve.hpp:359), instead of from a w[] that k_gather_scale wrote --
// one launch and one write + read of the level's rows less.  bin.direct == nullptr && bin.slot == nullptr: not fused.
template <class T>
struct FirstL {
  IoPtr<const T> bin;
  int64_t ldb;
  int nrhs;
  const int32_t *p;
  const double *s;
  __device__ __forceinline__ bool on() const { return bin.direct != nullptr || bin.slot != nullptr; }
};
template <class T>
__device__ __forceinline__ T first_l_rhs(const T *__restrict__ bin, const FirstL<T> &f, int32_t i, int lane) {
  const int32_t src = f.p[i];
  const T b = bin[(int64_t)src * f.ldb + min(lane, f.nrhs - 1)];
  return lane < f.nrhs ? vscale(f.s[src], b) : vzero(T());
}

// What a level's FIRST solve may leave out, per slot of a sparse-own triangle (engine.hip build_row_flags; NULL otherwise):
//   bit 0  nobody reads this row's result from memory in this solve: it is not stored (L: a row without entries whose
//          value only its own component uses; U: a row no other component and no column of E refers to);
//   bit 1  (U) the L solve did not store the row: its right-hand side is s[p[i]] * b[p[i]] (FirstL), the product the L
//          kernel would have stored.
// (p[i] and s[p[i]] in slot order beside the flags -- no dependent gathers -- measured SLOWER: the U band 244 -> 316 us.)
struct RowSkip {
  const uint8_t *flag;
};

// S7 fused into the LAST band of a level's final U solve: y[i] = t[i] * v[q_inv[i]] (prec_solve.hpp:411) is, for a row
// r that this band finishes, y[q[r]] = t[q[r]] * v_r -- the band writes the level's output itself and v[r], which
// nothing reads any more, not at all; k_scatter_scale_list serves the rows of the other bands and of the child.
template <class T>
struct LastU {
  IoPtr<T> out;
  int64_t ldy;
  int nrhs;
  const int32_t *q;
  const double *t;
  __device__ __forceinline__ bool on() const { return out.direct != nullptr || out.slot != nullptr; }
};

// ---------------------------------------------------------------------------------------------
// S1: w[i] = s[p[i]] * b[p[i]],  rows [0, cnt)
// ---------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(256) k_gather_scale(IoPtr<const T> bin_, int64_t ldb, int nrhs,
                                                      const int32_t *__restrict__ p,
                                                      const double *__restrict__ s, int64_t cnt,
                                                      T *__restrict__ w, int logR) {
  const T *__restrict__ bin = bin_.get();
  const LaneMap lm = lane_map(logR);
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave * lm.G + lm.g; i < cnt; i += nwaves * lm.G) {
    const int32_t src = p[i];
    T val = vzero(T());
    if (lm.c < nrhs) val = vscale(s[src], bin[(int64_t)src * ldb + lm.c]);
    w[(i << logR) + lm.c] = val;
  }
}

// ---------------------------------------------------------------------------------------------
// out[i] = in[map[i]], rows [0, n) of an arena block: the P^T x of the adjoint dense solve
// (QRCP::_solve_t, QRCP.hpp:428-433)
// ---------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(256) k_row_gather(const T *__restrict__ in, const int32_t *__restrict__ map,
                                                    int64_t n, T *__restrict__ out, int logR) {
  const LaneMap lm = lane_map(logR);
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave * lm.G + lm.g; i < n; i += nwaves * lm.G)
    out[(i << logR) + lm.c] = in[((int64_t)map[i] << logR) + lm.c];
}

// ---------------------------------------------------------------------------------------------
// S7: y[i] = t[i] * v[q_inv[i]],  rows [0, n)
// ---------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(256) k_scatter_scale(const T *__restrict__ v,
                                                       const int32_t *__restrict__ qinv,
                                                       const double *__restrict__ t, int64_t n,
                                                       IoPtr<T> yout_, int64_t ldy, int nrhs,
                                                       int logR) {
  T *__restrict__ yout = yout_.get();
  const LaneMap lm = lane_map(logR);
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave * lm.G + lm.g; i < n; i += nwaves * lm.G) {
    if (lm.c < nrhs) {
      const int64_t src = qinv[i];
      yout[i * ldy + lm.c] = vscale(t[i], v[(src << logR) + lm.c]);
    }
  }
}

// the same for a LIST of output rows (the rows a fused last U band -- LastU -- does not write itself); R = 64
template <class T>
__global__ void __launch_bounds__(256) k_scatter_scale_list(const T *__restrict__ v, const int32_t *__restrict__ qinv,
                                                            const double *__restrict__ t, const int32_t *__restrict__ list,
                                                            int64_t cnt, IoPtr<T> yout_, int64_t ldy, int nrhs) {
  T *__restrict__ yout = yout_.get();
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  // four rows per trip: the three dependent hops of a row (list -> q_inv, t -> v row) overlap across the four
  constexpr int UR = 4;
  for (int64_t k0 = wave * UR; k0 < cnt; k0 += nwaves * UR) {
    int64_t i_[UR];
    int32_t q_[UR];
    double t_[UR];
    T x_[UR];
#pragma unroll
    for (int u = 0; u < UR; ++u) i_[u] = list[min(k0 + u, cnt - 1)];
#pragma unroll
    for (int u = 0; u < UR; ++u) q_[u] = qinv[i_[u]], t_[u] = t[i_[u]];
#pragma unroll
    for (int u = 0; u < UR; ++u) x_[u] = v[((int64_t)q_[u] << 6) + min(lane, nrhs - 1)];  // (a narrow batch reads the columns it has)
#pragma unroll
    for (int u = 0; u < UR; ++u)
      if (k0 + u < cnt && lane < nrhs) yout[i_[u] * ldy + lane] = vscale(t_[u], x_[u]);
  }
}

// ---------------------------------------------------------------------------------------------
// one row of a triangular solve.  LOWER: acc = w[i] - sum_asc L(i,j) w[j]; w[i] = acc
//                                 UPPER: acc = w[i]/d[i] (first touch) or v[i]; acc -= sum_desc U(i,j) v[j]; v[i] = acc
// (the CSR row already lists its columns in the order the reference's column sweep meets them)
// ---------------------------------------------------------------------------------------------
template <class T, bool LOWER, bool PREFIX>
__device__ __forceinline__ void trsv_row(int64_t slot, const int32_t *__restrict__ ptr,
                                         const int32_t *__restrict__ split,
                                         const int32_t *__restrict__ col, const T *__restrict__ val,
                                         const int32_t *__restrict__ rowid, const T *__restrict__ d,
                                         T *w, T *v, int logR, int c, bool first_u) {
  const int64_t i = rowid[slot];
  const int32_t k0 = ptr[slot], k1 = PREFIX ? split[slot] : ptr[slot + 1];
  T *x = LOWER ? w : v;
  // U's right-hand side is D^{-1} (L^{-1} w): the kernel that touches a U row FIRST divides (prec_solve.hpp:219)
  T acc = (!LOWER && first_u) ? vdiv(w[(i << logR) + c], d[i]) : x[(i << logR) + c];
  int32_t k = k0;
  for (; k + 4 <= k1; k += 4) {  // 4 independent gathers in flight, accumulated in order
    const int32_t j0 = col[k], j1 = col[k + 1], j2 = col[k + 2], j3 = col[k + 3];
    const T a0 = val[k], a1 = val[k + 1], a2 = val[k + 2], a3 = val[k + 3];
    const T x0 = x[((int64_t)j0 << logR) + c], x1 = x[((int64_t)j1 << logR) + c];
    const T x2 = x[((int64_t)j2 << logR) + c], x3 = x[((int64_t)j3 << logR) + c];
    acc = vsub(acc, vmul(a0, x0));
    acc = vsub(acc, vmul(a1, x1));
    acc = vsub(acc, vmul(a2, x2));
    acc = vsub(acc, vmul(a3, x3));
  }
  for (; k < k1; ++k) acc = vsub(acc, vmul(val[k], x[((int64_t)col[k] << logR) + c]));
  x[(i << logR) + c] = acc;
}

// ---------------------------------------------------------------------------------------------
// R = 64 software pipeline of the level-scheduled solves: a wave owns rows s_first, s_first+stride,
// ... (slot order) and streams them as ITEMS of up to 64 nonzeros.  The 64 lanes fetch an item's
// (column, value, source-slot) triples with ONE coalesced load each and broadcast them with
// v_readlane; the NEXT item (next 64 nonzeros of the row, or the head of the wave's next row with
// its right-hand side and pivot) is always in flight while the current one is consumed, and the
// row headers run two rows ahead on the scalar unit.  Gathers go out eight 512-byte rows at a time;
// accumulation stays in the reference's order.  In place: x[i] holds the rhs on entry and the
// solution on exit.  UPPER rows start from rhs_u[i] / d[i] when this kernel is the first to touch them (first_u).
//   MODE 0: all dependencies were finished by earlier launches                   (k_trsv_wide)
//   MODE 2: dependencies with srcslot >= slot0 are acquired through LDS flags     (k_trsv_band)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t rl32(int32_t v, int idx) { return __builtin_amdgcn_readlane(v, idx); }
__device__ __forceinline__ double rl64(double v, int idx) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffLL), idx);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), idx);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double rlv(double v, int idx) { return rl64(v, idx); }
__device__ __forceinline__ cplx rlv(cplx v, int idx) { return cplx{rl64(v.x, idx), rl64(v.y, idx)}; }
__device__ __forceinline__ int32_t rfl(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }
// compiler barrier that "touches" a value: nothing that depends on it is scheduled above this point
__device__ __forceinline__ void pin_here(double &v) { asm volatile("" : "+v"(v)::"memory"); }
__device__ __forceinline__ void pin_here(cplx &v) { asm volatile("" : "+v"(v.x), "+v"(v.y)::"memory"); }
__device__ __forceinline__ void pin_here(uint32_t &v) { asm volatile("" : "+v"(v)::"memory"); }

// Development probe (make PROBE=1): wall_clock64 stamps of every wave of k_trsv_band -- kernel entry, start
// of work, exit, and per row (the wave's first two) start / first gather / last accumulation / flag, number
// of nonzeros and poll sleeps.  tests/probe_summary.py and tests/probe_rows.py read the dump
// (HIFIR_AMD_PROBE_OUT); profiles/r01_band_*_timestamps.* were made with it.  Compiled out by default.
#ifdef HIFAMD_PROBE
#define HIFAMD_PROBE_ARG , unsigned long long *tsw = nullptr
#define HIFAMD_STAMP(k) \
  if (tsw && lane == 0 && prow < 2) tsw[4 + prow * 6 + (k)] = wall_clock64();
#define HIFAMD_STAMP_VAL(k, v) \
  if (tsw && lane == 0 && prow < 2) tsw[4 + prow * 6 + (k)] = (unsigned long long)(v);
#else
#define HIFAMD_PROBE_ARG
#define HIFAMD_STAMP(k)
#define HIFAMD_STAMP_VAL(k, v)
#endif
// make PROBE=2 (-DHIFAMD_PROBE -DHIFAMD_PROBE_BATCH): instead of the per-row stamps, the wave's FIRST row records the
// timeline of its leading full batches in words 4..15 of its record: (gathers issued, accumulated) x up to six batches
#if defined(HIFAMD_PROBE) && defined(HIFAMD_PROBE_BATCH)
#undef HIFAMD_STAMP
#undef HIFAMD_STAMP_VAL
#define HIFAMD_STAMP(k)
#define HIFAMD_STAMP_VAL(k, v)
#define HIFAMD_STAMP_BATCH(e)                                                                   \
  if (tsw && lane == 0 && prow == 0 && pbatch < 6) {                                            \
    tsw[4 + 2 * pbatch + (e)] = wall_clock64();                                                 \
    pbatch += (e);                                                                              \
  }
#else
#define HIFAMD_STAMP_BATCH(e)
#endif

template <class T, int MODE, bool LOWER, bool PREFIX>
__device__ __forceinline__ bool trsv_stream_r64(int32_t s_first, int32_t s_end, int32_t stride,
                                                const int32_t *__restrict__ ptr, const int32_t *__restrict__ split,
                                                const int32_t *__restrict__ col,
                                                const T *__restrict__ val, const int32_t *__restrict__ srcslot,
                                                const int32_t *__restrict__ rowid, const T *__restrict__ d, T *x,
                                                const T *__restrict__ rhs_u, int lane, int *flag, int32_t slot0,
                                                unsigned *errflag, bool first_u, T *tb = nullptr, int32_t tb_s0 = 0,
                                                int32_t tb_s1 = 0, const T *fl_bin = nullptr,
                                                const FirstL<T> *fl = nullptr HIFAMD_PROBE_ARG) {
  int32_t s = rfl(s_first);
  if (s >= s_end) return true;
  const bool first_l = LOWER && fl_bin != nullptr;  // this kernel is the first to touch its L rows: S1 fused (FirstL)
#ifdef HIFAMD_PROBE
  int prow = 0;
  bool pfirst = false;
#endif
  // nonzero range of a row: the whole row, its PREFIX [ptr, split) (dependencies finished before the
  // thin run started; exact partial sum, no division yet) or, in a thin run, the rest [split, end)
#define HIFAMD_KBEG(sl) rfl((MODE == 2) ? split[sl] : ptr[sl])
#define HIFAMD_KEND(sl) rfl(PREFIX ? split[sl] : ptr[(sl) + 1])
  int32_t i_c = rfl(rowid[s]), k_c = HIFAMD_KBEG(s), e_c = HIFAMD_KEND(s);
  int32_t s_n = s + stride;
  bool has_n = s_n < s_end;
  int32_t i_n = 0, k_n = 0, e_n = 0;
  if (has_n) {
    i_n = rfl(rowid[s_n]);
    k_n = HIFAMD_KBEG(s_n);
    e_n = HIFAMD_KEND(s_n);
  }
  int32_t colv = 0, ssv = 0;
  T valv = vzero(T());
  {
    const int32_t kk = k_c + lane;
    if (kk < e_c) {
      colv = col[kk];
      valv = val[kk];
      if (MODE == 2) ssv = srcslot[kk];
    }
  }
  // U rows start from D^{-1} times the L solution (rhs_u = w) when this kernel is the first to touch them
  const bool div_u = !LOWER && first_u;
  T acc = div_u ? vdiv(rhs_u[((int64_t)i_c << 6) + lane], d[i_c])
                : (first_l ? first_l_rhs(fl_bin, *fl, i_c, lane) : x[((int64_t)i_c << 6) + lane]);
  // head of the wave's next row: its first item, right-hand side, pivot, and the header two rows
  // ahead.  MODE 0 issues it while the current row is consumed; MODE 2 only AFTER the current row's
  // flag is up, because a workgroup-scope release waits for every outstanding vector-memory
  // operation of the wave (vmcnt(0)) and these cold loads would sit on the dependency chain.
#define HIFAMD_PREFETCH_NEXT_ROW()                          \
  do {                                                      \
    const int32_t kk_ = k_n + lane;                         \
    if (kk_ < e_n) {                                        \
      colv2 = col[kk_];                                     \
      valv2 = val[kk_];                                     \
      if (MODE == 2) ssv2 = srcslot[kk_];                   \
    }                                                       \
    acc2 = div_u ? vdiv(rhs_u[((int64_t)i_n << 6) + lane], d[i_n])                                  \
                 : (first_l ? first_l_rhs(fl_bin, *fl, i_n, lane) : x[((int64_t)i_n << 6) + lane]); \
    s_nn = s_n + stride;                                    \
    has_nn = s_nn < s_end;                                  \
    if (has_nn) {                                           \
      i_nn = rfl(rowid[s_nn]);                              \
      k_nn = HIFAMD_KBEG(s_nn);                             \
      e_nn = HIFAMD_KEND(s_nn);                             \
    }                                                       \
  } while (0)
  for (;;) {
    const int32_t cnt = min(64, e_c - k_c);  // <= 0 for an empty row
    const bool row_done = (k_c + 64 >= e_c);
    // ---- prefetch the next item (and, at a row end, the header two rows ahead)
    int32_t colv2 = 0, ssv2 = 0;
    T valv2 = vzero(T()), acc2 = vzero(T());
    int32_t s_nn = 0, i_nn = 0, k_nn = 0, e_nn = 0;
    bool has_nn = false;
    if (!row_done) {
      const int32_t kk = k_c + 64 + lane;
      if (kk < e_c) {
        colv2 = col[kk];
        valv2 = val[kk];
        if (MODE == 2) ssv2 = srcslot[kk];
      }
    } else if (has_n && MODE != 2) {
      HIFAMD_PREFETCH_NEXT_ROW();
    }
    // ---- consume the current item in order.  MODE 2: the item's source slots sit one per lane, so
    // ONE LDS instruction polls the flags of all its in-run dependencies; the ready prefix of the
    // item is consumed (eight gathers per batch) and only then is the rest polled again.
    int32_t t = 0;
    unsigned spins = 0;
#ifdef HIFAMD_PROBE
    if (k_c == HIFAMD_KBEG(s)) {
      HIFAMD_STAMP(0)
      HIFAMD_STAMP_VAL(4, e_c - k_c)
      pfirst = false;
    }
#endif
    while (t < cnt) {
      int32_t lim = cnt;
      if (MODE == 2) {
        const bool inrun = lane >= t && lane < cnt && ssv >= slot0;
        bool rdy = true;
        if (inrun) rdy = __hip_atomic_load(&flag[ssv - slot0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != 0;
        const unsigned long long pending = ~__ballot(rdy);
        if (pending) lim = min(cnt, (int32_t)__builtin_ctzll(pending));
        if (lim <= t) {
          __builtin_amdgcn_s_sleep(1);
          if ((++spins & 4095u) == 0 && spins > (1u << 24)) {
            if (lane == 0) __hip_atomic_store(errflag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
          }
          continue;
        }
      }
#ifdef HIFAMD_PROBE
      if (!pfirst) {
        HIFAMD_STAMP(1)
        pfirst = true;
      }
#endif
      while (t < lim) {
        const int nb = min(8, lim - t);
        int32_t j[8];
        T a[8], xv[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          const int idx = min(t + b, 63);
          j[b] = rl32(colv, idx);
          a[b] = rlv(valv, idx);
        }
#pragma unroll
        for (int b = 0; b < 8; ++b)
          if (b < nb) xv[b] = x[((int64_t)j[b] << 6) + lane];
#pragma unroll
        for (int b = 0; b < 8; ++b)
          if (b < nb) acc = vsub(acc, vmul(a[b], xv[b]));
        t += nb;
      }
    }
    if (row_done) {
      HIFAMD_STAMP(2)
      // PREFIX pass of a block-dense band: the rows of the band's FIRST block have no other contribution
      // before their block product, so their partial sums go straight into the product's right-hand side
      // (saves that block's k_thin_update launch)
      if (PREFIX && tb && s < tb_s1)
        tb[((int64_t)(s - tb_s0) << 6) + lane] = acc;
      else
        x[((int64_t)i_c << 6) + lane] = acc;
      if (MODE == 2) {  // release: the row's stores (all 64 lanes) are complete before its flag goes up
        if (lane == 0) __hip_atomic_store(&flag[s - slot0], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
#ifdef HIFAMD_PROBE
      HIFAMD_STAMP(3)
      HIFAMD_STAMP_VAL(5, spins)
      ++prow;
#endif
      if (!has_n) break;
      if (MODE == 2) HIFAMD_PREFETCH_NEXT_ROW();
      s = s_n;
      i_c = i_n;
      k_c = k_n;
      e_c = e_n;
      acc = acc2;
      s_n = s_nn;
      has_n = has_nn;
      i_n = i_nn;
      k_n = k_nn;
      e_n = e_nn;
    } else {
      k_c += 64;
    }
    colv = colv2;
    valv = valv2;
    ssv = ssv2;
  }
  return true;
}

// wide wavefront: slots [s0, s1) are mutually independent -> any number of workgroups
template <class T, bool LOWER, bool PREFIX>
__global__ void __launch_bounds__(256) k_trsv_wide(int64_t s0, int64_t s1, const int32_t *__restrict__ ptr,
                                                   const int32_t *__restrict__ split,
                                                   const int32_t *__restrict__ col,
                                                   const T *__restrict__ val,
                                                   const int32_t *__restrict__ rowid,
                                                   const T *__restrict__ d, T *w, T *v, int logR, int first_u,
                                                   T *tb, int32_t tb_s1, FirstL<T> fl) {
  const LaneMap lm = lane_map(logR);
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  if (logR == 6) {  // (tb: R = 64 only; rows [s0, tb_s1) deliver their result to tb, see trsv_stream_r64)
    const T *fl_bin = (LOWER && fl.on()) ? fl.bin.get() : nullptr;
    trsv_stream_r64<T, 0, LOWER, PREFIX>((int32_t)(s0 + wave), (int32_t)s1, (int32_t)nwaves, ptr, split, col, val,
                                         nullptr, rowid, d, LOWER ? w : v, w, threadIdx.x & 63, nullptr, 0, nullptr,
                                         first_u != 0, tb, (int32_t)s0, tb_s1, fl_bin, &fl);
    return;
  }
  for (int64_t slot = s0 + wave * lm.G + lm.g; slot < s1; slot += nwaves * lm.G)
    trsv_row<T, LOWER, PREFIX>(slot, ptr, split, col, val, rowid, d, w, v, logR, lm.c, first_u != 0);
}

// ---------------------------------------------------------------------------------------------
// One BAND of a triangle (host.hpp BandPlan): workgroup wg0 + blockIdx.x owns the slot range of its
// groups, i.e. a set of whole connected components of the band's dependency graph.  Dependencies on
// rows before the band were finished by earlier launches (plain loads); dependencies inside the
// workgroup's own range are handed over through one LDS flag per row with workgroup-scope
// release/acquire (all waves share this CU's L1/L2 path).  No workgroup ever waits for another
// one, so any number of them may run in any order.  In place: x[i] holds the rhs on entry and the
// solution on exit (LOWER also writes v[i] = x[i] / d[i]).
// R = 64: rows are dealt round-robin over the 16 waves in SLOT order (a row only waits for smaller
// slots of the same workgroup, so this cannot deadlock) and streamed through trsv_stream_r64.
// R < 64: a wave takes G = 64/R rows of ONE group (same depth, hence independent) at a time.
// If the band had a PREFIX pass (k_trsv_wide<.., true>), rows start at split[slot].
// ---------------------------------------------------------------------------------------------
#define HIFAMD_TAIL_MAX 16384
template <class T, bool LOWER>
__global__ void __launch_bounds__(1024) k_trsv_band(int32_t wg0, const int32_t *__restrict__ wg_grp_ptr,
                                                    const int32_t *__restrict__ grp_slot_ptr,
                                                    const int32_t *__restrict__ ptr,
                                                    const int32_t *__restrict__ split,
                                                    const int32_t *__restrict__ col, const T *__restrict__ val,
                                                    const int32_t *__restrict__ srcslot,
                                                    const int32_t *__restrict__ rowid, const T *__restrict__ d,
                                                    T *w, T *v, int logR, unsigned *errflag, int first_u
#ifdef HIFAMD_PROBE
                                                    ,
                                                    unsigned long long *ts, int probe_id
#endif
) {
  __shared__ int flag[HIFAMD_TAIL_MAX];
  const LaneMap lm = lane_map(logR);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#ifdef HIFAMD_PROBE  // [launch][workgroup < 256][wave][16]: 0 entry, 2 start of work, 3 exit, 4.. two rows x 6
  unsigned long long *tsw =
      (ts && blockIdx.x < 256) ? ts + (((size_t)probe_id * 256 + blockIdx.x) * 16 + wave) * 16 : nullptr;
  if (tsw && lane == 0) tsw[0] = wall_clock64();
#endif
  const int32_t wf0 = wg_grp_ptr[wg0 + blockIdx.x], wf1 = wg_grp_ptr[wg0 + blockIdx.x + 1];
  const int32_t *wfptr = grp_slot_ptr;
  const int32_t slot0 = wfptr[wf0], slot1 = wfptr[wf1];
  for (int t = threadIdx.x; t < slot1 - slot0; t += blockDim.x) flag[t] = 0;
  __syncthreads();
  T *x = LOWER ? w : v;
  if (logR == 6) {
#ifdef HIFAMD_PROBE
    if (tsw && lane == 0) tsw[2] = wall_clock64();
    trsv_stream_r64<T, 2, LOWER, false>(slot0 + wave, slot1, nw, ptr, split, col, val, srcslot, rowid, d, x, w, lane,
                                        flag, slot0, errflag, first_u != 0, nullptr, 0, 0, tsw);
    if (tsw && lane == 0) tsw[3] = wall_clock64();
#else
    trsv_stream_r64<T, 2, LOWER, false>(slot0 + wave, slot1, nw, ptr, split, col, val, srcslot, rowid, d, x, w, lane,
                                        flag, slot0, errflag, first_u != 0);
#endif
    return;
  }
  for (int32_t wf = wf0; wf < wf1; ++wf) {
    const int32_t s0 = wfptr[wf], s1 = wfptr[wf + 1];
    for (int32_t base = s0 + wave * lm.G; base < s1; base += nw * lm.G) {
      const int32_t slot = base + lm.g;
      const bool active = slot < s1;
      int64_t i = 0;
      int32_t k = 0, k1 = 0;
      T acc = vzero(T());
      if (active) {
        i = rowid[slot];
        k = split[slot];  // [ptr, split) was folded in by the prefix pass
        k1 = ptr[slot + 1];
        acc = (!LOWER && first_u) ? vdiv(w[(i << logR) + lm.c], d[i]) : x[(i << logR) + lm.c];
      }
      while (__any(k < k1)) {
        const int nb = min(4, k1 - k);
        int32_t j[4], ss[4];
        T a[4], xv[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          j[b] = 0;
          ss[b] = -1;
          a[b] = vzero(T());
          if (b < nb) {
            j[b] = col[k + b];
            a[b] = val[k + b];
            ss[b] = srcslot[k + b];
          }
        }
        unsigned spins = 0;
        for (;;) {  // acquire every in-run dependency of this batch (rows of earlier wavefronts only)
          bool ok = true;
#pragma unroll
          for (int b = 0; b < 4; ++b)
            if (b < nb && ss[b] >= slot0)
              ok = ok && (__hip_atomic_load(&flag[ss[b] - slot0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != 0);
          if (__all(ok)) break;
          __builtin_amdgcn_s_sleep(1);
          if ((++spins & 4095u) == 0 && spins > (1u << 24)) {
            if (lane == 0) __hip_atomic_store(errflag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
          }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (b < nb) xv[b] = x[((int64_t)j[b] << logR) + lm.c];
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (b < nb) acc = vsub(acc, vmul(a[b], xv[b]));
        if (nb > 0) k += nb;
      }
      if (active) {
        x[(i << logR) + lm.c] = acc;
      }
      // release: every lane's stores are complete before the row's flag goes up
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (active && lm.c == 0)
        __hip_atomic_store(&flag[slot - slot0], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The band form of the R = 64 pipeline (k_trsv_band_p, the default at R = 64): dependencies with srcslot >= slot0 are
// acquired through LDS flags.  Per row and wave the first version (trsv_stream_r64 MODE 2, still selectable with
// HIFIR_AMD_BAND_PIPE=0) pays two serial memory round trips -- the row's gathers, then, behind the row's flag, the head
// of the wave's next row -- plus scalar-memory waits for the row headers.  This version overlaps them:
//  * row headers (row id, nonzero range, pivot) of the wave's next 64 rows sit one per lane in registers (one vector
//    load per array and 64 rows, the following block is requested half a block ahead) and are broadcast with
//    v_readlane: no scalar-memory wait inside the loop;
//  * the head of the wave's NEXT row (first item, right-hand side) goes out right BEHIND the last gathers of the
//    current row.  Loads return in order: issued in front of the gathers these cold loads would delay them and with
//    them the row's flag; issued after the flag they add a full memory round trip to every row;
//  * that last batch, the trailing loads, the accumulation, the row's store and its flag are ONE basic block of
//    straight-line code per batch size (0, 1, 2, 3, 4, 6 or 8 gathers; slots beyond the row's end read one valid word
//    that is ignored, addresses are selected instead of branched on).  The compiler then counts its waits exactly
//    (e.g. s_waitcnt vmcnt(11) ... vmcnt(4) in front of eight accumulations: only the gathers are waited for) and has
//    no block boundary at which to copy a register that a trailing load is still going to write.  The next row's
//    data is first touched behind the flag (pin_here).  The batch sizes matter: with eight gathers always, the
//    padding loads of the one- and two-nonzero rows of the wide first bands cost more gather slots of the compute
//    unit than the overlap saves (measured: 10.92 -> 11.16 ms; with the sizes above 10.04 -> 9.65 ms).
// Longer rows run their leading full batches through plain loops in front of that block.
// Accumulation order is the reference's (exact mode stays bit-exact).  In place: x[i] holds the rhs on entry, the
// solution on exit; UPPER rows start from rhs_u[i] / d[i] when this kernel is the first to touch them (first_u).
// ---------------------------------------------------------------------------------------------
template <class T, bool LOWER>
__device__ __forceinline__ bool trsv_band_r64(const int32_t s_first_, const int32_t s_end, const int32_t stride,
                                              const int32_t *__restrict__ ptr, const int32_t *__restrict__ split,
                                              const int32_t *__restrict__ col, const T *__restrict__ val,
                                              const int32_t *__restrict__ srcslot,
                                              const int32_t *__restrict__ rowid, const T *__restrict__ d, T *x,
                                              const T *__restrict__ rhs_u, const int lane, int *flag,
                                              const int32_t slot0, unsigned *errflag, const bool first_u,
                                              const T *fl_bin = nullptr, const FirstL<T> *fl = nullptr HIFAMD_PROBE_ARG) {
#ifdef HIFAMD_PROBE
  int prow = 0;
  int pbatch = 0;
  (void)pbatch;
#endif
  const int32_t s_first = rfl(s_first_);  // (wave-uniform, which the compiler cannot see from threadIdx.x >> 6)
  const bool div_u = !LOWER && first_u;
  // S1 fused (FirstL): this kernel touches its L rows first and reads rhs[i] = s[p[i]] * b[p[i]]; the row's source row
  // p[i] and scale s[p[i]] travel in the header blocks, so the loop still issues ONE right-hand-side load per row
  const bool first_l = LOWER && first_u && fl_bin != nullptr;
  const T *rhs = div_u ? rhs_u : (first_l ? fl_bin : (const T *)x);
  const int64_t rstride = first_l ? fl->ldb : 64;
  const int rlane = first_l ? min(lane, fl->nrhs - 1) : lane;
  // header blocks: lane l holds the header of the wave's row number (64 * block + l)
  int32_t h_i = 0, h_k = 0, h_e = 0, g_i = 0, g_k = 0, g_e = 0, h_p = 0, g_p = 0;
  T h_d = vzero(T()), g_d = vzero(T());
  double h_s = 0.0, g_s = 0.0;
#define HIFAMD_LOAD_HDR(hi, hk, he, hd, hp, hs, base)    \
  {                                                      \
    const int32_t sl_ = (base) + lane * stride;          \
    if (sl_ < s_end) {                                   \
      hi = rowid[sl_];                                   \
      hk = split[sl_];                                   \
      he = ptr[sl_ + 1];                                 \
      if (div_u) hd = d[hi];                             \
      if (first_l) {                                     \
        hp = fl->p[hi];                                  \
        hs = fl->s[hp];                                  \
      }                                                  \
    }                                                    \
  }
  // right-hand side of row (id i, source row pr, scale sc) as loaded / as used
#define HIFAMD_RHS_AT(i, pr) rhs[(int64_t)(first_l ? (pr) : (i)) * rstride + rlane]
#define HIFAMD_RHS_FIX(val, sc) (first_l ? (lane < fl->nrhs ? vscale((sc), (val)) : vzero(T())) : (val))
  // wait until the leading `hi` nonzeros of the current item (item_cnt of them valid) have their in-band sources
  // finished.  ONE LDS instruction polls the flags of the whole item (source slots sit one per lane) and `ready`
  // remembers how many leading nonzeros were found ready, so that a row whose sources all finished before the
  // band -- phase 1 of every band -- polls once, not once per batch.
#define HIFAMD_BAND_POLL(hi)                                                                                      \
  if (ready < (hi)) {                                                                                             \
    unsigned spins_ = 0;                                                                                          \
    for (;;) {                                                                                                    \
      bool rdy_ = true;                                                                                           \
      if (lane < item_cnt && ssv >= slot0)                                                                        \
        rdy_ = __hip_atomic_load(&flag[ssv - slot0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != 0;        \
      const unsigned long long pend_ = ~__ballot(rdy_);                                                           \
      ready = pend_ ? (int32_t)__builtin_ctzll(pend_) : 64;                                                       \
      if (ready >= (hi)) break;                                                                                   \
      __builtin_amdgcn_s_sleep(1);                                                                                \
      if ((++spins_ & 4095u) == 0 && spins_ > (1u << 24)) {                                                       \
        if (lane == 0) __hip_atomic_store(errflag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);               \
        return false;                                                                                             \
      }                                                                                                           \
    }                                                                                                             \
  }
  // a full batch of eight nonzeros starting at lane t of the current item (plain: leading part of longer rows)
#define HIFAMD_BAND_FULL8(t)                                                                 \
  {                                                                                          \
    int32_t j_[8];                                                                           \
    T a_[8], xv_[8];                                                                         \
    _Pragma("unroll") for (int b = 0; b < 8; ++b) {                                          \
      j_[b] = rl32(colv, (t) + b);                                                           \
      a_[b] = rlv(valv, (t) + b);                                                            \
    }                                                                                        \
    _Pragma("unroll") for (int b = 0; b < 8; ++b) xv_[b] = x[((int64_t)j_[b] << 6) + lane];  \
    HIFAMD_STAMP_BATCH(0) /* (all eight gathers issued) */                                   \
    _Pragma("unroll") for (int b = 0; b < 8; ++b) acc = vsub(acc, vmul(a_[b], xv_[b]));      \
    HIFAMD_STAMP_BATCH(1) /* (all eight accumulated) */                                      \
  }
  HIFAMD_LOAD_HDR(h_i, h_k, h_e, h_d, h_p, h_s, s_first)  // (requested first: in flight while the flags are cleared)
  // the workgroup's flags: one per slot of its range [slot0, s_end)
  for (int t_ = (int)threadIdx.x; t_ < s_end - slot0; t_ += (int)blockDim.x) flag[t_] = 0;
  __syncthreads();
  if (s_first >= s_end) return true;
  int hidx = 0;
  int32_t s = s_first;
  int32_t i_c = rl32(h_i, 0), k_c = rl32(h_k, 0), e_c = rl32(h_e, 0);
  int32_t colv = col[k_c + lane], ssv = srcslot[k_c + lane];  // (80 padding elements: DevCsr::upload)
  T valv = val[k_c + lane];
  T acc = HIFAMD_RHS_AT(i_c, rl32(h_p, 0));
  acc = HIFAMD_RHS_FIX(acc, rl64(h_s, 0));
  if (div_u) acc = vdiv(acc, rlv(h_d, 0));
  for (;;) {  // one row per iteration
    // header of the wave's next row: registers only.  Without a next row the trailing loads re-read
    // the current row (valid, ignored).
    const int32_t s_n = s + stride;
    const bool has_n = s_n < s_end;
    int32_t i_n = i_c, k_n = k_c, e_n = e_c, p_n = rl32(h_p, hidx);
    T d_n = vzero(T());
    double s_n2 = rl64(h_s, hidx);
    if (has_n) {
      if (hidx < 63) {
        i_n = rl32(h_i, hidx + 1);
        k_n = rl32(h_k, hidx + 1);
        e_n = rl32(h_e, hidx + 1);
        if (div_u) d_n = rlv(h_d, hidx + 1);
        if (first_l) p_n = rl32(h_p, hidx + 1), s_n2 = rl64(h_s, hidx + 1);
      } else {
        i_n = rl32(g_i, 0);
        k_n = rl32(g_k, 0);
        e_n = rl32(g_e, 0);
        if (div_u) d_n = rlv(g_d, 0);
        if (first_l) p_n = rl32(g_p, 0), s_n2 = rl64(g_s, 0);
      }
    }
    // the following header block is requested half a block ahead
    if (hidx == 32 && s + 32 * stride < s_end) HIFAMD_LOAD_HDR(g_i, g_k, g_e, g_d, g_p, g_s, s + 32 * stride)
    // ---- long rows: full 64-nonzero items in front of the row's last item
    while (e_c - k_c > 64) {
      const int32_t c2 = col[k_c + 64 + lane], s2 = srcslot[k_c + 64 + lane];
      const T v2 = val[k_c + 64 + lane];
      {
        const int32_t item_cnt = 64;
        int32_t ready = 0;
        for (int t = 0; t < 64; t += 8) {
          HIFAMD_BAND_POLL(t + 8)
          HIFAMD_BAND_FULL8(t)
        }
      }
      colv = c2;
      valv = v2;
      ssv = s2;
      k_c += 64;
    }
    // ---- the row's last item: leading full batches ...
    const int32_t cnt = e_c - k_c;  // <= 64, <= 0 for a row without nonzeros in this band
    const int32_t item_cnt = cnt;
    int32_t ready = 0, t = 0;
    HIFAMD_STAMP(0)
    HIFAMD_STAMP_VAL(4, cnt)
    while (cnt - t > 8) {
      HIFAMD_BAND_POLL(t + 8)
      HIFAMD_BAND_FULL8(t)
      t += 8;
    }
    // ---- ... and the last batch (0..8 nonzeros) with everything behind it, one basic block per batch size
    // (1, 2, 4 or 8 gathers issued: the rows of the wide first bands have one or two nonzeros, and every padding
    // load costs a slot of the compute unit's gather rate)
    const int nb = max(cnt - t, 0);
    HIFAMD_STAMP(1)  // (leading batches done)
    HIFAMD_BAND_POLL(t + nb)
    HIFAMD_STAMP(2)  // (the last batch's sources are finished)
    {
      const T *xrow = x + lane;
      const T *xdummy = x + ((int64_t)i_c << 6);  // one valid word for the slots beyond nb
#define HIFAMD_BAND_FINAL(NBT)                                                                            \
  {                                                                                                       \
    const T *pj[NBT ? NBT : 1];                                                                           \
    T a[NBT ? NBT : 1], xv[NBT ? NBT : 1];                                                                                    \
    _Pragma("unroll") for (int b = 0; b < NBT; ++b) {                                                     \
      const int idx = min(t + b, 63);                                                                     \
      const int32_t jb = rl32(colv, idx);                                                                 \
      a[b] = rlv(valv, idx);                                                                              \
      pj[b] = (b < nb) ? xrow + ((int64_t)jb << 6) : xdummy;                                              \
    }                                                                                                     \
    _Pragma("unroll") for (int b = 0; b < NBT; ++b) xv[b] = *pj[b];                                       \
    colv = col[k_n + lane];                                                                               \
    valv = val[k_n + lane];                                                                               \
    ssv = srcslot[k_n + lane];                                                                            \
    T acc2 = HIFAMD_RHS_AT(i_n, p_n);                                                                     \
    asm volatile("" ::: "memory"); /* pins the trailing loads HERE */                                     \
    _Pragma("unroll") for (int b = 0; b < NBT; ++b) {                                                     \
      const T pr = vmul(a[b], xv[b]);                                                                     \
      if (b < nb) acc = vsub(acc, pr);                                                                    \
    }                                                                                                     \
    x[((int64_t)i_c << 6) + lane] = acc;                                                                  \
    /* release: the row's stores (all 64 lanes) are ordered before its flag */                            \
    if (lane == 0) __hip_atomic_store(&flag[s - slot0], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); \
    pin_here(acc2); /* the next row's data is first touched HERE, behind the flag */                      \
    acc = div_u ? vdiv(acc2, d_n) : HIFAMD_RHS_FIX(acc2, s_n2);                                           \
  }
      if (nb <= 0)
        HIFAMD_BAND_FINAL(0)
      else if (nb <= 1)
        HIFAMD_BAND_FINAL(1)
      else if (nb <= 2)
        HIFAMD_BAND_FINAL(2)
      else if (nb <= 3)
        HIFAMD_BAND_FINAL(3)
      else if (nb <= 4)
        HIFAMD_BAND_FINAL(4)
      else if (nb <= 6)
        HIFAMD_BAND_FINAL(6)
      else
        HIFAMD_BAND_FINAL(8)
#undef HIFAMD_BAND_FINAL
    }
    HIFAMD_STAMP(3)  // (row stored, flag raised, next row's head has arrived)
#ifdef HIFAMD_PROBE
    ++prow;
#endif
    if (!has_n) break;
    s = s_n;
    i_c = i_n;
    k_c = k_n;
    e_c = e_n;
    if (++hidx == 64) {
      hidx = 0;
      h_i = g_i;
      h_k = g_k;
      h_e = g_e;
      h_d = g_d;
      h_p = g_p;
      h_s = g_s;
    }
  }
#undef HIFAMD_LOAD_HDR
#undef HIFAMD_RHS_AT
#undef HIFAMD_RHS_FIX
#undef HIFAMD_BAND_POLL
#undef HIFAMD_BAND_FULL8
  return true;
}

template <class T, bool LOWER>
__global__ void __launch_bounds__(1024) k_trsv_band_p(int32_t wg0, const int32_t *__restrict__ wg_slot,
                                                      const int32_t *__restrict__ ptr,
                                                      const int32_t *__restrict__ split,
                                                      const int32_t *__restrict__ col, const T *__restrict__ val,
                                                      const int32_t *__restrict__ srcslot,
                                                      const int32_t *__restrict__ rowid, const T *__restrict__ d,
                                                      T *w, T *v, unsigned *errflag, int first_u, int32_t n_band,
                                                      int32_t ps0, int32_t ps1, FirstL<T> fl
#ifdef HIFAMD_PROBE
                                                      ,
                                                      unsigned long long *ts, int probe_id
#endif
) {
  __shared__ int flag[HIFAMD_TAIL_MAX];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  // workgroups beyond the band's own: the carried prefix of the NEXT band, slots [ps0, ps1), over the sources older than
  // this band (host.hpp finish_band_plan) -- independent of everything this launch computes, on otherwise idle units
  const T *fl_bin = (LOWER && fl.on()) ? fl.bin.get() : nullptr;
  if ((int32_t)blockIdx.x >= n_band) {
    const int32_t pw = __builtin_amdgcn_readfirstlane(((int32_t)blockIdx.x - n_band) * nw + wave);
    trsv_stream_r64<T, 0, LOWER, true>(ps0 + pw, ps1, ((int32_t)gridDim.x - n_band) * nw, ptr, split, col, val, nullptr, rowid,
                                       d, LOWER ? w : v, w, lane, nullptr, 0, nullptr, true, nullptr, 0, 0, fl_bin, &fl);
    return;
  }
#ifdef HIFAMD_PROBE  // same record layout as k_trsv_band: 0 entry, 2 start of work, 3 exit, 4.. two rows x 6
  unsigned long long *tsw =
      (ts && blockIdx.x < 256) ? ts + (((size_t)probe_id * 256 + blockIdx.x) * 16 + wave) * 16 : nullptr;
  if (tsw && lane == 0) tsw[0] = tsw[2] = wall_clock64();
#endif
  // the workgroup's slot range in ONE load level (wg_slot[g] = grp_slot_ptr[wg_grp_ptr[g]])
  const int32_t slot0 = wg_slot[wg0 + blockIdx.x], slot1 = wg_slot[wg0 + blockIdx.x + 1];
#ifdef HIFAMD_PROBE
  trsv_band_r64<T, LOWER>(slot0 + wave, slot1, nw, ptr, split, col, val, srcslot, rowid, d, LOWER ? w : v, w, lane, flag,
                          slot0, errflag, first_u != 0, fl_bin, &fl, tsw);
  if (tsw && lane == 0) tsw[3] = wall_clock64();
#else
  trsv_band_r64<T, LOWER>(slot0 + wave, slot1, nw, ptr, split, col, val, srcslot, rowid, d, LOWER ? w : v, w, lane, flag,
                          slot0, errflag, first_u != 0, fl_bin, &fl);
#endif
}

// ---------------------------------------------------------------------------------------------
// Block-dense thin bands (host.hpp build_dense_blocks), step (1) for the block of slots [r0, r1):
//   t[s - r0] = x[row(s)] - sum over the row's nonzeros in [split, end) whose source slot lies
//               BEFORE the block (rows before the band or in earlier blocks: all finished).
// Step (2) is k_dense_gemm with the block's explicit inverse.  One row per wave group.
// ---------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(256) k_thin_update(int32_t r0, int32_t r1, const int32_t *__restrict__ ptr,
                                                     const int32_t *__restrict__ split,
                                                     const int32_t *__restrict__ col, const T *__restrict__ val,
                                                     const int32_t *__restrict__ srcslot,
                                                     const int32_t *__restrict__ rowid, const T *__restrict__ x,
                                                     T *__restrict__ tbuf, int logR) {
  const LaneMap lm = lane_map(logR);
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t s = r0 + wave * lm.G + lm.g; s < r1; s += nwaves * lm.G) {
    const int64_t i = rowid[s];
    const int32_t k0 = split[s], k1 = ptr[s + 1];
    T acc = x[(i << logR) + lm.c];
    int32_t k = k0;
    for (; k + 4 <= k1; k += 4) {
      const int32_t j0 = col[k], j1 = col[k + 1], j2 = col[k + 2], j3 = col[k + 3];
      const int32_t q0 = srcslot[k], q1 = srcslot[k + 1], q2 = srcslot[k + 2], q3 = srcslot[k + 3];
      const T a0 = val[k], a1 = val[k + 1], a2 = val[k + 2], a3 = val[k + 3];
      const T x0 = x[((int64_t)j0 << logR) + lm.c], x1 = x[((int64_t)j1 << logR) + lm.c];
      const T x2 = x[((int64_t)j2 << logR) + lm.c], x3 = x[((int64_t)j3 << logR) + lm.c];
      if (q0 < r0) acc = vsub(acc, vmul(a0, x0));
      if (q1 < r0) acc = vsub(acc, vmul(a1, x1));
      if (q2 < r0) acc = vsub(acc, vmul(a2, x2));
      if (q3 < r0) acc = vsub(acc, vmul(a3, x3));
    }
    for (; k < k1; ++k)
      if (srcslot[k] < r0) acc = vsub(acc, vmul(val[k], x[((int64_t)col[k] << logR) + lm.c]));
    tbuf[((s - r0) << logR) + lm.c] = acc;
  }
}

// ---------------------------------------------------------------------------------------------
// R = 64 software pipeline of the Schur products (k_spmm_epi): a wave owns rows row0, row0 + stride, ...
// and streams each as items of up to 64 nonzeros, exactly like trsv_stream_r64 (MODE 0): the lanes fetch
// an item's (column, value) pairs with one coalesced load each and broadcast them with v_readlane,
// gathers go out eight 512-byte rows at a time, and while an item is consumed the next one (or the first
// item, scaled right-hand side and header of the wave's next row) is already in flight.  The sum starts
// from 0.0 and runs in ascending column order; the scaled right-hand side is combined at the end, as
// y = E*work; y = s*b - y does (prec_solve.hpp:366-368, :397-399).
// ---------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ void spmm_stream_r64(int64_t row0, int64_t nrows, int64_t stride,
                                                const int32_t *__restrict__ ptr, const int32_t *__restrict__ col,
                                                const T *__restrict__ val, const T *__restrict__ x,
                                                const T *__restrict__ bin, int64_t ldb, int nrhs,
                                                const int32_t *__restrict__ p, const double *__restrict__ s,
                                                int64_t roff, T *__restrict__ out, int lane) {
  if (row0 >= nrows) return;
  int64_t i = row0;
  int32_t k_c = rfl(ptr[i]), e_c = rfl(ptr[i + 1]);
  int64_t i_n = i + stride;
  bool has_n = i_n < nrows;
  int32_t k_n = 0, e_n = 0;
  if (has_n) {
    k_n = rfl(ptr[i_n]);
    e_n = rfl(ptr[i_n + 1]);
  }
  int32_t colv = 0;
  T valv = vzero(T());
  if (k_c + lane < e_c) {
    colv = col[k_c + lane];
    valv = val[k_c + lane];
  }
  T rhs = vzero(T());
  {
    const int32_t src = rfl(p[roff + i]);
    if (lane < nrhs) rhs = vscale(s[src], bin[(int64_t)src * ldb + lane]);
  }
  T acc = vzero(T());
  for (;;) {
    const int32_t cnt = min(64, e_c - k_c);  // <= 0 for an empty row
    const bool row_done = (k_c + 64 >= e_c);
    int32_t colv2 = 0;
    T valv2 = vzero(T()), rhs2 = vzero(T());
    int64_t i_nn = 0;
    int32_t k_nn = 0, e_nn = 0;
    bool has_nn = false;
    if (!row_done) {
      const int32_t kk = k_c + 64 + lane;
      if (kk < e_c) {
        colv2 = col[kk];
        valv2 = val[kk];
      }
    } else if (has_n) {
      const int32_t kk = k_n + lane;
      if (kk < e_n) {
        colv2 = col[kk];
        valv2 = val[kk];
      }
      const int32_t src = rfl(p[roff + i_n]);
      if (lane < nrhs) rhs2 = vscale(s[src], bin[(int64_t)src * ldb + lane]);
      i_nn = i_n + stride;
      has_nn = i_nn < nrows;
      if (has_nn) {
        k_nn = rfl(ptr[i_nn]);
        e_nn = rfl(ptr[i_nn + 1]);
      }
    }
    int32_t t = 0;
    while (t < cnt) {
      const int nb = min(8, cnt - t);
      int32_t j[8];
      T a[8], xv[8];
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const int idx = min(t + b, 63);
        j[b] = rl32(colv, idx);
        a[b] = rlv(valv, idx);
      }
#pragma unroll
      for (int b = 0; b < 8; ++b)
        if (b < nb) xv[b] = x[((int64_t)j[b] << 6) + lane];
#pragma unroll
      for (int b = 0; b < 8; ++b)
        if (b < nb) acc = vadd(acc, vmul(xv[b], a[b]));
      t += nb;
    }
    if (row_done) {
      out[(i << 6) + lane] = vsub(rhs, acc);
      if (!has_n) break;
      i = i_n;
      k_c = k_n;
      e_c = e_n;
      rhs = rhs2;
      acc = vzero(T());
      i_n = i_nn;
      has_n = has_nn;
      k_n = k_nn;
      e_n = e_nn;
    } else {
      k_c += 64;
    }
    colv = colv2;
    valv = valv2;
  }
}

// ---------------------------------------------------------------------------------------------
// S3 / S5:  out[i] = s[p[roff+i]] * b[p[roff+i]] - sum_asc A(i,j) x[j],  rows [0, nrows)
// (accumulate from 0.0 in ascending column order, THEN subtract from the scaled rhs: exactly
//  y = E*work followed by y = s*b - y of prec_solve.hpp:366-368 / :397-399)
// ---------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(256) k_spmm_epi(int64_t nrows, const int32_t *__restrict__ ptr,
                                                  const int32_t *__restrict__ col,
                                                  const T *__restrict__ val, const T *__restrict__ x,
                                                  IoPtr<const T> bin_, int64_t ldb, int nrhs,
                                                  const int32_t *__restrict__ p,
                                                  const double *__restrict__ s, int64_t roff,
                                                  T *__restrict__ out, int logR) {
  const T *__restrict__ bin = bin_.get();
  const LaneMap lm = lane_map(logR);
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  if (logR == 6) {
    spmm_stream_r64<T>(__builtin_amdgcn_readfirstlane((int)wave), nrows, nwaves, ptr, col, val, x, bin, ldb, nrhs, p, s,
                       roff, out, threadIdx.x & 63);
    return;
  }
  for (int64_t i = wave * lm.G + lm.g; i < nrows; i += nwaves * lm.G) {
    const int32_t k0 = ptr[i], k1 = ptr[i + 1];
    T acc = vzero(T());
    int32_t k = k0;
    for (; k + 4 <= k1; k += 4) {
      const int32_t j0 = col[k], j1 = col[k + 1], j2 = col[k + 2], j3 = col[k + 3];
      const T a0 = val[k], a1 = val[k + 1], a2 = val[k + 2], a3 = val[k + 3];
      const T x0 = x[((int64_t)j0 << logR) + lm.c], x1 = x[((int64_t)j1 << logR) + lm.c];
      const T x2 = x[((int64_t)j2 << logR) + lm.c], x3 = x[((int64_t)j3 << logR) + lm.c];
      acc = vadd(acc, vmul(x0, a0));
      acc = vadd(acc, vmul(x1, a1));
      acc = vadd(acc, vmul(x2, a2));
      acc = vadd(acc, vmul(x3, a3));
    }
    for (; k < k1; ++k) acc = vadd(acc, vmul(x[((int64_t)col[k] << logR) + lm.c], val[k]));
    const int32_t src = p[roff + i];
    T rhs = vzero(T());
    if (lm.c < nrhs) rhs = vscale(s[src], bin[(int64_t)src * ldb + lm.c]);
    out[(i << logR) + lm.c] = vsub(rhs, acc);
  }
}

// ---------------------------------------------------------------------------------------------
// S3 / S5 for a NARROW batch in the 64-column arena (round 3): k_spmm_epi at R = 64 spends a whole wave -- and a 512-byte
// (complex: 1 KB) gather -- on every nonzero, whatever the batch width.  Here a wave is G = 64 / R row groups of R lanes
// (R = 16 or 32 >= nrhs): G rows side by side, each lane group walking ITS row's nonzeros in the reference's order
// (column and value are fetched per lane; the R lanes of a group read the same address), eight gathers of R columns in
// flight.  Arena rows stay 64 columns apart.  Same arithmetic as k_spmm_epi: a column's bits do not depend on the width.
// ---------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(256) k_spmm_epi_narrow(int64_t nrows, const int32_t *__restrict__ ptr,
                                                         const int32_t *__restrict__ col, const T *__restrict__ val,
                                                         const T *__restrict__ x, IoPtr<const T> bin_, int64_t ldb, int nrhs,
                                                         const int32_t *__restrict__ p, const double *__restrict__ s,
                                                         int64_t roff, T *__restrict__ out, int logR) {
  const T *__restrict__ bin = bin_.get();
  const LaneMap lm = lane_map(logR);
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave * lm.G + lm.g; i < nrows; i += nwaves * lm.G) {
    const int32_t k0 = ptr[i], k1 = ptr[i + 1];
    T acc = vzero(T());
    int32_t k = k0;
    for (; k + 8 <= k1; k += 8) {
      int32_t j_[8];
      T a_[8], x_[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) j_[u] = col[k + u], a_[u] = val[k + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) x_[u] = x[((int64_t)j_[u] << 6) + lm.c];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = vadd(acc, vmul(x_[u], a_[u]));
    }
    for (; k < k1; ++k) acc = vadd(acc, vmul(x[((int64_t)col[k] << 6) + lm.c], val[k]));
    const int32_t src = p[roff + i];
    T rhs = vzero(T());
    if (lm.c < nrhs) rhs = vscale(s[src], bin[(int64_t)src * ldb + lm.c]);
    out[(i << 6) + lm.c] = vsub(rhs, acc);
  }
}

// ---------------------------------------------------------------------------------------------
// S3 / S5 on the matrix cores (host.hpp SpmmTiles): out[i] = s[p[roff+i]] * b[p[roff+i]] - sum_j A(i,j) x[j] with the
// rows in blocks of 16 and each block's distinct columns in groups of 4.  One wave per block: per group ONE coalesced
// load of the 16 x 4 coefficient tile (A operand), the 4 source rows gathered as the B operands of the four
// 16-column tiles (lane l fetches x[ucol[4g + (l >> 4)]][16 ct + (l & 15)]), four MFMAs.  Two groups in flight.
// Every distinct source row of a block is fetched once, not once per nonzero.  R = 64, real data, fast mode.
// ---------------------------------------------------------------------------------------------
//
// The group loop of k_spmm_tile / k_spmm_tile4 with its requests running ahead (AHEAD; the former loop and epilogue are the
// second instance, bit 4096 of the development switch, engine.hip kDbgSpmmPlain -- the same products in the same order).
// A wave's groups k = 0 .. ng - 1 (HIFAMD_TL_GID(k): the group's number, clamped to the wave's last group; ng is
// wave-uniform) are multiplied in batches of BU, the sequence form of k_band_ct's phase 1: at the top of the step that
// multiplies batch b the ids of batch b + 1 and the gathers and coefficient tiles of batch b are in flight, in that order;
// the step requests the ids of batch b + 2, then -- the wait for the ids of b + 1 leaves batch b's operands in flight --
// the operands of batch b + 1, and only then multiplies batch b: that wait leaves everything the step requested in flight.
// Every load is unconditional; a group past the wave's last reads that group again and its coefficient is replaced by
// zero where it is multiplied (a batch wholly past the end is never multiplied).  Two register sets of each kind rotate by
// name over a loop of two steps with one exit, at its top; the remainder is multiplied behind the loop, with no requests.
// BU groups per batch: 4 for the per-wave kernel on 16-row blocks (168 registers, three waves per SIMD as before), 2 on
// 32-row blocks and for k_spmm_tile4 (116 registers, four waves per SIMD as before; 3 and 4 measured slower).
// The second bound of __launch_bounds__ (two workgroups per compute unit) keeps the accumulators in vector registers: with
// 512 registers allowed the matrix instructions take theirs in AGPRs and the loop copies every one in and out per trip.
template <int RB>
struct SpmmAhead {
  static constexpr int BU = RB == 1 ? 4 : 2;  // k_spmm_tile
  static constexpr int BU4 = 2;               // k_spmm_tile4
  static constexpr int WGS = 2;               // workgroups per compute unit the register allocation leaves room for
};
typedef __attribute__((address_space(1))) double tl_gdouble;
typedef __attribute__((address_space(1))) int32_t tl_gint32;
#define HIFAMD_TLA_IDS(ii, kb_) \
  _Pragma("unroll") for (int u = 0; u < BU; ++u) ii[u] = (uint32_t)ucol_g[4 * (int64_t)HIFAMD_TL_GID((kb_) + u) + kq];
#define HIFAMD_TLA_OPS(gg, cf, ii, kb_)                                                            \
  {                                                                                                \
    _Pragma("unroll") for (int u = 0; u < BU; ++u) {                                               \
      _Pragma("unroll") for (int rb = 0; rb < RB; ++rb)                                            \
        cf[u][rb] = coef_g[64 * (RB * (int64_t)HIFAMD_TL_GID((kb_) + u) + rb) + lane];             \
    }                                                                                              \
    __builtin_amdgcn_sched_barrier(0); /* (the tiles need no ids: they go out in front of the wait for them) */ \
    _Pragma("unroll") for (int u = 0; u < BU; ++u) {                                               \
      _Pragma("unroll") for (int ct = 0; ct < NCT; ++ct) gg[u][ct] = x_g[((uint64_t)ii[u] << 6) + (uint32_t)(16 * ct + jc)]; \
    }                                                                                              \
  }
#define HIFAMD_TLA_MUL(gg, cf, kb_)                                                                \
  _Pragma("unroll") for (int u = 0; u < BU; ++u) {                                                 \
    _Pragma("unroll") for (int rb = 0; rb < RB; ++rb) {                                            \
      const double c_ = ((kb_) + u < ng) ? cf[u][rb] : 0.0;                                        \
      _Pragma("unroll") for (int ct = 0; ct < NCT; ++ct)                                           \
        acc[rb][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(c_, gg[u][ct], acc[rb][ct], 0, 0, 0);   \
    }                                                                                              \
  }
// ifree: the id set whose gathers are out; inext: the ids of the batch behind the one being multiplied
#define HIFAMD_TLA_STEP(ifree, inext, gcur, ccur, gnew, cnew, kb_)                                 \
  {                                                                                                \
    HIFAMD_TLA_IDS(ifree, (kb_) + 2 * BU)                                                          \
    __builtin_amdgcn_sched_barrier(0); /* (the ids lead: the next step's wait for them is counted) */ \
    HIFAMD_TLA_OPS(gnew, cnew, inext, (kb_) + BU)                                                  \
    __builtin_amdgcn_sched_barrier(0); /* (the requests stay in front of the products) */          \
    HIFAMD_TLA_MUL(gcur, ccur, kb_)                                                                \
    HIFAMD_TLA_PIN_ACC                                                                             \
  }
// (the accumulators are touched behind each step's products, as in k_band_ct: without it the next step's id requests land
// behind products of this one, and the instances take four registers more -- k_spmm_tile<1,4> 172, one wave per SIMD less)
#define HIFAMD_TLA_PIN_ACC                                                                         \
  _Pragma("unroll") for (int rb = 0; rb < RB; ++rb) {                                              \
    _Pragma("unroll") for (int ct = 0; ct < NCT; ++ct) asm volatile("" : "+v"(acc[rb][ct]));       \
  }
// the epilogue's operands of row tile rb_: scales and right-hand sides of its four rows (rows and columns clamped)
#define HIFAMD_TLA_RHS(rb_)                                                                        \
  _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                  \
    sc[rb_][r] = s_g[prow[rb_][r]];                                                                \
    _Pragma("unroll") for (int ct = 0; ct < NCT; ++ct)                                             \
      bv_[rb_][r][ct] = bin_g[(int64_t)prow[rb_][r] * ldb + min(16 * ct + jc, nrhs - 1)];          \
  }

template <int RB, int NCT, bool AHEAD>
__global__ void __launch_bounds__(256, AHEAD ? SpmmAhead<RB>::WGS : 1) k_spmm_tile(int64_t nrows, int64_t nblk, const int32_t *__restrict__ blk_gptr,
                                                   const int32_t *__restrict__ ucol, const double *__restrict__ coef,
                                                   const double *__restrict__ x, IoPtr<const double> bin_, int64_t ldb,
                                                   int nrhs, const int32_t *__restrict__ p, const double *__restrict__ s,
                                                   int64_t roff, double *__restrict__ out) {
  // RB row tiles of 16 rows per block (host.hpp SpmmTiles::rb): a block's distinct columns are gathered ONCE for all of
  // them -- the product runs at the fabric's gather rate, and 32-row blocks gather a quarter less than 16-row blocks.
  // NCT: 16-column tiles of the batch in use (round 4: a batch of <= 16 columns gathers 128 of a source row's 512 bytes
  // and multiplies one tile per group; per column the arithmetic is the same whatever NCT: same bits at every width)
  const double *__restrict__ bin = bin_.get();
  const int lane = threadIdx.x & 63;
  const int kq = lane >> 4, jc = lane & 15;
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t b = wave; b < nblk; b += nwaves) {
    const int32_t g0 = rfl(blk_gptr[b]), g1 = rfl(blk_gptr[b + 1]);
    v4f64 acc[RB][NCT];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc[rb][ct] = v4f64{0.0, 0.0, 0.0, 0.0};
    if constexpr (AHEAD) {
      constexpr int BU = SpmmAhead<RB>::BU;
      const tl_gdouble *x_g = (const tl_gdouble *)x, *coef_g = (const tl_gdouble *)coef, *bin_g = (const tl_gdouble *)bin;
      const tl_gdouble *s_g = (const tl_gdouble *)s;
      const tl_gint32 *ucol_g = (const tl_gint32 *)ucol, *p_g = (const tl_gint32 *)p;
      // The epilogue's operands do not depend on the product: the rows' places in the level's input are requested when the
      // block opens, their scales and right-hand sides behind the loop, in front of the last batch's products (rows and
      // columns clamped, zero selected at the use) -- not 4 RB (1 + NCT) serial round trips behind the last product.
      uint32_t prow[RB][4];
      double sc[RB][4], bv_[RB][4][NCT];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t i = 16 * (RB * b + rb) + kq + 4 * r;
          prow[rb][r] = (uint32_t)p_g[roff + (i < nrows ? i : nrows - 1)];
        }
      const int32_t ng = g1 - g0;
      if (ng > 0) {
#define HIFAMD_TL_GID(k) (g0 + min((k), ng - 1))
        uint32_t ia[BU], ib[BU];  // (row ids are not negative: widened by zero, nothing waits for the load that early)
        double ca[BU][RB], cb[BU][RB], ga[BU][NCT], gb[BU][NCT];
        HIFAMD_TLA_IDS(ia, 0)
        HIFAMD_TLA_IDS(ib, BU)
        // (the second id set is touched here, or its request sinks into the loop's entry, behind batch 0's operands)
#pragma unroll
        for (int u = 0; u < BU; ++u) pin_here(ib[u]);
        HIFAMD_TLA_OPS(ga, ca, ia, 0)
        int32_t k = 0;
        for (; k + BU < ng; k += 2 * BU) {  // (one exit, at the top; two batches per trip)
          HIFAMD_TLA_STEP(ia, ib, ga, ca, gb, cb, k)
          HIFAMD_TLA_STEP(ib, ia, gb, cb, ga, ca, k + BU)
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) { HIFAMD_TLA_RHS(rb) }
        __builtin_amdgcn_sched_barrier(0);  // (these requests stand in front of the last batch's products)
        if (k < ng) {  // the block's last batch: in registers or on its way
          HIFAMD_TLA_MUL(ga, ca, k)
        }
#undef HIFAMD_TL_GID
      } else {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) { HIFAMD_TLA_RHS(rb) }
      }
      // epilogue: C layout col = l & 15, row = (l >> 4) + 4 * reg; only the stores depend on the row
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t i = 16 * (RB * b + rb) + kq + 4 * r;
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) {
            const int c = 16 * ct + jc;
            const double rhs = c < nrhs ? sc[rb][r] * bv_[rb][r][ct] : 0.0;
            if (i < nrows) out[(i << 6) + c] = rhs - acc[rb][ct][r];
          }
        }
      continue;
    }
    // The former software pipeline over the groups, all loads unconditional (indices clamped to the block's last group,
    // whose coefficient is then zeroed): source-row indices 7 groups ahead, coefficient + B fragments 3 groups ahead of the
    // MFMAs in the source; the compiler clusters them per trip of eight groups.
    if (g0 < g1) {
      const int32_t gl = g1 - 1;
      int32_t src[8];
      double av[4][RB], bv[4][NCT];
#define HIFAMD_TL_SRC(slot, g) src[slot] = ucol[4 * (int64_t)min((g), gl) + kq];
#define HIFAMD_TL_LOAD(slot, sslot, g)                                                                               \
  _Pragma("unroll") for (int rb = 0; rb < RB; ++rb) av[slot][rb] = coef[64 * (RB * (int64_t)min((g), gl) + rb) + lane]; \
  _Pragma("unroll") for (int ct = 0; ct < NCT; ++ct) bv[slot][ct] = x[((int64_t)src[sslot] << 6) + 16 * ct + jc];
#pragma unroll
      for (int q = 0; q < 7; ++q) { HIFAMD_TL_SRC(q, g0 + q) }
#pragma unroll
      for (int q = 0; q < 3; ++q) { HIFAMD_TL_LOAD(q, q, g0 + q) }
      for (int32_t g = g0; g < g1; g += 8) {
#pragma unroll
        for (int dd = 0; dd < 8; ++dd) {
          const int32_t cur = g + dd;
          HIFAMD_TL_LOAD((dd + 3) & 3, (dd + 3) & 7, cur + 3)
          HIFAMD_TL_SRC((dd + 7) & 7, cur + 7)
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) {
            const double am = cur < g1 ? av[dd & 3][rb] : 0.0;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[rb][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(am, bv[dd & 3][ct], acc[rb][ct], 0, 0, 0);
          }
        }
      }
#undef HIFAMD_TL_SRC
#undef HIFAMD_TL_LOAD
    }
    // epilogue: C layout col = l & 15, row = (l >> 4) + 4 * reg
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i = 16 * (RB * b + rb) + kq + 4 * r;
        if (i < nrows) {
          const int32_t srow = p[roff + i];
          const double sc = s[srow];
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) {
            const int c = 16 * ct + jc;
            const double rhs = c < nrhs ? sc * bin[(int64_t)srow * ldb + c] : 0.0;
            out[(i << 6) + c] = rhs - acc[rb][ct][r];
          }
        }
      }
  }
}

// The same product with ONE block per workgroup, its column groups dealt round-robin to the four waves (wave w
// takes groups g0 + w, g0 + w + 4, ...).  A block is a sequential chain of groups (each waits for its gathers), and the
// blocks of the reference's coupling matrices are long and uneven (level 2 of the 1M-row default hierarchy: 86 groups
// on average, 188 at most, 1,987 blocks of 16 rows -- fewer waves than the chip holds, and the launch lasts as long as
// the longest chain): four waves per block cut every chain to a quarter and quadruple the gathers in flight.  Partial
// tiles meet in LDS; wave w finishes column tile w of the block (fixed order: deterministic).
template <int RB, int NCT, bool AHEAD>
__global__ void __launch_bounds__(256, AHEAD ? SpmmAhead<RB>::WGS : 1) k_spmm_tile4(int64_t nrows, int64_t nblk, const int32_t *__restrict__ blk_gptr,
                                                    const int32_t *__restrict__ ucol, const double *__restrict__ coef,
                                                    const double *__restrict__ x, IoPtr<const double> bin_, int64_t ldb,
                                                    int nrhs, const int32_t *__restrict__ p, const double *__restrict__ s,
                                                    int64_t roff, double *__restrict__ out) {
  __shared__ double red[4][NCT][4][64];  // [wave][tile][reg][lane], 8 KB per column tile (one row tile at a time)
  const double *__restrict__ bin = bin_.get();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int kq = lane >> 4, jc = lane & 15;
  const int64_t b = (int64_t)xcd_block();
  if (b >= nblk) return;
  const int32_t g0 = rfl(blk_gptr[b]), g1 = rfl(blk_gptr[b + 1]);
  v4f64 acc[RB][NCT];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[rb][ct] = v4f64{0.0, 0.0, 0.0, 0.0};
  // this wave's groups: g0 + wave + 4 k, k = 0 .. ng - 1; same software pipeline as k_spmm_tile (loads unconditional,
  // indices clamped to the wave's last group, whose coefficient is then zeroed)
  const int32_t ng = (g1 - g0 > wave) ? (g1 - g0 - wave + 3) / 4 : 0;
  const int c = 16 * wave + jc;
  // AHEAD: the epilogue of column tile `wave` needs its rows' places in the level's input, their scales and right-hand sides,
  // none of which depends on the product -- requested up front, rows and the column clamped, zero selected at the use
  // -- the request order is places, the first two id sets, then (the wait for the places leaves the ids in flight) scales
  // and right-hand sides, then batch 0's operands: the loop's first wait for operands covers them all
  double sc[RB][4], bw[RB][4];
  if constexpr (AHEAD) {
    constexpr int BU = SpmmAhead<RB>::BU4;
    const tl_gdouble *bin_g = (const tl_gdouble *)bin, *s_g = (const tl_gdouble *)s;
    const tl_gdouble *x_g = (const tl_gdouble *)x, *coef_g = (const tl_gdouble *)coef;
    const tl_gint32 *p_g = (const tl_gint32 *)p, *ucol_g = (const tl_gint32 *)ucol;
#define HIFAMD_TL_GID(k) (g0 + wave + 4 * min((k), ng - 1))
    uint32_t prow[RB][4];
    uint32_t ia[BU], ib[BU];
    double ca[BU][RB], cb[BU][RB], ga[BU][NCT], gb[BU][NCT];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i = 16 * (RB * b + rb) + kq + 4 * r;
        prow[rb][r] = (uint32_t)p_g[roff + (i < nrows ? i : nrows - 1)];
      }
    if (ng > 0) {
      HIFAMD_TLA_IDS(ia, 0)
      HIFAMD_TLA_IDS(ib, BU)
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sc[rb][r] = s_g[prow[rb][r]];
        bw[rb][r] = bin_g[(int64_t)prow[rb][r] * ldb + min(c, nrhs - 1)];
      }
    __builtin_amdgcn_sched_barrier(0);
    if (ng > 0) {
      // (the second id set is touched here, or its request sinks into the loop's entry, behind batch 0's operands)
#pragma unroll
      for (int u = 0; u < BU; ++u) pin_here(ib[u]);
      HIFAMD_TLA_OPS(ga, ca, ia, 0)
      int32_t k = 0;
      for (; k + BU < ng; k += 2 * BU) {  // (one exit, at the top; two batches per trip)
        HIFAMD_TLA_STEP(ia, ib, ga, ca, gb, cb, k)
        HIFAMD_TLA_STEP(ib, ia, gb, cb, ga, ca, k + BU)
      }
      if (k < ng) {  // the wave's last batch: in registers or on its way
        HIFAMD_TLA_MUL(ga, ca, k)
      }
    }
#undef HIFAMD_TL_GID
  }
  if (!AHEAD && ng > 0) {
    const int32_t kl = ng - 1;
    int32_t src[8];
    double av[4][RB], bv[4][NCT];
#define HIFAMD_TL_GID(k) (g0 + wave + 4 * min((k), kl))
#define HIFAMD_TL_SRC(slot, k) src[slot] = ucol[4 * (int64_t)HIFAMD_TL_GID(k) + kq];
#define HIFAMD_TL_LOAD(slot, sslot, k)                                                                                \
  _Pragma("unroll") for (int rb = 0; rb < RB; ++rb) av[slot][rb] = coef[64 * (RB * (int64_t)HIFAMD_TL_GID(k) + rb) + lane]; \
  _Pragma("unroll") for (int ct = 0; ct < NCT; ++ct) bv[slot][ct] = x[((int64_t)src[sslot] << 6) + 16 * ct + jc];
#pragma unroll
    for (int q = 0; q < 7; ++q) { HIFAMD_TL_SRC(q, q) }
#pragma unroll
    for (int q = 0; q < 3; ++q) { HIFAMD_TL_LOAD(q, q, q) }
    for (int32_t k = 0; k < ng; k += 8) {
#pragma unroll
      for (int dd = 0; dd < 8; ++dd) {
        const int32_t cur = k + dd;
        HIFAMD_TL_LOAD((dd + 3) & 3, (dd + 3) & 7, cur + 3)
        HIFAMD_TL_SRC((dd + 7) & 7, cur + 7)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          const double am = cur < ng ? av[dd & 3][rb] : 0.0;
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) acc[rb][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(am, bv[dd & 3][ct], acc[rb][ct], 0, 0, 0);
        }
      }
    }
#undef HIFAMD_TL_GID
#undef HIFAMD_TL_SRC
#undef HIFAMD_TL_LOAD
  }
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    if (rb) __syncthreads();  // (the previous row tile's partials have been read)
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][ct][r][lane] = acc[rb][ct][r];
    __syncthreads();
    // epilogue of column tile `wave`: C layout col = l & 15, row = (l >> 4) + 4 * reg
    if (wave >= NCT) continue;  // (a narrow batch: fewer column tiles than waves)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = 16 * (RB * b + rb) + kq + 4 * r;
      if constexpr (AHEAD) {  // (only the store depends on the row)
        const double tot = ((red[0][wave][r][lane] + red[1][wave][r][lane]) + red[2][wave][r][lane]) + red[3][wave][r][lane];
        const double rhs = c < nrhs ? sc[rb][r] * bw[rb][r] : 0.0;
        if (i < nrows) out[(i << 6) + c] = rhs - tot;
      } else if (i < nrows) {
        const double tot = ((red[0][wave][r][lane] + red[1][wave][r][lane]) + red[2][wave][r][lane]) + red[3][wave][r][lane];
        const int32_t srow = p[roff + i];
        const double rhs = c < nrhs ? s[srow] * bin[(int64_t)srow * ldb + c] : 0.0;
        out[(i << 6) + c] = rhs - tot;
      }
    }
  }
}

#undef HIFAMD_TLA_IDS
#undef HIFAMD_TLA_OPS
#undef HIFAMD_TLA_MUL
#undef HIFAMD_TLA_STEP
#undef HIFAMD_TLA_RHS
#undef HIFAMD_TLA_PIN_ACC

// The tiled product for COMPLEX coupling blocks (round 4; host.hpp build_spmm_tiles(Csr<zdouble>)): one wave per 16-row
// block and 16-column slice of the (complex) batch -- blockIdx.y = slice --; a group's coefficients are two real tiles
// [re | im], a lane gathers the 16 bytes (re, im) of ITS source row and column, and the complex tile product is four real
// matrix instructions (rr, ii, ri, ir; out = (rr - ii) + i (ri + ir)).  Same software pipeline as k_spmm_tile: source-row
// indices 7 groups ahead, coefficient tiles and gathered rows 3 groups ahead, every load unconditional.
__global__ void __launch_bounds__(256) k_spmm_tile_z(int64_t nrows, int64_t nblk, const int32_t *__restrict__ blk_gptr,
                                                     const int32_t *__restrict__ ucol, const double *__restrict__ coef,
                                                     const cplx *__restrict__ x, IoPtr<const cplx> bin_, int64_t ldb, int nrhs,
                                                     const int32_t *__restrict__ p, const double *__restrict__ s, int64_t roff,
                                                     cplx *__restrict__ out) {
  const cplx *__restrict__ bin = bin_.get();
  const int lane = threadIdx.x & 63;
  const int kq = lane >> 4, jc = lane & 15;
  const int c = 16 * (int)blockIdx.y + jc;  // this lane's column of the 64-column (complex) arena
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t b = wave; b < nblk; b += nwaves) {
    const int32_t g0 = rfl(blk_gptr[b]), g1 = rfl(blk_gptr[b + 1]);
    v4f64 a_rr = v4f64{0.0, 0.0, 0.0, 0.0}, a_ii = a_rr, a_ri = a_rr, a_ir = a_rr;
    if (g0 < g1) {
      const int32_t gl = g1 - 1;
      int32_t src[8];
      double ar[4], ai[4];
      cplx bv[4];
#define HIFAMD_TLZ_SRC(slot, g) src[slot] = ucol[4 * (int64_t)min((g), gl) + kq];
#define HIFAMD_TLZ_LOAD(slot, sslot, g)                              \
  ar[slot] = coef[128 * (int64_t)min((g), gl) + lane];               \
  ai[slot] = coef[128 * (int64_t)min((g), gl) + 64 + lane];          \
  bv[slot] = x[((int64_t)src[sslot] << 6) + c];
#pragma unroll
      for (int q = 0; q < 7; ++q) { HIFAMD_TLZ_SRC(q, g0 + q) }
#pragma unroll
      for (int q = 0; q < 3; ++q) { HIFAMD_TLZ_LOAD(q, q, g0 + q) }
      for (int32_t g = g0; g < g1; g += 8) {
#pragma unroll
        for (int dd = 0; dd < 8; ++dd) {
          const int32_t cur = g + dd;
          HIFAMD_TLZ_LOAD((dd + 3) & 3, (dd + 3) & 7, cur + 3)
          HIFAMD_TLZ_SRC((dd + 7) & 7, cur + 7)
          const double mr = cur < g1 ? ar[dd & 3] : 0.0, mi = cur < g1 ? ai[dd & 3] : 0.0;
          a_rr = __builtin_amdgcn_mfma_f64_16x16x4f64(mr, bv[dd & 3].x, a_rr, 0, 0, 0);
          a_ii = __builtin_amdgcn_mfma_f64_16x16x4f64(mi, bv[dd & 3].y, a_ii, 0, 0, 0);
          a_ri = __builtin_amdgcn_mfma_f64_16x16x4f64(mr, bv[dd & 3].y, a_ri, 0, 0, 0);
          a_ir = __builtin_amdgcn_mfma_f64_16x16x4f64(mi, bv[dd & 3].x, a_ir, 0, 0, 0);
        }
      }
#undef HIFAMD_TLZ_SRC
#undef HIFAMD_TLZ_LOAD
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = 16 * b + kq + 4 * r;
      if (i < nrows) {
        const int32_t srow = p[roff + i];
        cplx rhs = cplx{0.0, 0.0};
        if (c < nrhs) rhs = vscale(s[srow], bin[(int64_t)srow * ldb + c]);
        out[(i << 6) + c] = cplx{rhs.x - (a_rr[r] - a_ii[r]), rhs.y - (a_ri[r] + a_ir[r])};
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// outer CRS SpMM: y = A x (RESID = false) or r = b - A x (RESID = true), tmp = 0; tmp += a*x
// ---------------------------------------------------------------------------------------------
template <class T, bool RESID>
__global__ void __launch_bounds__(256) k_crs_spmm(int64_t nrows, const int32_t *__restrict__ ptr,
                                                  const int32_t *__restrict__ col,
                                                  const T *__restrict__ val, const T *__restrict__ x,
                                                  int64_t ldx, const T *__restrict__ b, int64_t ldb,
                                                  T *__restrict__ y, int64_t ldy, int nrhs, int logR) {
  const LaneMap lm = lane_map(logR);
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave * lm.G + lm.g; i < nrows; i += nwaves * lm.G) {
    if (lm.c >= nrhs) continue;
    const int32_t k0 = ptr[i], k1 = ptr[i + 1];
    T acc = vzero(T());
    for (int32_t k = k0; k < k1; ++k) acc = vadd(acc, vmul(val[k], x[(int64_t)col[k] * ldx + lm.c]));
    if (RESID) acc = vsub(b[i * ldb + lm.c], acc);
    y[i * ldy + lm.c] = acc;
  }
}

// ---------------------------------------------------------------------------------------------
// compensated residual r = b - A x: every row's sum carried as an unevaluated pair (s, c), as if in twice the
// working precision (Dot2 of Ogita, Rump and Oishi with b_i as the first term).  Per row and column, in CRS order:
//   s = b_i; c = 0
//   per nonzero: p = (-a) x; e = fma(-a, x, -p)                          (TwoProd)
//                t = s + p; z = t - s; q = (s - (t - z)) + (p - z)       (TwoSum)
//                s = t; c = c + (q + e)
//   r_i = s + c
// A complex sum is two independent real sums of this form, started from Re b and Im b; per nonzero the real part takes
// (-ar xr) then (+ai xi), the imaginary part (-ar xi) then (-ai xr).  The order is fixed: a host restatement matches
// bit for bit.  One chain per sum -- a second accumulator would change the bits.  -ffp-contract=off keeps TwoSum as
// written; the fused multiply-add is explicit.  Launch shape and lane map of k_crs_spmm.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void dd_step(double &s, double &c, double a, double x) {
  const double p = a * x;
  const double e = __builtin_fma(a, x, -p);
  const double t = s + p;
  const double z = t - s;
  const double q = (s - (t - z)) + (p - z);
  s = t;
  c = c + (q + e);
}
struct DdAcc {
  double s, c;
};
struct DdAccZ {
  double sr, cr, si, ci;
};
__device__ __forceinline__ DdAcc dd_init(double b) { return DdAcc{b, 0.0}; }
__device__ __forceinline__ DdAccZ dd_init(cplx b) { return DdAccZ{b.x, 0.0, b.y, 0.0}; }
__device__ __forceinline__ void dd_sub(DdAcc &r, double a, double x) { dd_step(r.s, r.c, -a, x); }
__device__ __forceinline__ void dd_sub(DdAccZ &r, cplx a, cplx x) {
  dd_step(r.sr, r.cr, -a.x, x.x);
  dd_step(r.sr, r.cr, a.y, x.y);
  dd_step(r.si, r.ci, -a.x, x.y);
  dd_step(r.si, r.ci, -a.y, x.x);
}
__device__ __forceinline__ double dd_value(const DdAcc &r) { return r.s + r.c; }
__device__ __forceinline__ cplx dd_value(const DdAccZ &r) { return cplx{r.sr + r.cr, r.si + r.ci}; }

// AH >= 2 slots hold the nonzeros k .. k + AH - 1 (coefficient and x entry) and the column indices of the next AH; a
// slot is requested again right behind its sum, so a request has the AH - 1 sums of the other slots to land in (asked
// for IN FRONT of the sum, the old value is still live, the new one gets a register of its own and the copy at the
// back edge waits for every load).  Full trips in a loop with one exit, the remainder behind it from the slots; every
// load is unconditional (clamped to the row's last nonzero), and the values requested in front of the loop
// are touched there (pin_here), or the compiler folds each request into a load in front of its use.
// Timing only: every AH gives the same bits.
template <class T, int AH>
__global__ void __launch_bounds__(256) k_crs_resid_dd(int64_t nrows, const int32_t *__restrict__ ptr,
                                                      const int32_t *__restrict__ col,
                                                      const T *__restrict__ val, const T *__restrict__ x,
                                                      int64_t ldx, const T *__restrict__ b, int64_t ldb,
                                                      T *__restrict__ y, int64_t ldy, int nrhs, int logR) {
  const LaneMap lm = lane_map(logR);
  const int cc = min(lm.c, nrhs - 1);  // a lane beyond the batch reads its last column and stores nothing
  const uint32_t *__restrict__ ucol = (const uint32_t *)col;  // (never negative: widened by zero)
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave * lm.G + lm.g; i < nrows; i += nwaves * lm.G) {
    const int32_t k0 = ptr[i], k1 = ptr[i + 1];
    auto acc = dd_init(b[i * ldb + cc]);
    if (k0 < k1) {
      const int32_t kl = k1 - 1;
      T a[AH], xv[AH];
      uint32_t j[AH];
#pragma unroll
      for (int q = 0; q < AH; ++q) {
        j[q] = ucol[min(k0 + AH + q, kl)];
        a[q] = val[min(k0 + q, kl)];
        xv[q] = x[(int64_t)ucol[min(k0 + q, kl)] * ldx + cc];
      }
#pragma unroll
      for (int q = 0; q < AH; ++q) {
        pin_here(j[q]);
        pin_here(a[q]);
        pin_here(xv[q]);
      }
      int32_t k = k0;
      for (; k + AH <= k1; k += AH) {  // full trips; a slot is requested again right behind its sum
#pragma unroll
        for (int q = 0; q < AH; ++q) {
          dd_sub(acc, a[q], xv[q]);
          const uint32_t jc = j[q];
          j[q] = ucol[min(k + q + 2 * AH, kl)];
          a[q] = val[min(k + q + AH, kl)];
          xv[q] = x[(int64_t)jc * ldx + cc];
        }
      }
#pragma unroll
      for (int q = 0; q < AH - 1; ++q)  // the remainder sits in the slots already
        if (k + q < k1) dd_sub(acc, a[q], xv[q]);
    }
    if (lm.c < nrhs) y[i * ldy + lm.c] = dd_value(acc);
  }
}

// ---------------------------------------------------------------------------------------------
// prec_prod (y = M b, alg/prec_prod.hpp:55-147): the inverse direction of the apply.  No dependent steps
// except the one LDU solve of the Schur coupling term, so these are plain row-gather kernels.
// ---------------------------------------------------------------------------------------------
// g[i] = b[q[i]] / t[q[i]], rows [0, cnt)   (:76, :97; with (p, s) for the transposed product)
template <class T>
__global__ void __launch_bounds__(256) k_gather_div(IoPtr<const T> bin_, int64_t ldb, int nrhs,
                                                    const int32_t *__restrict__ q, const double *__restrict__ t,
                                                    int64_t cnt, T *__restrict__ g, int logR) {
  const T *__restrict__ bin = bin_.get();
  const LaneMap lm = lane_map(logR);
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave * lm.G + lm.g; i < cnt; i += nwaves * lm.G) {
    const int32_t src = q[i];
    T val = vzero(T());
    if (lm.c < nrhs) val = vdivr(bin[(int64_t)src * ldb + lm.c], t[src]);
    g[(i << logR) + lm.c] = val;
  }
}

// y[i] = r[p_inv[i]] / s[i], rows [0, n)   (:132)
template <class T>
__global__ void __launch_bounds__(256) k_scatter_div(const T *__restrict__ r, const int32_t *__restrict__ pinv,
                                                     const double *__restrict__ s, int64_t n, IoPtr<T> yout_,
                                                     int64_t ldy, int nrhs, int logR) {
  T *__restrict__ yout = yout_.get();
  const LaneMap lm = lane_map(logR);
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave * lm.G + lm.g; i < n; i += nwaves * lm.G)
    if (lm.c < nrhs) yout[i * ldy + lm.c] = vdivr(r[((int64_t)pinv[i] << logR) + lm.c], s[i]);
}

// rows of a unit triangle times a vector, slot-ordered CSR (rowid): out[i] = (sum_k A(i,k) x[k] + x[i]) [* d[i]]
// (:101-103 with d, :106-108 without)
template <class T, bool SCALE>
__global__ void __launch_bounds__(256) k_prod_rows(int64_t nrows, const int32_t *__restrict__ ptr,
                                                   const int32_t *__restrict__ col, const T *__restrict__ val,
                                                   const int32_t *__restrict__ rowid, const T *__restrict__ x,
                                                   const T *__restrict__ d, T *__restrict__ out, int logR) {
  const LaneMap lm = lane_map(logR);
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t sidx = wave * lm.G + lm.g; sidx < nrows; sidx += nwaves * lm.G) {
    const int64_t i = rowid[sidx];
    T acc = vzero(T());
    for (int32_t k = ptr[sidx]; k < ptr[sidx + 1]; ++k) acc = vadd(acc, vmul(x[((int64_t)col[k] << logR) + lm.c], val[k]));
    acc = vadd(acc, x[(i << logR) + lm.c]);
    if (SCALE) acc = vmul(acc, d[i]);
    out[(i << logR) + lm.c] = acc;
  }
}

// t = sum_k A(i,k) x[k];  MODE 0: out[i] = t, acc[i] += t  (F term, :113-114)
//                         MODE 1: out[i] = t + add[i]      (E term + child product, :125-127)
template <class T, int MODE>
__global__ void __launch_bounds__(256) k_spmm_prod(int64_t nrows, const int32_t *__restrict__ ptr,
                                                   const int32_t *__restrict__ col, const T *__restrict__ val,
                                                   const T *__restrict__ x, T *__restrict__ out, T *accio,
                                                   const T *__restrict__ add, int logR) {
  const LaneMap lm = lane_map(logR);
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave * lm.G + lm.g; i < nrows; i += nwaves * lm.G) {
    T t = vzero(T());
    for (int32_t k = ptr[i]; k < ptr[i + 1]; ++k) t = vadd(t, vmul(x[((int64_t)col[k] << logR) + lm.c], val[k]));
    if (MODE == 0) {
      out[(i << logR) + lm.c] = t;
      accio[(i << logR) + lm.c] = vadd(accio[(i << logR) + lm.c], t);
    } else {
      out[(i << logR) + lm.c] = vadd(t, add[(i << logR) + lm.c]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// BLAS-1 helpers of iterative refinement (alg/IterRefine.hpp:99,103,147,156-157), [n][nrhs] blocks
// ---------------------------------------------------------------------------------------------
// op 0: y = 0 | 1: y = x | 2: y += x | 3: y = x + z
template <class T>
__global__ void __launch_bounds__(256) k_vec_op(int op, int64_t n, int nrhs, T *y, int64_t ldy,
                                                const T *x, int64_t ldx, const T *z, int64_t ldz) {
  const int64_t total = n * nrhs;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / nrhs;
    const int c = (int)(e - i * nrhs);
    T r;
    if (op == 0)
      r = vzero(T());
    else if (op == 1)
      r = x[i * ldx + c];
    else if (op == 2)
      r = vadd(y[i * ldy + c], x[i * ldx + c]);
    else
      r = vadd(x[i * ldx + c], z[i * ldz + c]);
    y[i * ldy + c] = r;
  }
}

// masked axpy kernel for the bounded IR variant
template <class D>
__global__ void __launch_bounds__(256) k_masked_add(int64_t n, int nrhs, D *y, int64_t ldy, const D *x, int64_t ldx,
                                                    const int *mask) {
  const int64_t total = n * nrhs;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / nrhs;
    const int c = (int)(e - i * nrhs);
    if (mask[c]) y[i * ldy + c] = vadd(y[i * ldy + c], x[i * ldx + c]);
  }
}

// where mask[c]: y[:, c] = x[:, c], or 0 when x is NULL
template <class D>
__global__ void __launch_bounds__(256) k_masked_set(int64_t n, int nrhs, D *y, int64_t ldy, const D *x, int64_t ldx,
                                                    const int *mask) {
  const int64_t total = n * nrhs;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / nrhs;
    const int c = (int)(e - i * nrhs);
    if (mask[c]) y[i * ldy + c] = x ? x[i * ldx + c] : vzero(D());
  }
}

__device__ __forceinline__ double vabs2(double a) { return a * a; }
__device__ __forceinline__ double vabs2(cplx a) { return a.x * a.x + a.y * a.y; }

// per-column sum of squares; partial[block][c] then a tiny second pass on the host side of the API
template <class T>
__global__ void __launch_bounds__(256) k_colnorm2_partial(int64_t n, int nrhs, const T *x, int64_t ldx,
                                                          double *partial /* [gridDim.x][nrhs] */) {
  __shared__ double sm[256];
  // thread t owns column c = t % nrhs_pad over a strided set of rows
  const int cpad = nrhs;  // nrhs <= 64 here
  const int rows_per_pass = 256 / cpad;
  const int c = threadIdx.x % cpad, rloc = threadIdx.x / cpad;
  double acc = 0.0;
  if (rloc < rows_per_pass)
    for (int64_t i = (int64_t)blockIdx.x * rows_per_pass + rloc; i < n; i += (int64_t)gridDim.x * rows_per_pass)
      acc += vabs2(x[i * ldx + c]);
  sm[threadIdx.x] = (rloc < rows_per_pass) ? acc : 0.0;
  __syncthreads();
  if (threadIdx.x < cpad) {
    double tot = 0.0;
    for (int r = 0; r < rows_per_pass; ++r) tot += sm[r * cpad + threadIdx.x];
    partial[(int64_t)blockIdx.x * nrhs + threadIdx.x] = tot;
  }
}

// ---------------------------------------------------------------------------------------------
// Constant-mode null-space filter (NspFilter::_const_filter, NspFilter.hpp:161-175): every column loses
// the mean of its rows [r0, r1).  Two launches, no host round trip: per-block partial column sums, then
// every block re-adds the partials (fixed order: deterministic) and subtracts.
// ---------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(256) k_colsum_partial(int64_t r0, int64_t r1, int nrhs, const T *x, int64_t ldx,
                                                        T *partial /* [gridDim.x][nrhs] */) {
  __shared__ T sm[256];
  const int cpad = nrhs;  // nrhs <= 64 here
  const int rows_per_pass = 256 / cpad;
  const int c = threadIdx.x % cpad, rloc = threadIdx.x / cpad;
  T acc = vzero(T());
  if (rloc < rows_per_pass)
    for (int64_t i = r0 + (int64_t)blockIdx.x * rows_per_pass + rloc; i < r1; i += (int64_t)gridDim.x * rows_per_pass)
      acc = vadd(acc, x[i * ldx + c]);
  sm[threadIdx.x] = (rloc < rows_per_pass) ? acc : vzero(T());
  __syncthreads();
  if (threadIdx.x < cpad) {
    T tot = vzero(T());
    for (int r = 0; r < rows_per_pass; ++r) tot = vadd(tot, sm[r * cpad + threadIdx.x]);
    partial[(int64_t)blockIdx.x * nrhs + threadIdx.x] = tot;
  }
}

template <class T>
__global__ void __launch_bounds__(256) k_sub_colmean(int64_t r0, int64_t r1, int nrhs, T *x, int64_t ldx,
                                                     const T *__restrict__ partial, int nblk) {
  __shared__ T mean[64];
  if (threadIdx.x < nrhs) {
    T tot = vzero(T());
    for (int b = 0; b < nblk; ++b) tot = vadd(tot, partial[(int64_t)b * nrhs + threadIdx.x]);
    mean[threadIdx.x] = vdivr(tot, (double)(r1 - r0));
  }
  __syncthreads();
  const int64_t total = (r1 - r0) * nrhs;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = r0 + e / nrhs;
    const int c = (int)(e % nrhs);
    x[i * ldx + c] = vsub(x[i * ldx + c], mean[c]);
  }
}

// ---------------------------------------------------------------------------------------------
// Device-resident Arnoldi process of the batched GMRES driver (examples/advanced/gmres.hpp:57-103 for up to
// 64 columns in lock step): the Hessenberg column, the rotations, the residuals and the per-column state
// (iteration count, flag, active mask) live in HBM; the host sees the three ctl counters per inner step.
// The inner product is the Hermitian one, h = sum conj(q_i) v_i (for real data this IS hif::inner,
// utils/math.hpp:83; for complex data the example's sum conj(v_i) q_i would not orthogonalize).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double vconj(double a) { return a; }
__device__ __forceinline__ cplx vconj(cplx a) { return cplx{a.x, -a.y}; }
__device__ __forceinline__ double vreal(double a) { return a; }
__device__ __forceinline__ double vreal(cplx a) { return a.x; }
__device__ __forceinline__ double vfromreal(double r, double) { return r; }
__device__ __forceinline__ cplx vfromreal(double r, cplx) { return cplx{r, 0.0}; }
__device__ __forceinline__ double vabs1(double a) { return fabs(a); }
__device__ __forceinline__ double vabs1(cplx a) { return sqrt(a.x * a.x + a.y * a.y); }
__device__ __forceinline__ bool viszero(double a) { return a == 0.0; }
__device__ __forceinline__ bool viszero(cplx a) { return a.x == 0.0 && a.y == 0.0; }

template <class T>
struct GmState : KrylovState {  // bnorm: ||b|| (beta0, :30); ctl: [0] columns still active after the step  [1] max jfin  [2] columns not done
  T *w2;          // [nc][restart]           Hessenberg column of the running step (gmres.hpp:64,73-78)
  T *Jc;          // [nc][restart]           J(:,0)
  double *Js;     // [nc][restart]           J(:,1) (real)
  T *y;           // [nc][restart + 1]
  T *R;           // [nc][restart][restart]  column j of column c at R + (c * restart + j) * restart
  double *resid;
  int *jfin, *done, *sweeps;
  T *alpha;       // [nc] coefficient of the next column operation
  int restart;
};

// One modified-Gram-Schmidt step, fused: first v -= h_prev q_prev (the axpy of the PREVIOUS step, :65), then the
// block's share of sum conj(q_i) v_i (:64) -- or of sum |v_i|^2 (:67) when q == nullptr.  v, q: [n][nc] contiguous.
template <class T>
__global__ void __launch_bounds__(256) k_gm_step(int64_t n, int nc, T *__restrict__ v, const T *__restrict__ qp,
                                                 const T *__restrict__ hp, const T *__restrict__ q,
                                                 T *__restrict__ partial /* [gridDim.x][nc] */) {
  __shared__ T sm[256];
  const int rpp = 256 / nc;
  const int c = threadIdx.x % nc, rloc = threadIdx.x / nc;
  T acc = vzero(T());
  if (rloc < rpp) {
    const T h = qp ? hp[c] : vzero(T());
    const int64_t step = (int64_t)gridDim.x * rpp;
    for (int64_t i = (int64_t)blockIdx.x * rpp + rloc; i < n; i += step) {
      T x = v[i * nc + c];
      if (qp) {
        x = vsub(x, vmul(h, qp[i * nc + c]));
        v[i * nc + c] = x;
      }
      acc = vadd(acc, q ? vmul(vconj(q[i * nc + c]), x) : vfromreal(vabs2(x), T()));
    }
  }
  sm[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < nc) {
    T tot = vzero(T());
    for (int r = 0; r < rpp; ++r) tot = vadd(tot, sm[r * nc + threadIdx.x]);
    partial[(int64_t)blockIdx.x * nc + threadIdx.x] = tot;
  }
}

// Modified Gram-Schmidt against a BLOCK of MB basis vectors in one pass over v (the orthogonalization is bound by
// the bytes of v and Q it moves: 4 vector passes per basis vector one at a time, (2 MB + 2) / MB in blocks).  In exact
// arithmetic the coefficients of modified Gram-Schmidt satisfy
//     h_{k+a} = q_{k+a}^H v^(k+a) = q_{k+a}^H v^(k) - sum_{l<a} h_{k+l} (q_{k+a}^H q_{k+l}),
// so one pass delivers b_a = q_{k+a}^H v^(k) and the block's Gram entries g_{a,l} = q_{k+a}^H q_{k+l} (l < a) -- the
// basis vectors are being read anyway -- and a finishing kernel runs the recursion (k_gm_hblock).  The same pass first
// applies the PREVIOUS block's update v -= sum_l h_l q_l (gmres.hpp:65).  Value list of a block: b_0..b_{mn-1}, then
// g_{1,0}, g_{2,0}, g_{2,1}, ...; mn == 0: |v|^2 only (the pass behind the last block, :67).
constexpr int kGmBlock = 4;
constexpr int kGmVals = kGmBlock + kGmBlock * (kGmBlock - 1) / 2;
template <class T>
__global__ void __launch_bounds__(256) k_gm_block(int64_t n, int nc, T *__restrict__ v, const T *__restrict__ Qp, int mp,
                                                  const T *__restrict__ hp /* [kGmBlock][64] */, const T *__restrict__ Qn,
                                                  int mn, T *__restrict__ partial /* [gridDim.x][nv][nc] */) {
  __shared__ T sm[256];
  const int rpp = 256 / nc;
  const int c = threadIdx.x % nc, rloc = threadIdx.x / nc;
  const int64_t vec = n * nc;
  T acc[kGmVals];
#pragma unroll
  for (int a = 0; a < kGmVals; ++a) acc[a] = vzero(T());
  if (rloc < rpp) {
    T h[kGmBlock];
#pragma unroll
    for (int l = 0; l < kGmBlock; ++l) h[l] = (l < mp) ? hp[l * 64 + c] : vzero(T());
    const int64_t step = (int64_t)gridDim.x * rpp;
    for (int64_t i = (int64_t)blockIdx.x * rpp + rloc; i < n; i += step) {
      const int64_t o = i * nc + c;
      T x = v[o];
      if (mp) {
#pragma unroll
        for (int l = 0; l < kGmBlock; ++l)
          if (l < mp) x = vsub(x, vmul(h[l], Qp[(int64_t)l * vec + o]));
        v[o] = x;
      }
      if (mn == 0) {
        acc[0] = vadd(acc[0], vfromreal(vabs2(x), T()));
      } else {
        T q[kGmBlock];
#pragma unroll
        for (int a = 0; a < kGmBlock; ++a) q[a] = (a < mn) ? Qn[(int64_t)a * vec + o] : vzero(T());
#pragma unroll
        for (int a = 0; a < kGmBlock; ++a) {
          const T qc = vconj(q[a]);
          acc[a] = vadd(acc[a], vmul(qc, x));
#pragma unroll
          for (int l = 0; l < a; ++l) acc[kGmBlock + a * (a - 1) / 2 + l] = vadd(acc[kGmBlock + a * (a - 1) / 2 + l], vmul(qc, q[l]));
        }
      }
    }
  }
  // value a of the block lives at slot (a < kGmBlock ? a : mn + (a - kGmBlock)) of the launch's value list
  const int nv = mn ? mn + mn * (mn - 1) / 2 : 1;
#pragma unroll
  for (int a = 0; a < kGmVals; ++a) {
    int slot;
    if (a < kGmBlock) {
      slot = (a < mn || (mn == 0 && a == 0)) ? a : -1;
    } else {
      // (a - kGmBlock) enumerates pairs (row, l) with row = 1.., l < row in the order above
      int row = 1, rem = a - kGmBlock;
      while (rem >= row) rem -= row, ++row;
      slot = row < mn ? mn + row * (row - 1) / 2 + rem : -1;
    }
    if (slot < 0) continue;  // (block-uniform)
    __syncthreads();
    sm[threadIdx.x] = acc[a];
    __syncthreads();
    if (threadIdx.x < nc) {
      T tot = vzero(T());
      for (int r = 0; r < rpp; ++r) tot = vadd(tot, sm[r * nc + threadIdx.x]);
      partial[((int64_t)blockIdx.x * nv + slot) * nc + threadIdx.x] = tot;
    }
  }
}

// red[val][c] = sum over the blocks' partials, fixed order; one workgroup per value of the list
template <class T>
__global__ void __launch_bounds__(256) k_gm_reduce(const T *__restrict__ partial, int nblk, int nv, int nc, T *__restrict__ red) {
  __shared__ T sm[256];
  const int val = blockIdx.x;
  const int rpp = 256 / nc;
  const int c = threadIdx.x % nc, g = threadIdx.x / nc;
  T acc = vzero(T());
  if (g < rpp)
    for (int b = g; b < nblk; b += rpp) acc = vadd(acc, partial[((int64_t)b * nv + val) * nc + c]);
  sm[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < nc) {
    T tot = vzero(T());
    for (int r = 0; r < rpp; ++r) tot = vadd(tot, sm[r * nc + c]);
    red[val * 64 + c] = tot;
  }
}

// the recursion of a block (see k_gm_block): h_{k+a} into the Hessenberg column and into hb[a][c] for the next pass
template <class T>
__global__ void __launch_bounds__(64) k_gm_hblock(const T *__restrict__ red, int nc, int k, int mn, GmState<T> S,
                                                  T *__restrict__ hb /* [kGmBlock][64] */) {
  const int c = threadIdx.x;
  if (c >= nc) return;
  T h[kGmBlock];
#pragma unroll
  for (int a = 0; a < kGmBlock; ++a) {
    if (a >= mn) break;
    T t = red[a * 64 + c];
    for (int l = 0; l < a; ++l) t = vsub(t, vmul(h[l], red[(mn + a * (a - 1) / 2 + l) * 64 + c]));
    h[a] = t;
    S.w2[(size_t)c * S.restart + k + a] = t;
    hb[a * 64 + c] = t;
  }
}

// Finishes a reduction (fixed order: deterministic) and does the per-column scalar work of the driver.
//   mode 0: h_k of step k -> w2[k], alpha                                       (:64)
//   mode 1: |v|^2 of step j: rotations, residual, stopping rules                 (:67-103); alpha = |v| for :69-70
//   mode 2: start of an outer cycle: beta, y[0], active mask                    (:53-55)
//   mode 3: start of the solve: beta0, quick return                              (:30-36)
template <class T>
__global__ void __launch_bounds__(256) k_gm_finish(const T *__restrict__ partial, int nblk, int nc, int mode, int k,
                                                   int nirs, GmState<T> S) {
  __shared__ T sm[256];
  __shared__ int cnt[2];
  const int rpp = 256 / nc;
  const int c = threadIdx.x % nc, g = threadIdx.x / nc;
  T acc = vzero(T());
  if (g < rpp)
    for (int b = g; b < nblk; b += rpp) acc = vadd(acc, partial[(int64_t)b * nc + c]);
  sm[threadIdx.x] = acc;
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x < nc) {
    T tot = vzero(T());
    for (int r = 0; r < rpp; ++r) tot = vadd(tot, sm[r * nc + c]);
    const int rs = S.restart;
    if (mode == 0) {
      S.w2[(size_t)c * rs + k] = tot;
      S.alpha[c] = tot;
    } else if (mode == 3) {
      const double b0 = sqrt(vreal(tot));
      S.bnorm[c] = b0;
      S.done[c] = (b0 == 0.0);
      S.resid[c] = 1.0;
      S.iter[c] = 0;
      S.flag[c] = 0;
      S.sweeps[c] = 0;
      S.active[c] = 0;
      S.jfin[c] = -1;
      if (b0 != 0.0) atomicAdd(&cnt[1], 1);
    } else if (mode == 2) {
      const double beta = sqrt(vreal(tot));
      int dn = S.done[c];
      if (!dn && beta == 0.0) dn = 1;  // exact solution reached
      S.done[c] = dn;
      S.y[(size_t)c * (rs + 1)] = vfromreal(beta, T());
      S.alpha[c] = vfromreal(dn ? 0.0 : beta, T());
      S.active[c] = !dn;
      S.jfin[c] = -1;
      if (!dn) atomicAdd(&cnt[0], 1);
    } else {
      const int j = k;
      const double v_norm2 = vreal(tot), v_norm = sqrt(v_norm2);
      const int act = S.active[c];
      S.alpha[c] = vfromreal(act ? v_norm : 0.0, T());
      if (act) {
        S.sweeps[c] += nirs;
        T *wc = S.w2 + (size_t)c * rs, *yc = S.y + (size_t)c * (rs + 1), *Jc = S.Jc + (size_t)c * rs;
        double *Js = S.Js + (size_t)c * rs;
        T *Rc = S.R + (size_t)c * rs * rs;
        for (int cj = 0; cj + 1 <= j; ++cj) {  // :73-78
          const T t0 = wc[cj], t1 = wc[cj + 1];
          wc[cj] = vadd(vmul(vconj(Jc[cj]), t0), vscale(Js[cj], t1));
          wc[cj + 1] = vadd(vscale(-Js[cj], t0), vmul(Jc[cj], t1));
        }
        const double rho = sqrt(vabs2(wc[j]) + v_norm2);  // :79
        Jc[j] = vdivr(wc[j], rho);
        Js[j] = v_norm / rho;
        yc[j + 1] = vscale(-Js[j], yc[j]);
        yc[j] = vmul(vconj(Jc[j]), yc[j]);
        wc[j] = vfromreal(rho, T());
        for (int i = 0; i <= j; ++i) Rc[(size_t)j * rs + i] = wc[i];  // :85
        const double resid_prev = S.resid[c];
        const double resid = vabs1(yc[j + 1]) / S.bnorm[c];  // :89
        S.resid[c] = resid;
        bool brk = false;
        if (resid >= resid_prev * (1.0 - 1e-8)) {  // :90-93
          S.flag[c] = 1;
          brk = true;
        } else if (S.iter[c] >= S.maxit) {  // :94-97
          S.flag[c] = 2;
          brk = true;
        } else {
          S.iter[c] += 1;
          if (resid <= S.rtol || j + 1 >= rs) brk = true;  // :102
        }
        if (brk) {
          S.jfin[c] = j;
          S.active[c] = 0;
        } else {
          atomicAdd(&cnt[0], 1);
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (mode == 1 || mode == 2) S.ctl[0] = cnt[0];
    if (mode == 3) S.ctl[2] = cnt[1];
  }
}

// End of an outer cycle: back substitution R y = g per column (:106-110), alpha = 1 for the columns that took part,
// done flags (:120); ctl[1] = max jfin, ctl[2] = columns not done.
template <class T>
__global__ void __launch_bounds__(64) k_gm_backsolve(int nc, GmState<T> S) {
  __shared__ int red[2];
  if (threadIdx.x < 2) red[threadIdx.x] = threadIdx.x ? 0 : -1;
  __syncthreads();
  const int c = threadIdx.x;
  if (c < nc) {
    const int rs = S.restart, jf = S.jfin[c];
    if (jf >= 0) {
      T *yc = S.y + (size_t)c * (rs + 1);
      const T *Rc = S.R + (size_t)c * rs * rs;
      for (int k = jf; k > -1; --k) {
        yc[k] = vdiv(yc[k], Rc[(size_t)k * rs + k]);
        const T t0 = yc[k];
        for (int i = k - 1; i > -1; --i) yc[i] = vsub(yc[i], vmul(t0, Rc[(size_t)k * rs + i]));
      }
      atomicMax(&red[0], jf);
      if (S.resid[c] <= S.rtol || S.flag[c] != 0) S.done[c] = 1;
    }
    S.alpha[c] = vfromreal(jf >= 0 ? 1.0 : 0.0, T());
    if (!S.done[c]) atomicAdd(&red[1], 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    S.ctl[1] = red[0];
    S.ctl[2] = red[1];
  }
}

// out = (accumulate ? out : 0) + sum_{k <= jmax} coef_k Q_k, coef_k[c] = y[c][k] for the columns with jfin >= k, in
// the order of :112-116 / :214-218; Q_k = Q + k * n * nc, [n][nc] contiguous
template <class T>
__global__ void __launch_bounds__(256) k_gm_combine(int64_t n, int nc, T *__restrict__ out, int64_t ldo, int accumulate,
                                                    const T *__restrict__ Q, int jmax, GmState<T> S) {
  const int64_t total = n * nc;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / nc;
    const int c = (int)(e - i * nc);
    const int jf = S.jfin[c];
    const T *yc = S.y + (size_t)c * (S.restart + 1);
    T r = accumulate ? out[i * ldo + c] : vzero(T());
    for (int k = 0; k <= jmax; ++k) {
      const T a = (jf >= k) ? yc[k] : vzero(T());
      r = vadd(r, vmul(a, Q[(size_t)k * (size_t)total + (size_t)e]));
    }
    out[i * ldo + c] = r;
  }
}

// op 0: y[:,c] += alpha[c] x[:,c] | 1: y[:,c] = x[:,c] / real(alpha[c]) (0 where alpha[c] == 0: a column that has
// left the iteration keeps a zero basis vector); alpha on the device
template <class T>
__global__ void __launch_bounds__(256) k_gm_colop(int op, int64_t n, int nc, T *__restrict__ y, int64_t ldy,
                                                  const T *__restrict__ x, int64_t ldx, const T *__restrict__ alpha) {
  const int64_t total = n * nc;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / nc;
    const int c = (int)(e - i * nc);
    const T a = alpha[c];
    if (op == 0)
      y[i * ldy + c] = vadd(y[i * ldy + c], vmul(a, x[i * ldx + c]));
    else
      y[i * ldy + c] = viszero(a) ? vzero(T()) : vdivr(x[i * ldx + c], vreal(a));
  }
}

// ---------------------------------------------------------------------------------------------
// Device-resident preconditioned CG for a Hermitian positive-definite pair (A, M), up to 64 columns in lock step
// (Engine::pcg_tile).  Vectors are [n][nc] contiguous.  Lane = column: wave w of block b owns the rows
// i = 4 b + w + k * 4 kCgBlocks, every lane walks them in that order, the four waves of a block are added in wave
// order and the kCgBlocks partials of a column in a fixed order by k_cg_finish.  Nothing of that depends on nc or
// on the other columns, so a column's bits do not depend on the batch it travels in (unlike k_gm_step, whose
// rows per pass are 256 / nc).  Inner products are Hermitian, sum conj(a_i) b_i.
// ---------------------------------------------------------------------------------------------
constexpr int kCgBlocks = 1024;  // blocks of 4 waves of every fused pass (and partials per column)

// (KrylovState, what the lock-step solvers' states share: blockcg_small.hpp, whose host-tested decisions need it HIP-free)

template <class T>
struct CgState : KrylovState {
  T *rho, *alpha, *beta;  // [64]  r^H z of the last step, rho / sigma, rho' / rho (0 for a frozen column)
};

// adds the four wave partials of a block in wave order: partial[blockIdx.x][c], stride 64
template <class T>
__device__ __forceinline__ void cg_block_partial(T acc, T *sm /* [4][64] */, T *__restrict__ partial) {
  const int w = threadIdx.x >> 6, c = threadIdx.x & 63;
  sm[w * 64 + c] = acc;
  __syncthreads();
  if (threadIdx.x < 64)
    partial[(int64_t)blockIdx.x * 64 + c] = vadd(vadd(vadd(sm[c], sm[64 + c]), sm[128 + c]), sm[192 + c]);
}

// the block's share of sum conj(a_i) b_i per column (b == nullptr: sum |a_i|^2); a has the row stride lda
template <class T>
__global__ void __launch_bounds__(256) k_cg_dot(int64_t n, int nc, const T *__restrict__ a, int64_t lda,
                                                const T *__restrict__ b, T *__restrict__ partial /* [kCgBlocks][64] */) {
  __shared__ T sm[256];
  const int c = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  T acc = vzero(T());
  if (c < nc) {
    // (one loop per form: with the choice inside the loop the load of b stays conditional and the pass does not pipeline)
    if (b)
      for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += stride)
        acc = vadd(acc, vmul(vconj(a[i * lda + c]), b[i * nc + c]));
    else
      for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += stride)
        acc = vadd(acc, vfromreal(vabs2(a[i * lda + c]), T()));
  }
  cg_block_partial(acc, sm, partial);
}

// x += alpha p, r -= alpha q on the active columns, fused with the block's share of |r|^2 (x: row stride ldx).  Also
// BiCGSTAB's half step x += alpha y, r -= alpha v (r then holds s).
template <class T>
__global__ void __launch_bounds__(256) k_cg_xr(int64_t n, int nc, T *__restrict__ x, int64_t ldx, T *__restrict__ r,
                                               const T *__restrict__ p, const T *__restrict__ q,
                                               const T *__restrict__ alpha, const int *__restrict__ active,
                                               T *__restrict__ partial /* [kCgBlocks][64] */) {
  __shared__ T sm[256];
  const int c = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  T acc = vzero(T());
  if (c < nc) {
    const bool act = active[c] != 0;
    const T al = alpha[c];
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += stride) {
      T ri = r[i * nc + c];
      if (act) {
        x[i * ldx + c] = vadd(x[i * ldx + c], vmul(al, p[i * nc + c]));
        ri = vsub(ri, vmul(al, q[i * nc + c]));
        r[i * nc + c] = ri;
      }
      acc = vadd(acc, vfromreal(vabs2(ri), T()));
    }
  }
  cg_block_partial(acc, sm, partial);
}

// p = z + beta p on the active columns
template <class T>
__global__ void __launch_bounds__(256) k_cg_p(int64_t n, int nc, T *__restrict__ p, const T *__restrict__ z,
                                              const T *__restrict__ beta, const int *__restrict__ active) {
  const int c = threadIdx.x & 63;
  if (c >= nc || !active[c]) return;
  const T be = beta[c];
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += stride)
    p[i * nc + c] = vadd(z[i * nc + c], vmul(be, p[i * nc + c]));
}

// not a usable curvature / preconditioned residual norm: not finite, or real part <= 0
__device__ __forceinline__ bool cg_bad(double v) { return !(v > 0.0) || !isfinite(v); }
__device__ __forceinline__ bool cg_bad(cplx v) { return !(v.x > 0.0) || !isfinite(v.x) || !isfinite(v.y); }

// The two shared parts of the finishing kernels (one workgroup of 16 waves; every thread calls both).
// The kCgBlocks partials of column c = threadIdx.x & 63 in a fixed order: wave w takes blocks w, w + 16, ..., then
// the 16 wave sums are added in wave order.  Thread c < nc gets the total.  partial == nullptr sums to zero.  Its
// barrier also publishes what the caller wrote to shared memory before (the zeroed active count).
template <class T>
__device__ __forceinline__ T cg_sum_partials(const T *__restrict__ partial, int nc, T *sm /* [16][64] */) {
  const int w = threadIdx.x >> 6, c = threadIdx.x & 63;
  T acc = vzero(T());
  if (c < nc && partial)
    for (int b = w; b < kCgBlocks; b += 16) acc = vadd(acc, partial[(int64_t)b * 64 + c]);
  sm[threadIdx.x] = acc;
  __syncthreads();
  T tot = vzero(T());
  if (threadIdx.x < nc)
    for (int v = 0; v < 16; ++v) tot = vadd(tot, sm[v * 64 + c]);
  return tot;
}
// Closes a mode for column c = threadIdx.x < nc: a column that stops here (stop >= 0: its flag, it: its count) leaves
// the iteration, zero(c) clears the coefficients of a column that is out (so that the vector passes leave it alone; a
// column that left earlier has them zero already), active[c], and the active count (*cnt, zeroed by the caller) to ctl[0].
template <class Zero>
__device__ __forceinline__ void cg_close_mode(const KrylovState &S, int nc, int act, int stop, int it, int *cnt, Zero zero) {
  if (threadIdx.x < nc) {
    const int c = threadIdx.x;
    if (stop >= 0) S.flag[c] = stop, S.iter[c] = it, act = 0;
    if (!act) zero(c);
    S.active[c] = act;
    if (act) atomicAdd(cnt, 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) S.ctl[0] = *cnt;
}

// Sums the kCgBlocks partials of every column (cg_sum_partials) and does the per-column scalar work of step k:
//   mode 0: ||b||: the state; a zero column is done (x = 0, flag 0, 0 iterations)
//   mode 1: rho = r^H z of the start                                   (not positive: flag 1, 0 iterations)
//   mode 2: sigma = p^H A p: alpha = rho / sigma                       (not positive: flag 1, k iterations)
//   mode 3: |r|^2 after the update: ||r|| / ||b|| <= rtol -> flag 0, k + 1 iterations; k + 1 == maxit -> flag 2
//   mode 4: rho' = r^H z: beta = rho' / rho, rho = rho'                (not positive: flag 1, k + 1 iterations)
// A column that stops gets alpha = beta = 0 and active = 0; ctl[0] = columns still active.
template <class T>
__global__ void __launch_bounds__(1024) k_cg_finish(const T *__restrict__ partial, int nc, int mode, int k, CgState<T> S) {
  __shared__ T sm[16 * 64];
  __shared__ int cnt;
  const int c = threadIdx.x & 63;
  if (threadIdx.x == 0) cnt = 0;
  const T tot = cg_sum_partials(partial, nc, sm);
  int act = 0, stop = -1, it = 0;  // stop, it: flag and iterations of a column that stops here
  if (threadIdx.x < nc) {
    act = S.active[c];
    if (mode == 0) {
      const double bn = sqrt(vreal(tot));
      S.bnorm[c] = bn;
      S.iter[c] = 0;
      S.flag[c] = 0;
      S.alpha[c] = vzero(T());
      S.beta[c] = vzero(T());
      act = !(bn == 0.0);
    } else if (act && mode == 1) {
      if (cg_bad(tot)) stop = 1, it = 0;
      else S.rho[c] = tot;
    } else if (act && mode == 2) {
      if (cg_bad(tot)) stop = 1, it = k;
      else S.alpha[c] = vdiv(S.rho[c], tot);
    } else if (act && mode == 3) {
      if (sqrt(vreal(tot)) / S.bnorm[c] <= S.rtol) stop = 0, it = k + 1;
      else if (k + 1 >= S.maxit) stop = 2, it = S.maxit;
    } else if (act && mode == 4) {
      if (cg_bad(tot)) {
        stop = 1, it = k + 1;
      } else {
        S.beta[c] = vdiv(tot, S.rho[c]);
        S.rho[c] = tot;
      }
    }
  }
  cg_close_mode(S, nc, act, stop, it, &cnt, [&](int c) { S.alpha[c] = S.beta[c] = vzero(T()); });
}

// ---------------------------------------------------------------------------------------------
// Device-resident right-preconditioned BiCGSTAB with x0 = 0 and r^ = b, up to 64 columns in lock step
// (Engine::bicgstab_tile).  Same layout and row walk as k_cg_*: vectors [n][nc] (r^ is b itself, row stride ldh),
// lane = column, wave w of block b owns the rows i = 4 b + w + k * 4 kCgBlocks, wave partials added in wave order and
// the kCgBlocks block partials of a column in k_cg_finish's order by k_bs_finish; a column's bits do not depend on
// the batch it travels in.  A step is one M^{-1} apply plus one SpMM; one iteration is two steps.
// ---------------------------------------------------------------------------------------------
template <class T>
struct BsState : KrylovState {  // (iter counts steps)
  T *rho, *alpha, *omega, *beta;  // [64]  (r^, r), rho / (r^, v), (t, r) / (t, t), (rho' / rho)(alpha / omega); 0 when frozen
};

// the block's shares of (t, r) = sum conj(t_i) r_i and (t, t) = sum |t_i|^2, one read of t and r
template <class T>
__global__ void __launch_bounds__(256) k_bs_tr(int64_t n, int nc, const T *__restrict__ t, const T *__restrict__ r,
                                               T *__restrict__ part_tr, T *__restrict__ part_tt) {
  __shared__ T sm[512];
  const int c = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  T tr = vzero(T()), tt = vzero(T());
  if (c < nc)
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += stride) {
      const T ti = t[i * nc + c];
      tr = vadd(tr, vmul(vconj(ti), r[i * nc + c]));
      tt = vadd(tt, vfromreal(vabs2(ti), T()));
    }
  cg_block_partial(tr, sm, part_tr);
  cg_block_partial(tt, sm + 256, part_tt);
}

// full step on the active columns: x += omega y, r -= omega t, fused with the block's shares of |r|^2 and (r^, r)
template <class T>
__global__ void __launch_bounds__(256) k_bs_xr_full(int64_t n, int nc, T *__restrict__ x, int64_t ldx, T *__restrict__ r,
                                                    const T *__restrict__ y, const T *__restrict__ t,
                                                    const T *__restrict__ rh, int64_t ldh, BsState<T> S,
                                                    T *__restrict__ part_rr, T *__restrict__ part_hr) {
  __shared__ T sm[512];
  const int c = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  T rr = vzero(T()), hr = vzero(T());
  if (c < nc) {
    const bool act = S.active[c] != 0;
    const T om = S.omega[c];
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += stride) {
      T ri = r[i * nc + c];
      if (act) {
        x[i * ldx + c] = vadd(x[i * ldx + c], vmul(om, y[i * nc + c]));
        ri = vsub(ri, vmul(om, t[i * nc + c]));
        r[i * nc + c] = ri;
      }
      rr = vadd(rr, vfromreal(vabs2(ri), T()));
      hr = vadd(hr, vmul(vconj(rh[i * ldh + c]), ri));
    }
  }
  cg_block_partial(rr, sm, part_rr);
  cg_block_partial(hr, sm + 256, part_hr);
}

// p = r + beta (p - omega v) on the active columns
template <class T>
__global__ void __launch_bounds__(256) k_bs_p(int64_t n, int nc, T *__restrict__ p, const T *__restrict__ r,
                                              const T *__restrict__ v, BsState<T> S) {
  const int c = threadIdx.x & 63;
  if (c >= nc || !S.active[c]) return;
  const T be = S.beta[c], om = S.omega[c];
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += stride)
    p[i * nc + c] = vadd(r[i * nc + c], vmul(be, vsub(p[i * nc + c], vmul(om, v[i * nc + c]))));
}

// a BiCGSTAB breakdown value: exactly zero or not finite
__device__ __forceinline__ bool bs_bad(double v) { return v == 0.0 || !isfinite(v); }
__device__ __forceinline__ bool bs_bad(cplx v) { return (v.x == 0.0 && v.y == 0.0) || !isfinite(v.x) || !isfinite(v.y); }

// Sums the kCgBlocks partials of every column of p0 (and of p1 when given; cg_sum_partials) and does the
// per-column scalar work of iteration k (steps 2k + 1 and 2k + 2):
//   mode 0: p0 = ||b||^2: ||b||, rho = ||b||^2; b = 0 is done (x = 0, flag 0, 0 steps); rho bad: flag 1, 0 steps
//   mode 1: p0 = (r^, v): alpha = rho / (r^, v)                                   (bad: flag 1, 2k + 1 steps)
//   mode 2: p0 = |s|^2: ||s|| / ||b|| <= rtol -> flag 0, 2k + 1 steps; 2k + 1 >= maxit -> flag 2
//   mode 3: p0 = (t, r), p1 = (t, t): omega = (t, r) / (t, t)          ((t, t) or omega bad: flag 1, 2k + 2 steps)
//   mode 4: p0 = |r|^2, p1 = rho' = (r^, r): ||r|| / ||b|| <= rtol -> flag 0, 2k + 2 steps; 2k + 2 >= maxit -> flag 2;
//           rho' bad -> flag 1, 2k + 2 steps; else beta = (rho' / rho)(alpha / omega), rho = rho'
// A column that stops gets rho = alpha = omega = beta = 0 and active = 0; ctl[0] = columns still active.
template <class T>
__global__ void __launch_bounds__(1024) k_bs_finish(const T *__restrict__ p0, const T *__restrict__ p1, int nc, int mode,
                                                    int k, BsState<T> S) {
  __shared__ T sm0[16 * 64], sm1[16 * 64];
  __shared__ int cnt;
  const int c = threadIdx.x & 63;
  if (threadIdx.x == 0) cnt = 0;
  const T t0 = cg_sum_partials(p0, nc, sm0), t1 = cg_sum_partials(p1, nc, sm1);
  int act = 0, stop = -1, it = 0;  // stop, it: flag and steps of a column that stops here
  if (threadIdx.x < nc) {
    act = S.active[c];
    if (mode == 0) {
      const double bn = sqrt(vreal(t0));
      S.bnorm[c] = bn;
      S.iter[c] = 0;
      S.flag[c] = 0;
      act = !(bn == 0.0);
      if (act && bs_bad(t0)) stop = 1, it = 0;
      else S.rho[c] = t0;
    } else if (act && mode == 1) {
      if (bs_bad(t0)) stop = 1, it = 2 * k + 1;
      else S.alpha[c] = vdiv(S.rho[c], t0);
    } else if (act && mode == 2) {
      if (sqrt(vreal(t0)) / S.bnorm[c] <= S.rtol) stop = 0, it = 2 * k + 1;
      else if (2 * k + 1 >= S.maxit) stop = 2, it = S.maxit;
    } else if (act && mode == 3) {
      const T om = vdiv(t0, t1);
      if (bs_bad(t1) || bs_bad(om)) stop = 1, it = 2 * k + 2;
      else S.omega[c] = om;
    } else if (act && mode == 4) {
      if (sqrt(vreal(t0)) / S.bnorm[c] <= S.rtol) {
        stop = 0, it = 2 * k + 2;
      } else if (2 * k + 2 >= S.maxit) {
        stop = 2, it = S.maxit;
      } else if (bs_bad(t1)) {
        stop = 1, it = 2 * k + 2;
      } else {
        S.beta[c] = vmul(vdiv(t1, S.rho[c]), vdiv(S.alpha[c], S.omega[c]));
        S.rho[c] = t1;
      }
    }
  }
  cg_close_mode(S, nc, act, stop, it, &cnt,
                [&](int c) { S.rho[c] = S.alpha[c] = S.omega[c] = S.beta[c] = vzero(T()); });
}

// ---------------------------------------------------------------------------------------------
// Device-resident symmetric QMR (Freund / Nachtigal) for a Hermitian INDEFINITE pair (A, M) with x0 = 0, up to 64
// columns in lock step (Engine::sqmr_tile): PCG's coupled two-term recurrence without the positivity requirement, plus
// the quasi-minimal-residual smoothing of the iterates (d, g, x, s; s = b - A x by recurrence).  Same layout and row walk
// as k_cg_*: vectors [n][nc], lane = column, wave w of block b owns the rows i = 4 b + w + k * 4 kCgBlocks, wave
// partials added in wave order and the kCgBlocks block partials of a column in k_cg_finish's order by k_qm_finish; a
// column's bits do not depend on the batch it travels in.  k_cg_dot and k_cg_p serve the inner products and p = z + beta p.
// ---------------------------------------------------------------------------------------------
template <class T>
struct QmState : KrylovState {
  T *rho, *alpha, *beta, *zeta;  // [64]  r^H z, rho / sigma, rho' / rho, c^2 alpha (0 for a frozen column)
  double *eta, *tau, *theta;     // [64]  c^2 theta_old^2, the quasi-residual norm, ||r|| / tau_old
};

// a where the column is active, b where it is frozen (component by component: no branch, no stack object)
__device__ __forceinline__ double qm_sel(bool act, double a, double b) { return act ? a : b; }
__device__ __forceinline__ cplx qm_sel(bool act, cplx a, cplx b) { return cplx{act ? a.x : b.x, act ? a.y : b.y}; }

// r -= alpha q on the active columns, fused with the block's share of |r|^2: two vectors read, one written.  Every
// access is unconditional (a frozen column stores back the bits it loaded), so the pass stays pipelined.
template <class T>
__global__ void __launch_bounds__(256) k_qm_r(int64_t n, int nc, T *__restrict__ r, const T *__restrict__ q,
                                              const T *__restrict__ alpha, const int *__restrict__ active,
                                              T *__restrict__ partial /* [kCgBlocks][64] */) {
  __shared__ T sm[256];
  const int c = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  T acc = vzero(T());
  if (c < nc) {
    const bool act = active[c] != 0;
    const T al = alpha[c];
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += stride) {
      const T r0 = r[i * nc + c], qi = q[i * nc + c];
      const T r1 = vsub(r0, vmul(al, qi));
      const T ri = qm_sel(act, r1, r0);
      r[i * nc + c] = ri;
      acc = vadd(acc, vfromreal(vabs2(ri), T()));
    }
  }
  cg_block_partial(acc, sm, partial);
}

// d = eta d + zeta p, g = eta g + zeta q, x += d, s -= g on the active columns, fused with the block's share of |s|^2
// (x: row stride ldx): six vectors read, four written, each element once.  Unconditional accesses as in k_qm_r.
template <class T>
__global__ void __launch_bounds__(256) k_qm_ds(int64_t n, int nc, T *__restrict__ x, int64_t ldx, T *__restrict__ s,
                                               T *__restrict__ d, T *__restrict__ g, const T *__restrict__ p,
                                               const T *__restrict__ q, QmState<T> S,
                                               T *__restrict__ partial /* [kCgBlocks][64] */) {
  __shared__ T sm[256];
  const int c = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  T acc = vzero(T());
  if (c < nc) {
    const bool act = S.active[c] != 0;
    const double et = S.eta[c];
    const T ze = S.zeta[c];
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += stride) {
      const int64_t e = i * nc + c, ex = i * ldx + c;
      const T d0 = d[e], g0 = g[e], pi = p[e], qi = q[e], x0 = x[ex], s0 = s[e];
      const T d1 = vadd(vscale(et, d0), vmul(ze, pi));
      const T g1 = vadd(vscale(et, g0), vmul(ze, qi));
      const T si = qm_sel(act, vsub(s0, g1), s0);
      d[e] = qm_sel(act, d1, d0);
      g[e] = qm_sel(act, g1, g0);
      x[ex] = qm_sel(act, vadd(x0, d1), x0);
      s[e] = si;
      acc = vadd(acc, vfromreal(vabs2(si), T()));
    }
  }
  cg_block_partial(acc, sm, partial);
}

// Sums the kCgBlocks partials of every column (cg_sum_partials) and does the per-column scalar work of iteration k.
// alpha and beta are formed as k_cg_finish modes 1, 2 and 4 form them; a breakdown value is exactly zero or not finite
// (bs_bad), with no sign test:
//   mode 0: ||b||: the state, tau = ||b||, theta = 0; a zero column is done (x = 0, flag 0, 0 iterations)
//   mode 1: rho = r^H z of the start                                   (bad: flag 1, 0 iterations)
//   mode 2: sigma = p^H A p: alpha = rho / sigma                       (bad: flag 1, k iterations)
//   mode 3: |r|^2 after r -= alpha q: theta' = ||r|| / tau, c^2 = 1 / (1 + theta'^2), tau = tau theta' sqrt(c^2),
//           eta = c^2 theta^2, zeta = c^2 alpha, theta = theta'
//   mode 4: |s|^2 after the smoothed update: ||s|| / ||b|| <= rtol -> flag 0, k + 1 iterations; k + 1 == maxit -> flag 2
//   mode 5: rho' = r^H z: beta = rho' / rho, rho = rho'                (bad: flag 1, k + 1 iterations)
// A column that stops gets alpha = beta = zeta = eta = 0 and active = 0; ctl[0] = columns still active.
template <class T>
__global__ void __launch_bounds__(1024) k_qm_finish(const T *__restrict__ partial, int nc, int mode, int k, QmState<T> S) {
  __shared__ T sm[16 * 64];
  __shared__ int cnt;
  const int c = threadIdx.x & 63;
  if (threadIdx.x == 0) cnt = 0;
  const T tot = cg_sum_partials(partial, nc, sm);
  int act = 0, stop = -1, it = 0;  // stop, it: flag and iterations of a column that stops here
  if (threadIdx.x < nc) {
    act = S.active[c];
    if (mode == 0) {
      const double bn = sqrt(vreal(tot));
      S.bnorm[c] = bn;
      S.tau[c] = bn;
      S.theta[c] = 0.0;
      S.eta[c] = 0.0;
      S.iter[c] = 0;
      S.flag[c] = 0;
      S.alpha[c] = vzero(T());
      S.beta[c] = vzero(T());
      S.zeta[c] = vzero(T());
      act = !(bn == 0.0);
    } else if (act && mode == 1) {
      if (bs_bad(tot)) stop = 1, it = 0;
      else S.rho[c] = tot;
    } else if (act && mode == 2) {
      if (bs_bad(tot)) stop = 1, it = k;
      else S.alpha[c] = vdiv(S.rho[c], tot);
    } else if (act && mode == 3) {
      const double th0 = S.theta[c], ta = S.tau[c];
      const double th = sqrt(vreal(tot)) / ta;
      const double c2 = 1.0 / (1.0 + th * th);
      S.tau[c] = ta * th * sqrt(c2);
      S.eta[c] = c2 * th0 * th0;
      S.zeta[c] = vscale(c2, S.alpha[c]);
      S.theta[c] = th;
    } else if (act && mode == 4) {
      if (sqrt(vreal(tot)) / S.bnorm[c] <= S.rtol) stop = 0, it = k + 1;
      else if (k + 1 >= S.maxit) stop = 2, it = S.maxit;
    } else if (act && mode == 5) {
      if (bs_bad(tot)) {
        stop = 1, it = k + 1;
      } else {
        S.beta[c] = vdiv(tot, S.rho[c]);
        S.rho[c] = tot;
      }
    }
  }
  cg_close_mode(S, nc, act, stop, it, &cnt, [&](int c) {
    S.alpha[c] = S.beta[c] = S.zeta[c] = vzero(T());
    S.eta[c] = 0.0;
  });
}

// ---------------------------------------------------------------------------------------------
// Basis mode of the null-space filter (Engine::apply_nsp): every column x of a 64-column tile becomes x - Q (Q^H x),
// Q [n][K] orthonormal (K = the basis padded with zero vectors to 1, 2, 4, 8 or 16, a compile-time size so that the K
// accumulators stay in registers).  Three launches: k_nsp_coef (block partials of C = Q^H X), k_nsp_finish (one
// workgroup per basis vector adds them), k_nsp_sub (x_i -= sum_j q_ij c_j).  Same row walk and reduction order as
// k_cg_dot / k_cg_finish: lane = column, wave w of block b owns the rows i = 4 b + w + k * 4 kCgBlocks, wave partials
// added in wave order, block partials in k_cg_finish's order; nothing depends on nc or on the other columns, so a
// column's bits are the same alone and in any batch.  The row of Q is the same for all lanes of a wave: the row
// index is made provably uniform (readfirstlane) so that it is fetched by scalar loads.  X has a row stride (ldx).
// ---------------------------------------------------------------------------------------------
constexpr int kNspMax = 16;  // HIFAMD_NSP_MAX

__device__ __forceinline__ int nsp_wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// acc[j] += conj(q[j]) x, q the (wave-uniform) row of Q
template <class T, int K>
__device__ __forceinline__ void nsp_acc_row(T (&acc)[K], const T *__restrict__ q, T xi) {
#pragma unroll
  for (int j = 0; j < K; ++j) acc[j] = vadd(acc[j], vmul(vconj(q[j]), xi));
}
// sum_j q[j] c[j], j ascending
template <class T, int K>
__device__ __forceinline__ T nsp_row_dot(const T *__restrict__ q, const T (&cj)[K]) {
  T s = vmul(q[0], cj[0]);
#pragma unroll
  for (int j = 1; j < K; ++j) s = vadd(s, vmul(q[j], cj[j]));
  return s;
}

template <class T, int K>
__global__ void __launch_bounds__(256) k_nsp_coef(int64_t n, int nc, const T *__restrict__ x, int64_t ldx,
                                                  const T *__restrict__ Q /* [n][K] */,
                                                  T *__restrict__ partial /* [K][kCgBlocks][64] */) {
  __shared__ T sm[2][256];
  const int c = threadIdx.x & 63, w = nsp_wave_id();
  const int64_t stride = (int64_t)kCgBlocks * 4;
  T acc[K];
#pragma unroll
  for (int j = 0; j < K; ++j) acc[j] = vzero(T());
  if (c < nc) {
    // four rows per trip so that four loads of x are in flight (eight measured slower); the rows are still
    // accumulated in walk order
    int64_t i = (int64_t)blockIdx.x * 4 + w;
    for (; i + 3 * stride < n; i += 4 * stride) {
      const T x0 = x[i * ldx + c], x1 = x[(i + stride) * ldx + c], x2 = x[(i + 2 * stride) * ldx + c],
              x3 = x[(i + 3 * stride) * ldx + c];
      nsp_acc_row<T, K>(acc, Q + i * K, x0);
      nsp_acc_row<T, K>(acc, Q + (i + stride) * K, x1);
      nsp_acc_row<T, K>(acc, Q + (i + 2 * stride) * K, x2);
      nsp_acc_row<T, K>(acc, Q + (i + 3 * stride) * K, x3);
    }
    for (; i < n; i += stride) nsp_acc_row<T, K>(acc, Q + i * K, x[i * ldx + c]);
  }
  // the four wave partials of every basis vector in wave order (cg_block_partial's pattern, two LDS planes in turn)
#pragma unroll
  for (int j = 0; j < K; ++j) {
    T *s = sm[j & 1];
    s[threadIdx.x] = acc[j];
    __syncthreads();
    if (threadIdx.x < 64)
      partial[((int64_t)j * kCgBlocks + blockIdx.x) * 64 + c] = vadd(vadd(vadd(s[c], s[64 + c]), s[128 + c]), s[192 + c]);
  }
}

// C[j][c] = the kCgBlocks partials of basis vector j = blockIdx.x in k_cg_finish's order (wave w takes blocks w, w + 16,
// ..., then the 16 wave sums in wave order); all 64 columns, a column beyond nc holds zeros
template <class T>
__global__ void __launch_bounds__(1024) k_nsp_finish(const T *__restrict__ partial, T *__restrict__ C /* [K][64] */) {
  __shared__ T sm[16 * 64];
  const int w = threadIdx.x >> 6, c = threadIdx.x & 63;
  const T *__restrict__ p = partial + (int64_t)blockIdx.x * kCgBlocks * 64;
  T acc = vzero(T());
  for (int b = w; b < kCgBlocks; b += 16) acc = vadd(acc, p[(int64_t)b * 64 + c]);
  sm[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < 64) {
    T tot = vzero(T());
    for (int v = 0; v < 16; ++v) tot = vadd(tot, sm[v * 64 + c]);
    C[(int64_t)blockIdx.x * 64 + c] = tot;
  }
}

// x_i -= sum_j q_ij c_j, j ascending, the sum formed first and subtracted once
template <class T, int K>
__global__ void __launch_bounds__(256) k_nsp_sub(int64_t n, int nc, T *__restrict__ x, int64_t ldx,
                                                 const T *__restrict__ Q /* [n][K] */, const T *__restrict__ C /* [K][64] */) {
  const int c = threadIdx.x & 63, w = nsp_wave_id();
  if (c >= nc) return;
  T cj[K];
#pragma unroll
  for (int j = 0; j < K; ++j) cj[j] = C[j * 64 + c];
  const int64_t stride = (int64_t)kCgBlocks * 4;
  int64_t i = (int64_t)blockIdx.x * 4 + w;
  for (; i + 3 * stride < n; i += 4 * stride) {  // (four rows per trip: four loads of x in flight)
    T *p0 = x + i * ldx + c, *p1 = x + (i + stride) * ldx + c, *p2 = x + (i + 2 * stride) * ldx + c,
      *p3 = x + (i + 3 * stride) * ldx + c;
    const T x0 = *p0, x1 = *p1, x2 = *p2, x3 = *p3;
    *p0 = vsub(x0, nsp_row_dot<T, K>(Q + i * K, cj));
    *p1 = vsub(x1, nsp_row_dot<T, K>(Q + (i + stride) * K, cj));
    *p2 = vsub(x2, nsp_row_dot<T, K>(Q + (i + 2 * stride) * K, cj));
    *p3 = vsub(x3, nsp_row_dot<T, K>(Q + (i + 3 * stride) * K, cj));
  }
  for (; i < n; i += stride) x[i * ldx + c] = vsub(x[i * ldx + c], nsp_row_dot<T, K>(Q + i * K, cj));
}

// ---------------------------------------------------------------------------------------------
// Null-space search (Engine::nsp_find): the probe block and the 16 x 16 right-multiplication of an [n][16] block.
// The Gram matrix V^H V is k_nsp_coef<T, 16> + k_nsp_finish with Q = X = V (the fixed-order reduction above).
// ---------------------------------------------------------------------------------------------
// The counter-based probe generator that include/hifir_amd.h defines (import.hpp nsp_probe_value is its host twin):
// z = seed + 0x9E3779B97F4A7C15 * counter (mod 2^64), the splitmix64 finalizer, u = (z >> 11) 2^-53, value 2u - 1.
__device__ __forceinline__ double probe_value(uint64_t seed, uint64_t counter) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * counter;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return 2.0 * ((double)(z >> 11) * 0x1.0p-53) - 1.0;  // (both steps exact or correctly rounded: no contraction issue)
}

// X [n][16] contiguous: entry (i, j) from counter 16 i + j + 1, the imaginary part of a complex entry from
// counter 16 (n + i) + j + 1.  One pass, consecutive lanes write consecutive entries.
template <class T>
__global__ void __launch_bounds__(256) k_probe_fill(int64_t n, uint64_t seed, T *__restrict__ x) {
  const int64_t total = n * kNspMax;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (std::is_same<T, cplx>::value)
      x[e] = cplx{probe_value(seed, (uint64_t)e + 1), probe_value(seed, (uint64_t)(total + e) + 1)};
    else
      x[e] = probe_value(seed, (uint64_t)e + 1);
  }
}

// ---------------------------------------------------------------------------------------------
// Device-resident right-preconditioned IDR(s) with biorthogonalization (van Gijzen / Sonneveld, ACM TOMS 38(1), 2011)
// and x0 = 0, up to 64 columns in lock step (Engine::idrs_tile).  Same layout and row walk as k_cg_*: vectors [n][nc],
// lane = column, wave w of block b owns the rows i = 4 b + w + k * 4 kCgBlocks, wave partials added in wave order and the
// kCgBlocks block partials of a column in k_cg_finish's order by k_idr_finish; a column's bits do not depend on the batch
// it travels in.  The shadow block P is [n][K], K = s padded with zero columns to 1, 2, 4 or 8, shared by all columns:
// P^H r and P^H g are k_nsp_coef<T, K> + k_nsp_finish as they stand.  (t, r) and (t, t) are k_bs_tr, the omega update is
// k_cg_xr.  A step is one M^{-1} apply plus one SpMM; a cycle is s + 1 steps.
// ---------------------------------------------------------------------------------------------
constexpr int kIdrMax = 8;  // HIFAMD_IDRS_MAX

template <class T>
struct IdState : KrylovState {  // (iter counts steps)
  T *M;               // [s][s][64]  M[i][l] = p_i^H g_l (lower triangle in use; the identity at the start)
  T *f, *c, *alpha;   // [s][64]     P^H r as the cycle updates it, the combination coefficients, the biorthogonalization's
  T *omega, *beta;    // [64]        (beta: 0 for a frozen column)
  double *rr;         // [64]        ||r||^2 at the last stopping test (||b||^2 at the start)
  int s;
};

// a run of S work vectors of the pool (each [n][nc]) as a kernel argument
template <class T, int S>
struct IdRun {
  T *w[S > 0 ? S : 1];
};

// y = z - sum_j c_j W_j (U false: v from r and G_k ..) or y = omega z + sum_j c_j W_j (U true: u from v^ and U_k ..), the sum
// over the S vectors of the run formed first, j ascending.  The S loads of a row are unconditional, the coefficients stay
// in registers, every input is read once and y written once; y may be W_0 itself (u goes to U_k in place).
template <class T, int S, bool U>
__global__ void __launch_bounds__(256) k_idr_comb(int64_t n, int nc, T *y, const T *z, IdRun<T, S> W,
                                                  const T *__restrict__ coef /* [S][64] */, const T *__restrict__ omega) {
  const int c = threadIdx.x & 63;
  if (c >= nc) return;
  T cj[S];
#pragma unroll
  for (int j = 0; j < S; ++j) cj[j] = coef[j * 64 + c];
  const T om = U ? omega[c] : vzero(T());
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += stride) {
    T wv[S];
#pragma unroll
    for (int j = 0; j < S; ++j) wv[j] = W.w[j][i * nc + c];
    const T zi = z[i * nc + c];
    T acc = vmul(cj[0], wv[0]);
#pragma unroll
    for (int j = 1; j < S; ++j) acc = vadd(acc, vmul(cj[j], wv[j]));
    y[i * nc + c] = U ? vadd(vmul(om, zi), acc) : vsub(zi, acc);
  }
}

// The fused pass after the recursion of step k = S on the active columns: g_k -= sum_{l<k} alpha_l g_l,
// u_k -= sum_{l<k} alpha_l u_l (each sum formed first, l ascending), r -= beta g_k, x += beta u_k (x: row stride ldx), with
// the block's share of |r|^2.  All loads of a row are unconditional; a frozen column is not written (k_cg_xr's use of active).
template <class T, int S>
__global__ void __launch_bounds__(256) k_idr_gu(int64_t n, int nc, T *__restrict__ x, int64_t ldx, T *__restrict__ r,
                                                T *__restrict__ gk, T *__restrict__ uk, IdRun<T, S> G, IdRun<T, S> U,
                                                IdState<T> St, T *__restrict__ partial /* [kCgBlocks][64] */) {
  __shared__ T sm[256];
  const int c = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  T acc = vzero(T());
  if (c < nc) {
    const bool act = St.active[c] != 0;
    const T be = St.beta[c];
    T al[S > 0 ? S : 1];
#pragma unroll
    for (int l = 0; l < S; ++l) al[l] = St.alpha[l * 64 + c];
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += stride) {
      T gv[S > 0 ? S : 1], uv[S > 0 ? S : 1];
#pragma unroll
      for (int l = 0; l < S; ++l) gv[l] = G.w[l][i * nc + c], uv[l] = U.w[l][i * nc + c];
      T gi = gk[i * nc + c], ui = uk[i * nc + c], ri = r[i * nc + c];
      const T xi = x[i * ldx + c];
      if (act) {
        if constexpr (S > 0) {
          T ag = vmul(al[0], gv[0]), au = vmul(al[0], uv[0]);
#pragma unroll
          for (int l = 1; l < S; ++l) ag = vadd(ag, vmul(al[l], gv[l])), au = vadd(au, vmul(al[l], uv[l]));
          gi = vsub(gi, ag);
          ui = vsub(ui, au);
          gk[i * nc + c] = gi;
          uk[i * nc + c] = ui;
        }
        ri = vsub(ri, vmul(be, gi));
        r[i * nc + c] = ri;
        x[i * ldx + c] = vadd(xi, vmul(be, ui));
      }
      acc = vadd(acc, vfromreal(vabs2(ri), T()));
    }
  }
  cg_block_partial(acc, sm, partial);
}

// c_k .. c_{s-1} of column c by forward substitution on the lower triangle M[k:, k:] c = f[k:]
template <class T>
__device__ __forceinline__ void idr_forward(const IdState<T> &S, int c, int k) {
  const int s = S.s;
  for (int i = k; i < s; ++i) {
    T v = S.f[i * 64 + c];
    for (int l = k; l < i; ++l) v = vsub(v, vmul(S.M[(i * s + l) * 64 + c], S.c[l * 64 + c]));
    S.c[i * 64 + c] = vdiv(v, S.M[(i * s + i) * 64 + c]);
  }
}

constexpr double kIdrKappa = 0.7;  // the "maintaining convergence" bound on the cosine of t and r

// Sums the kCgBlocks partials of every column of p0 (and of p1 when given; cg_sum_partials) and does the per-column scalar
// work; step counts the steps completed before this one, k is the position in the cycle, C [K][64] what k_nsp_finish left:
//   mode 0: p0 = ||b||^2: ||b||, omega = 1, M = I; b = 0 is done (x = 0, flag 0, 0 steps); not finite: flag 1, 0 steps
//   mode 1: C = P^H r: f = C, c = the forward substitution from row 0
//   mode 2: C = P^H g: alpha_i = (C_i - sum_{l<i} alpha_l M[i,l]) / M[i,i] (i < k), M[i,k] = C_i - sum_{l<k} alpha_l M[i,l]
//           (i >= k); M[k,k] zero or not finite: flag 1, step + 1 steps; else beta = f_k / M[k,k], f_i = 0 (i <= k),
//           f_i -= beta M[i,k] (i > k), and c = the forward substitution from row k + 1
//   mode 3: p0 = |r|^2: ||r|| / ||b|| <= rtol -> flag 0, step + 1 steps; step + 1 >= maxit -> flag 2
//   mode 4: p0 = (t, r), p1 = (t, t): either zero or not finite: flag 1, step + 1 steps; else omega = (t, r) / (t, t),
//           rho = |(t, r)| / (||t|| ||r||), rho < kappa: omega *= kappa / rho
// A column that stops gets beta = 0 and active = 0; ctl[0] = columns still active.
template <class T>
__global__ void __launch_bounds__(1024) k_idr_finish(const T *__restrict__ p0, const T *__restrict__ p1,
                                                     const T *__restrict__ C, int nc, int mode, int k, int step,
                                                     IdState<T> S) {
  __shared__ T sm0[16 * 64], sm1[16 * 64];
  __shared__ int cnt;
  const int c = threadIdx.x & 63, s = S.s;
  if (threadIdx.x == 0) cnt = 0;
  const T t0 = cg_sum_partials(p0, nc, sm0), t1 = cg_sum_partials(p1, nc, sm1);
  int act = 0, stop = -1, it = 0;  // stop, it: flag and steps of a column that stops here
  if (threadIdx.x < nc) {
    act = S.active[c];
    if (mode == 0) {
      const double bn = sqrt(vreal(t0));
      S.bnorm[c] = bn;
      S.rr[c] = vreal(t0);
      S.iter[c] = 0;
      S.flag[c] = 0;
      S.omega[c] = vfromreal(1.0, T());
      for (int i = 0; i < s; ++i) S.M[(i * s + i) * 64 + c] = vfromreal(1.0, T());  // (the state arrives zeroed)
      act = !(bn == 0.0);
      if (act && bs_bad(t0)) stop = 1, it = 0;
    } else if (act && mode == 1) {
      for (int i = 0; i < s; ++i) S.f[i * 64 + c] = C[i * 64 + c];
      idr_forward(S, c, 0);
    } else if (act && mode == 2) {
      for (int i = 0; i < k; ++i) {
        T a = C[i * 64 + c];
        for (int l = 0; l < i; ++l) a = vsub(a, vmul(S.alpha[l * 64 + c], S.M[(i * s + l) * 64 + c]));
        S.alpha[i * 64 + c] = vdiv(a, S.M[(i * s + i) * 64 + c]);
      }
      for (int i = k; i < s; ++i) {
        T m = C[i * 64 + c];
        for (int l = 0; l < k; ++l) m = vsub(m, vmul(S.alpha[l * 64 + c], S.M[(i * s + l) * 64 + c]));
        S.M[(i * s + k) * 64 + c] = m;
      }
      const T mkk = S.M[(k * s + k) * 64 + c];
      if (bs_bad(mkk)) {
        stop = 1, it = step + 1;
      } else {
        const T be = vdiv(S.f[k * 64 + c], mkk);
        S.beta[c] = be;
        for (int i = 0; i <= k; ++i) S.f[i * 64 + c] = vzero(T());
        for (int i = k + 1; i < s; ++i) S.f[i * 64 + c] = vsub(S.f[i * 64 + c], vmul(be, S.M[(i * s + k) * 64 + c]));
        idr_forward(S, c, k + 1);
      }
    } else if (act && mode == 3) {
      S.rr[c] = vreal(t0);
      if (sqrt(vreal(t0)) / S.bnorm[c] <= S.rtol) stop = 0, it = step + 1;
      else if (step + 1 >= S.maxit) stop = 2, it = S.maxit;
    } else if (act && mode == 4) {
      if (bs_bad(t1) || bs_bad(t0)) {
        stop = 1, it = step + 1;
      } else {
        T om = vdiv(t0, t1);
        const double rho = vabs1(t0) / (sqrt(vreal(t1)) * sqrt(S.rr[c]));
        if (rho < kIdrKappa) om = vscale(kIdrKappa / rho, om);
        S.omega[c] = om;
      }
    }
  }
  cg_close_mode(S, nc, act, stop, it, &cnt, [&](int c) { S.beta[c] = vzero(T()); });
}

// The generated shadow block P [n][K]: entry (i, j), j < s, from counter 16 i + j + 1 (the imaginary part of a complex entry
// from counter 16 (n + i) + j + 1), the first s columns of k_probe_fill's block for the same seed; columns s .. K-1 zero.
template <class T>
__global__ void __launch_bounds__(256) k_idr_pfill(int64_t n, int s, int K, uint64_t seed, T *__restrict__ P) {
  const int64_t total = n * K;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / K;
    const int j = (int)(e - i * K);
    double re = 0.0, im = 0.0;
    if (j < s) {
      re = probe_value(seed, (uint64_t)(kNspMax * i + j) + 1);
      if constexpr (std::is_same<T, cplx>::value) im = probe_value(seed, (uint64_t)(kNspMax * (n + i) + j) + 1);
    }
    if constexpr (std::is_same<T, cplx>::value)
      P[e] = cplx{re, im};
    else
      P[e] = re;
  }
}

// V <- V C in place, V [n][16] contiguous, C [16][16] row-major (v_new[i][c] = sum_j v[i][j] C[j][c], j ascending).
// One row per 16 lanes: a wave moves four rows (512 B real, 1 KB complex) per access, lane c of a group keeps column c
// of C in registers for the whole kernel (read once, 32 / 64 VGPRs) and gets the 16 values of its row from the other
// lanes of its group by shuffles, so every entry of V is loaded once and stored once: HBM-bound, 256 FMA per row.
// Every wave runs the same number of trips with all lanes alive (rows beyond n are loaded as zero and not stored).
template <class T>
__global__ void __launch_bounds__(256) k_blk_rmul(int64_t n, T *__restrict__ v, const T *__restrict__ C) {
  const int c = threadIdx.x & 15;
  T cc[kNspMax];
#pragma unroll
  for (int j = 0; j < kNspMax; ++j) cc[j] = C[j * kNspMax + c];
  const int64_t step = (int64_t)gridDim.x * 16;
  for (int64_t base = (int64_t)blockIdx.x * 16; base < n; base += step) {  // (uniform over the block)
    const int64_t i = base + (threadIdx.x >> 4);
    const bool live = i < n;
    const T mine = live ? v[i * kNspMax + c] : vzero(T());
    T acc = vzero(T());
#pragma unroll
    for (int j = 0; j < kNspMax; ++j) {
      T vj;
      if constexpr (std::is_same<T, cplx>::value)
        vj = cplx{__shfl(mine.x, j, 16), __shfl(mine.y, j, 16)};
      else
        vj = __shfl(mine, j, 16);
      acc = vadd(acc, vmul(vj, cc[j]));
    }
    if (live) v[i * kNspMax + c] = acc;
  }
}

// ---------------------------------------------------------------------------------------------
// dense last level on the f64 matrix cores: Out[rowmap(i)] = sum_{k=kbeg(i)}^{kend-1} A(i,k) X[k]
//   A column-major (lda), rows >= mrows_valid are treated as zero rows (rank truncation);
//   upper != 0: A is upper triangular, k starts at the row tile's first row;
//   rowmap != NULL: output row permutation (jpvt scatter of QRCP.hpp:400-404).
// One wave owns a 16-row strip x all ceil(R/16) column tiles; v_mfma_f64_16x16x4_f64 lane maps:
//   A: lane l holds A[i = l&15][k = l>>4]; B: B[k = l>>4][j = l&15]; C/D: col = l&15, row = (l>>4) + 4*reg.
// ---------------------------------------------------------------------------------------------
// tri: 0 full, 1 upper (k >= row tile start), 2 lower (k < row tile end).  dscale/Out2 (optional):
// Out2[orow] = result / dscale[orow]  (the fused y /= d of the L solve, prec_solve.hpp:219).
// A is stored STRIP-MAJOR (host.hpp to_strip_layout): strip s = rows [16 s, 16 s + 16), element
// (row, k) at ((s * lda + k) * 16 + row % 16), lda = number of columns -- a strip streams through
// HBM sequentially, 128 B per k.
// Grid: (16-row strips) x (16-column tiles).  One 256-thread workgroup per 16x16 output tile: its 4
// waves split the K range (interleaved blocks of 32 k), each keeps two sets of 8 k-steps of operands
// (one in flight, one being multiplied; the loop is latency-bound at these sizes), and the partial
// tiles are summed through LDS in a fixed order.
template <int NW>
__global__ void __launch_bounds__(NW * 64) k_dense_gemm_d(int mrows_total, int mrows_valid, int kend, int tri,
                                                      const double *__restrict__ A, int lda,
                                                      const double *__restrict__ X, int logR,
                                                      const int32_t *__restrict__ rowmap,
                                                      double *__restrict__ Out,
                                                      const double *__restrict__ dscale,
                                                      double *__restrict__ Out2) {
  __shared__ double red[NW - 1][4][64];  // partial tiles of waves 1..NW-1: [wave-1][reg][lane]
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int i0 = blockIdx.x * 16;
  const int R = 1 << logR;
  const int colx = blockIdx.y * 16 + (lane & 15);
  const bool col_ok = colx < R;
  const int arow = i0 + (lane & 15);
  const int kq = lane >> 4;
  const bool arow_ok = arow < mrows_valid;
  v4f64 acc = v4f64{0.0, 0.0, 0.0, 0.0};
  const int kbeg = (tri == 1) ? i0 : 0;  // i0 is a multiple of 16, hence of 4
  if (tri == 2) kend = min(kend, i0 + 16);
  constexpr int KU = 8;  // k-steps (of 4) per operand set
  const int kstride = NW * (4 * KU);
  double a0[KU], b0[KU], a1[KU], b1[KU];
#define HIFAMD_LOAD_SET(aa, bb, kb_)                                                          \
  _Pragma("unroll") for (int u = 0; u < KU; ++u) {                                            \
    const int kk = (kb_) + 4 * u + kq;                                                        \
    const bool kok = kk < kend;                                                               \
    aa[u] = (arow_ok && kok) ? A[((int64_t)blockIdx.x * lda + kk) * 16 + (lane & 15)] : 0.0; \
    bb[u] = (col_ok && kok) ? X[((int64_t)kk << logR) + colx] : 0.0;                          \
  }
#define HIFAMD_MFMA_SET(aa, bb) \
  _Pragma("unroll") for (int u = 0; u < KU; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[u], bb[u], acc, 0, 0, 0);
  int kb = kbeg + wave * (4 * KU);
  if (kb < kend) { HIFAMD_LOAD_SET(a0, b0, kb) }
  while (kb < kend) {
    const int kb1 = kb + kstride;
    if (kb1 < kend) { HIFAMD_LOAD_SET(a1, b1, kb1) }
    HIFAMD_MFMA_SET(a0, b0)
    if (kb1 >= kend) break;
    const int kb2 = kb1 + kstride;
    if (kb2 < kend) { HIFAMD_LOAD_SET(a0, b0, kb2) }
    HIFAMD_MFMA_SET(a1, b1)
    kb = kb2;
  }
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave - 1][r][lane] = acc[r];
  }
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double val = acc[r];
#pragma unroll
    for (int w = 0; w < NW - 1; ++w) val += red[w][r][lane];
    const int row = i0 + kq + 4 * r;
    if (col_ok && row < mrows_total) {
      const int orow = rowmap ? rowmap[row] : row;
      Out[((int64_t)orow << logR) + colx] = val;
      if (Out2) Out2[((int64_t)orow << logR) + colx] = val / dscale[orow];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Full dense operator on a 64-column block (the combined top operator of a level, host.hpp build_top_operator):
// Out[rowmap[r]] = sum_k A(r,k) X[k],  A strip-major (lda = kend = columns rounded up to 32, zero padded), X = [kend][64]
// (rows beyond the operator's columns must be readable and finite).
// One workgroup per 16-row strip: wave = (column tile 0..3) x (K split 0..KS-1), so the strip's A panel is fetched
// from HBM ONCE (the four column-tile waves of a K split read the same fragments, they meet in the CU's L1) -- with a
// workgroup per (strip, tile), k_dense_gemm_d, every tile refetched the panel: 3.3x the operator's bytes in FETCH_SIZE.
// Operand sets of 8 k-steps double buffered, partial tiles of the K splits summed through LDS in a fixed order.
// ---------------------------------------------------------------------------------------------
template <int KS>
__global__ void __launch_bounds__(256 * KS) k_strip_gemm_d(int nrows, int kend, const double *__restrict__ A, int lda,
                                                           const double *__restrict__ X,
                                                           const int32_t *__restrict__ rowmap,
                                                           double *__restrict__ Out) {
  __shared__ double red[KS > 1 ? KS - 1 : 1][4][4][64];  // partial tiles of K splits 1..KS-1: [split-1][tile][reg][lane]
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ct = wave & 3, ks = wave >> 2;
  const int i0 = blockIdx.x * 16;
  const int colx = ct * 16 + (lane & 15);
  const int kq = lane >> 4;
  v4f64 acc0 = v4f64{0.0, 0.0, 0.0, 0.0}, acc1 = acc0;
  constexpr int KU = 8;
  const int kstride = KS * (4 * KU);
  double a0[KU], b0[KU], a1[KU], b1[KU];
  const double *Ap = A + ((int64_t)blockIdx.x * lda) * 16 + (lane & 15);
  // (unconditional loads -- kend is a multiple of 32, A zero-padded in k, X readable (finite) there: the compiler then
  //  counts its waits exactly and the next set stays in flight behind the MFMAs of the current one)
#define HIFAMD_SG_LOAD(aa, bb, kb_)                                  \
  _Pragma("unroll") for (int u = 0; u < KU; ++u) {                   \
    const int kk = (kb_) + 4 * u + kq;                               \
    aa[u] = Ap[(int64_t)kk * 16];                                    \
    bb[u] = X[((int64_t)kk << 6) + colx];                            \
  }
#define HIFAMD_SG_MFMA(aa, bb)                                                            \
  _Pragma("unroll") for (int u = 0; u < KU; u += 2) {                                     \
    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[u], bb[u], acc0, 0, 0, 0);             \
    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[u + 1], bb[u + 1], acc1, 0, 0, 0);     \
  }
  int kb = ks * (4 * KU);
  if (kb < kend) { HIFAMD_SG_LOAD(a0, b0, kb) }
  while (kb < kend) {
    const int kb1 = kb + kstride;
    if (kb1 < kend) { HIFAMD_SG_LOAD(a1, b1, kb1) }
    HIFAMD_SG_MFMA(a0, b0)
    if (kb1 >= kend) break;
    const int kb2 = kb1 + kstride;
    if (kb2 < kend) { HIFAMD_SG_LOAD(a0, b0, kb2) }
    HIFAMD_SG_MFMA(a1, b1)
    kb = kb2;
  }
#undef HIFAMD_SG_LOAD
#undef HIFAMD_SG_MFMA
  const v4f64 acc = acc0 + acc1;
  if (ks > 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) red[ks - 1][ct][r][lane] = acc[r];
  }
  __syncthreads();
  if (ks != 0) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double val = acc[r];
#pragma unroll
    for (int q = 0; q < KS - 1; ++q) val += red[q][ct][r][lane];
    const int row = i0 + kq + 4 * r;
    if (row < nrows) Out[((int64_t)(rowmap ? rowmap[row] : row) << 6) + colx] = val;
  }
}

// The same product with ONE A-fragment load per four MFMAs: a wave owns a K split (16 of them) and ALL four column
// tiles of the strip, so that per 4-k step it issues 1 load of A (HBM stream, every byte used once) and 4 loads of X
// (2 MB, L2-resident) for 4 MFMAs -- 1.25 wave-loads per MFMA instead of 2 (k_strip_gemm_d: the four column-tile waves
// of a K split load the same A fragment).  The product is bound by how many 512-byte wave-loads a compute unit gets
// issued (~180 per us), not by the matrix cores (tests/microbench/mfma_bench.hip).  Partial tiles are summed in two
// LDS rounds in a fixed order (deterministic).  kend: multiple of 8 * KU... of 32; A zero-padded in k; X finite there.
template <int KU>
__global__ void __launch_bounds__(1024) k_strip_gemm4_d(int nrows, int kend, const double *__restrict__ A, int lda,
                                                        const double *__restrict__ X, const int32_t *__restrict__ rowmap,
                                                        double *__restrict__ Out) {
  __shared__ double red[8][4][4][64];  // [wave][tile][reg][lane], 64 KB
  const int lane = threadIdx.x & 63;
  const int ks = threadIdx.x >> 6;  // 0..15
  const int cl = lane & 15, kq = lane >> 4;
  const int i0 = blockIdx.x * 16;
  v4f64 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = v4f64{0.0, 0.0, 0.0, 0.0};
  const int kstride = 16 * (4 * KU);
  double a0[KU], b0[KU][4], a1[KU], b1[KU][4];
  const double *Ap = A + ((int64_t)blockIdx.x * lda) * 16 + cl;
  const double *Xp = X + cl;
#define HIFAMD_SG_LOAD(aa, bb, kb_)                                                   \
  _Pragma("unroll") for (int u = 0; u < KU; ++u) {                                    \
    const int kk = (kb_) + 4 * u + kq;                                                \
    aa[u] = Ap[(int64_t)kk * 16];                                                     \
    _Pragma("unroll") for (int t = 0; t < 4; ++t) bb[u][t] = Xp[((int64_t)kk << 6) + 16 * t]; \
  }
#define HIFAMD_SG_MFMA(aa, bb)                                                                    \
  _Pragma("unroll") for (int u = 0; u < KU; ++u) {                                                \
    _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                 \
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[u], bb[u][t], acc[t], 0, 0, 0);          \
  }
  int kb = ks * (4 * KU);
  if (kb < kend) { HIFAMD_SG_LOAD(a0, b0, kb) }
  while (kb < kend) {
    const int kb1 = kb + kstride;
    if (kb1 < kend) { HIFAMD_SG_LOAD(a1, b1, kb1) }
    HIFAMD_SG_MFMA(a0, b0)
    if (kb1 >= kend) break;
    const int kb2 = kb1 + kstride;
    if (kb2 < kend) { HIFAMD_SG_LOAD(a0, b0, kb2) }
    HIFAMD_SG_MFMA(a1, b1)
    kb = kb2;
  }
#undef HIFAMD_SG_LOAD
#undef HIFAMD_SG_MFMA
  // round 1: waves 8..15 hand their tiles to waves 0..7; round 2: waves 1..7 to wave 0 (fixed order)
  if (ks >= 8) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[ks - 8][t][r][lane] = acc[t][r];
  }
  __syncthreads();
  if (ks < 8) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][r] += red[ks][t][r][lane];
  }
  __syncthreads();
  if (ks >= 1 && ks < 8) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[ks][t][r][lane] = acc[t][r];
  }
  __syncthreads();
  if (ks != 0) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = i0 + kq + 4 * r;
    if (row >= nrows) continue;
    const int64_t orow = (int64_t)(rowmap ? rowmap[row] : row) << 6;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      double val = acc[t][r];
#pragma unroll
      for (int q = 1; q < 8; ++q) val += red[q][t][r][lane];
      Out[orow + 16 * t + cl] = val;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Out[rowmap[r]] = sum_k G(r, k) X[k]: the combined top operator of a level and the tail operator of the hierarchy
// (round 3).  k_strip_gemm4_d gives a 16-row strip to a workgroup whose sixteen waves split K: every workgroup then pulls
// the WHOLE right-hand-side panel (nt x 512 B) through its compute unit's L1 beside its 16 x nt strip of G -- four times
// the bytes of the operator itself, served by the L2s: 48 us for 3,351 rows, 30 TFLOP/s (profiles/r02).  Here a
// workgroup owns 64 rows (four strips) x ONE K range of the grid's nks: its waves are (strip s, K quarter j); the
// panel's rows of the K range stream through LDS in chunks of 64 (double buffered, rows padded to 80 doubles: the two
// 16-lane halves of a ds_read_b64 then hit disjoint banks), so a panel row is fetched once per 64 output rows, and G
// streams from HBM once, each wave's fragments two chunks ahead in registers.  Partial tiles of the four K quarters are
// summed through LDS in a fixed order; nks > 1: the workgroup's 64 x 64 partial goes to part[ksplit][row][64] and
// k_top_reduce adds the splits in order (deterministic).  nct = 16-column tiles in use (a batch of <= 16 columns: one).
// Panel rows >= kvalid are read as zeros (the buffer behind them may hold anything, also non-finite values).
// G: strip-major MFMA operand (host.hpp mfma_operand), lda = K rounded up to 32.
// ---------------------------------------------------------------------------------------------
template <int NCT>
__global__ void __launch_bounds__(1024) k_top_gemm(int nrows, int kvalid, int kper /* K range per split, multiple of 64 */,
                                                   const double *__restrict__ A, int lda, const double *__restrict__ X,
                                                   const int32_t *__restrict__ rowmap, double *__restrict__ Out,
                                                   double *__restrict__ part, int nrows_pad, unsigned *tile_cnt) {
  // tile_cnt (round 4; NULL: the splits are added by k_top_reduce, a launch of its own): one counter per 64-row tile, zero
  // between launches.  The workgroup that finds its tile's other K splits already counted adds the gridDim.y partial tiles
  // in split order -- the order k_top_reduce uses: the same bits, replays stay bit-stable whichever split arrives last --
  // and writes the rows out; release / acquire fences at agent scope carry the partials across the XCDs' L2s.
  constexpr int nct = NCT;
  constexpr int XS = 80;               // LDS row stride of the panel (doubles)
  extern __shared__ double tg_lds[];   // kTopGemmLds (band_lds.hpp): two chunks of 64 panel rows; reused for the reduction
  double (*xb)[64 * XS] = reinterpret_cast<double (*)[64 * XS]>(tg_lds);
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;     // 0..15
  const int sw = wv & 3, jq = wv >> 2; // strip within the tile, K quarter within a chunk
  const int cl = lane & 15, kq = lane >> 4;
  const int tile = blockIdx.x, ksp = blockIdx.y;
  const int strip = tile * 4 + sw;
  const int nstrips = (nrows + 15) >> 4;
  const int k0 = ksp * kper, k1 = min(k0 + kper, lda);
  const int nchunks = (k1 - k0 + 63) >> 6;
  v4f64 acc[NCT];
#pragma unroll
  for (int t = 0; t < NCT; ++t) acc[t] = v4f64{0.0, 0.0, 0.0, 0.0};
  const bool live = strip < nstrips;
  // this wave's A fragments of chunk c: k = k0 + 64 c + 16 jq + 4 u + kq, u = 0..3 (512 contiguous bytes each).  Loads
  // are unconditional: a chunk index past the end re-reads the last chunk (never multiplied), a dead wave reads the
  // last strip, and k >= lda (the last chunk of the last split, at most 32 columns: the next strip's first ones, or the
  // padding behind the operand) meets panel rows >= kvalid, which are zero in LDS
  const double *Ap = A + ((int64_t)min(strip, nstrips - 1) * lda) * 16 + cl + (int64_t)(k0 + 16 * jq + kq) * 16;
  double a0[4], a1[4], a2[4];
#define HIFAMD_TG_A(aa, c_)                                                                   \
  {                                                                                           \
    const double *ap_ = Ap + (int64_t)min((c_), nchunks - 1) * (64 * 16);                     \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) aa[u] = ap_[u * 64];                        \
  }
  // panel chunk c into buffer b: 64 rows x 64 columns, 16 bytes per thread and pass (rows >= kvalid: zeros).  The loads
  // are unconditional too -- a load under a branch makes the compiler drain every outstanding load at the merge, the A
  // fragments with it: a row >= kvalid reads row kvalid - 1 and SELECTS zero (what lies behind kvalid is never touched),
  // a chunk index past the end re-reads the last chunk (stored to the idle buffer, never multiplied)
  typedef double v2f64 __attribute__((ext_vector_type(2)));
  const int xr = threadIdx.x >> 5, xc = (threadIdx.x & 31) * 2;  // row 0..31 (+32), columns xc, xc+1
  v2f64 xs0, xs1;
  bool xk0, xk1;  // (the row is a panel row: selected at the LDS store, behind the products, where the wait belongs)
#define HIFAMD_TG_XLOAD(c_)                                                                   \
  {                                                                                           \
    const int r0_ = k0 + 64 * min((c_), nchunks - 1) + xr, r1_ = r0_ + 32;                    \
    xk0 = r0_ < kvalid && xc < 16 * nct, xk1 = r1_ < kvalid && xc < 16 * nct;                 \
    xs0 = *reinterpret_cast<const v2f64 *>(X + ((int64_t)min(r0_, kvalid - 1) << 6) + xc);    \
    xs1 = *reinterpret_cast<const v2f64 *>(X + ((int64_t)min(r1_, kvalid - 1) << 6) + xc);    \
  }
#define HIFAMD_TG_XSTORE(b_)                                                                  \
  {                                                                                           \
    *reinterpret_cast<v2f64 *>(&xb[b_][xr * XS + xc]) = xk0 ? xs0 : v2f64{0.0, 0.0};          \
    *reinterpret_cast<v2f64 *>(&xb[b_][(xr + 32) * XS + xc]) = xk1 ? xs1 : v2f64{0.0, 0.0};   \
  }
#define HIFAMD_TG_MFMA(aa, b_)                                                                     \
  _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                  \
    const double *bp_ = &xb[b_][(16 * jq + 4 * u + kq) * XS + cl];                                 \
    _Pragma("unroll") for (int t = 0; t < NCT; ++t)                                                \
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[u], bp_[16 * t], acc[t], 0, 0, 0);        \
  }
  // one chunk: the panel of chunk c + 1 is requested FIRST, the A fragments of chunk c + 2 behind it -- vector loads
  // return in order, so the wait in front of the panel's LDS store leaves those four A loads in flight (a counted wait,
  // never vmcnt(0)); the A fragments of chunk c landed with the panel of chunk c, one step ago
#define HIFAMD_TG_STEP(c_, acur, anew)                                         \
  {                                                                            \
    HIFAMD_TG_XLOAD((c_) + 1)                                                  \
    __builtin_amdgcn_sched_barrier(0);                                         \
    HIFAMD_TG_A(anew, (c_) + 2)                                                \
    __builtin_amdgcn_sched_barrier(0); /* (the requests stay in this order, in front of the products) */ \
    HIFAMD_TG_MFMA(acur, ((c_) & 1))                                           \
    __builtin_amdgcn_sched_barrier(0);                                         \
    HIFAMD_TG_XSTORE((((c_) + 1) & 1))                                         \
    __syncthreads();                                                           \
  }
  HIFAMD_TG_XLOAD(0)
  HIFAMD_TG_A(a0, 0)
  HIFAMD_TG_A(a1, 1)
  HIFAMD_TG_XSTORE(0)
  __syncthreads();
  // (A fragments two chunks ahead in registers, the panel one chunk ahead in LDS; three chunks per trip: the fragment
  // sets rotate by name)
  int c = 0;
  for (; c + 3 <= nchunks; c += 3) {  // (one exit, at the top: the accumulators keep their registers round the loop)
    HIFAMD_TG_STEP(c, a0, a2)
    HIFAMD_TG_STEP(c + 1, a1, a0)
    HIFAMD_TG_STEP(c + 2, a2, a1)
  }
  if (c < nchunks) {  // the last one or two chunks
    HIFAMD_TG_STEP(c, a0, a2)
    if (c + 1 < nchunks) HIFAMD_TG_STEP(c + 1, a1, a0)
  }
#undef HIFAMD_TG_STEP
#undef HIFAMD_TG_A
#undef HIFAMD_TG_XLOAD
#undef HIFAMD_TG_XSTORE
#undef HIFAMD_TG_MFMA
  // (the panel buffers become the reduction scratch: every wave is past the loop's last barrier)
  // K quarters 1..3 hand their tiles to quarter 0 of the same strip, summed in the order 0, 1, 2, 3
  double *red = &xb[0][0];  // [jq - 1][sw][t][r][lane]: 3 x 4 x 4 x 4 x 64 doubles = 96 KB > 80 KB: two rounds
  // round 1: quarters 2, 3 -> scratch; quarters 0, 1 add (0 += 2 is NOT the order wanted) -- keep it simple and exact:
  // quarter 1 first, then 2, then 3, one quarter per round (3 rounds x 32 KB)
  for (int q = 1; q < 4; ++q) {
    if (jq == q) {
#pragma unroll
      for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(((sw * 4 + t) * 4 + r) << 6) + lane] = acc[t][r];
    }
    __syncthreads();
    if (jq == 0) {
#pragma unroll
      for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] += red[(((sw * 4 + t) * 4 + r) << 6) + lane];
    }
    __syncthreads();
  }
  if (jq == 0 && live) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * strip + kq + 4 * r;
      if (row >= nrows) continue;
      double *dst = (gridDim.y > 1) ? part + (((int64_t)ksp * nrows_pad + row) << 6) : Out + ((int64_t)(rowmap ? rowmap[row] : row) << 6);
#pragma unroll
      for (int t = 0; t < NCT; ++t) dst[16 * t + cl] = acc[t][r];
    }
  }
  if (gridDim.y == 1 || tile_cnt == nullptr) return;
  // ---- the last split of this tile to arrive adds the partial tiles (fixed order) and writes the rows out
  __shared__ int tg_last;
  __threadfence();  // (release: this workgroup's partial tile)
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned seen = atomicAdd(&tile_cnt[tile], 1u);
    tg_last = (seen == gridDim.y - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!tg_last) return;
  __threadfence();  // (acquire: the other splits' partial tiles)
  {
    const int row = 64 * tile + (int)(threadIdx.x >> 4), c4 = (int)(threadIdx.x & 15) * 4;  // 64 rows x 16 groups of 4 columns
    if (row < nrows && c4 < 16 * nct) {
      typedef double v4d __attribute__((ext_vector_type(4)));
      const double *pp = part + ((int64_t)row << 6) + c4;
      v4d sacc = *reinterpret_cast<const v4d *>(pp);
      for (int q = 1; q < (int)gridDim.y; ++q) sacc += *reinterpret_cast<const v4d *>(pp + (((int64_t)q * nrows_pad) << 6));
      *reinterpret_cast<v4d *>(Out + ((int64_t)(rowmap ? rowmap[row] : row) << 6) + c4) = sacc;
    }
  }
  if (threadIdx.x == 0) tile_cnt[tile] = 0u;  // (ready for the next launch: kernel boundaries order it)
}

// the K splits of k_top_gemm, added in order
__global__ void __launch_bounds__(256) k_top_reduce(int nrows, int nks, const double *__restrict__ part, int nrows_pad,
                                                    const int32_t *__restrict__ rowmap, double *__restrict__ Out, int nct) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows || lane >= 16 * nct) return;
  double sacc = part[((int64_t)row << 6) + lane];
  for (int q = 1; q < nks; ++q) sacc += part[(((int64_t)q * nrows_pad + row) << 6) + lane];
  Out[((int64_t)(rowmap ? rowmap[row] : row) << 6) + lane] = sacc;
}

// ---------------------------------------------------------------------------------------------
// The same product for complex handles: Out[rowmap[r]] = sum_k G(r, k) X[k], G complex as the two real strip-major
// planes [re | im] of host.hpp mfma_operand (each ceil(nrows / 16) * 16 * lda doubles), X and Out complex
// row-interleaved [rows][64], i.e. a real view [rows][128] with (re, im) in neighbouring columns.  gfx950 has no complex
// matrix instruction: P = G_re X and Q = G_im X are formed on the real view with the SAME B fragments, and complex
// column j is out_re(j) = P[2j] - Q[2j+1], out_im(j) = P[2j+1] + Q[2j].  In the C/D layout col = lane & 15, so a value's
// partner sits in the neighbouring lane: ONE cross-lane exchange per accumulator register at the very end combines
// them.  (The alternative -- de-interleaving X while it is staged and negating the G_im fragments -- needs two panels
// in LDS and four products per fragment pair with separate B fragments; the exchange costs 8 shuffles per lane and
// keeps the staging a plain copy, so it is what is done here.)
// Shape as k_top_gemm: 64-row tiles x K splits (nks, kper from the operator's size alone, never from the batch width:
// a column's sum order does not depend on the batch), panel chunks of 64 k-rows through LDS at the 80-double row
// stride, every global access unconditional (clamped indices; rows >= kvalid are selected to zero behind the
// products).  The column dimension is the grid's third axis: a workgroup takes a group of 32 real columns (two
// 16-column tiles = 16 complex columns), so its accumulators -- two planes x two tiles -- number what the real kernel's
// four tiles do.  NCT = tiles in use in the LAST group (a batch of <= 8 columns: one group, one tile); every group in
// front of it is full.  The K splits are never summed here (no atomics, no fences, no last arriver): nks > 1 writes
// the combined partial tiles to part[split][row][128] and k_top_reduce_z adds them in split order.
// ---------------------------------------------------------------------------------------------
template <int NT>
__device__ __forceinline__ void top_gemm_z_body(int nrows, int kvalid, int kper, const double *__restrict__ A, int lda,
                                                const double *__restrict__ X, const int32_t *__restrict__ rowmap,
                                                double *__restrict__ Out, double *__restrict__ part, int nrows_pad,
                                                double *tg_lds) {
  constexpr int XS = 80;  // LDS row stride of the panel (doubles)
  double (*xb)[64 * XS] = reinterpret_cast<double (*)[64 * XS]>(tg_lds);
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int sw = wv & 3, jq = wv >> 2;  // strip within the tile, K quarter within a chunk
  const int cl = lane & 15, kq = lane >> 4;
  const int tile = blockIdx.x, ksp = blockIdx.y;
  const int col0 = 32 * (int)blockIdx.z;  // first real column of this group
  const int strip = tile * 4 + sw;
  const int nstrips = (nrows + 15) >> 4;
  const int64_t plane = (int64_t)nstrips * 16 * lda;  // G_im behind G_re
  const int k0 = ksp * kper, k1 = min(k0 + kper, lda);
  const int nchunks = (k1 - k0 + 63) >> 6;
  v4f64 accP[NT], accQ[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) accP[t] = accQ[t] = v4f64{0.0, 0.0, 0.0, 0.0};
  const bool live = strip < nstrips;
  // A fragments of chunk c, both planes: k = k0 + 64 c + 16 jq + 4 u + kq.  Unconditional as in k_top_gemm: a chunk index
  // past the end re-reads the last chunk, a dead wave the last strip; k >= lda (at most 32 columns: the next strip, the
  // other plane or the padding behind the operand) meets panel rows >= kvalid, which are zero in LDS
  const double *Ap = A + ((int64_t)min(strip, nstrips - 1) * lda) * 16 + cl + (int64_t)(k0 + 16 * jq + kq) * 16;
  double ar0[4], ai0[4], ar1[4], ai1[4];
#define HIFAMD_TGZ_A(ar, ai, c_)                                                              \
  {                                                                                           \
    const double *ap_ = Ap + (int64_t)min((c_), nchunks - 1) * (64 * 16);                     \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) ar[u] = ap_[u * 64];                        \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) ai[u] = ap_[plane + u * 64];                \
  }
  // panel chunk c: 64 rows x 32 real columns, 16 bytes per thread (a row >= kvalid reads row kvalid - 1 and selects zero)
  typedef double v2f64 __attribute__((ext_vector_type(2)));
  const int xr = threadIdx.x >> 4, xc = (threadIdx.x & 15) * 2;  // row 0..63, columns xc, xc + 1 of the group
  v2f64 xs0;
  bool xk0;
#define HIFAMD_TGZ_XLOAD(c_)                                                                          \
  {                                                                                                   \
    const int r0_ = k0 + 64 * min((c_), nchunks - 1) + xr;                                            \
    xk0 = r0_ < kvalid && xc < 16 * NT;                                                               \
    xs0 = *reinterpret_cast<const v2f64 *>(X + ((int64_t)min(r0_, kvalid - 1) << 7) + col0 + xc);     \
  }
#define HIFAMD_TGZ_XSTORE(b_) *reinterpret_cast<v2f64 *>(&xb[b_][xr * XS + xc]) = xk0 ? xs0 : v2f64{0.0, 0.0};
#define HIFAMD_TGZ_MFMA(ar, ai, b_)                                                                \
  _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                  \
    const double *bp_ = &xb[b_][(16 * jq + 4 * u + kq) * XS + cl];                                 \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) {                                               \
      const double bv_ = bp_[16 * t];                                                              \
      accP[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[u], bv_, accP[t], 0, 0, 0);                \
      accQ[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[u], bv_, accQ[t], 0, 0, 0);                \
    }                                                                                              \
  }
  // one chunk: the panel of chunk c + 1 is requested first, the A fragments of chunk c + 1 behind it (vector loads return
  // in order: the wait in front of the panel's LDS store leaves the eight A loads in flight); a double buffer of fragment
  // sets -- the set being multiplied and the one in flight
#define HIFAMD_TGZ_STEP(c_, rcur, icur, rnew, inew)                            \
  {                                                                            \
    HIFAMD_TGZ_XLOAD((c_) + 1)                                                 \
    __builtin_amdgcn_sched_barrier(0);                                         \
    HIFAMD_TGZ_A(rnew, inew, (c_) + 1)                                         \
    __builtin_amdgcn_sched_barrier(0);                                         \
    HIFAMD_TGZ_MFMA(rcur, icur, ((c_) & 1))                                    \
    __builtin_amdgcn_sched_barrier(0);                                         \
    HIFAMD_TGZ_XSTORE((((c_) + 1) & 1))                                        \
    __syncthreads();                                                           \
  }
  HIFAMD_TGZ_XLOAD(0)
  HIFAMD_TGZ_A(ar0, ai0, 0)
  HIFAMD_TGZ_XSTORE(0)
  __syncthreads();
  int c = 0;
  for (; c + 2 <= nchunks; c += 2) {
    HIFAMD_TGZ_STEP(c, ar0, ai0, ar1, ai1)
    HIFAMD_TGZ_STEP(c + 1, ar1, ai1, ar0, ai0)
  }
  if (c < nchunks) HIFAMD_TGZ_STEP(c, ar0, ai0, ar1, ai1)
#undef HIFAMD_TGZ_STEP
#undef HIFAMD_TGZ_A
#undef HIFAMD_TGZ_XLOAD
#undef HIFAMD_TGZ_XSTORE
#undef HIFAMD_TGZ_MFMA
  // K quarters 1..3 hand their tiles to quarter 0 of the same strip, one quarter per round: the order 0, 1, 2, 3
  // (the panel buffers are the scratch: [sw][plane][t][r][lane], 4 x 2 x 2 x 4 x 64 doubles = 32 KB)
  double *red = &xb[0][0];
  for (int q = 1; q < 4; ++q) {
    if (jq == q) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          red[((((sw * 2 + 0) * 2 + t) * 4 + r) << 6) + lane] = accP[t][r];
          red[((((sw * 2 + 1) * 2 + t) * 4 + r) << 6) + lane] = accQ[t][r];
        }
    }
    __syncthreads();
    if (jq == 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          accP[t][r] += red[((((sw * 2 + 0) * 2 + t) * 4 + r) << 6) + lane];
          accQ[t][r] += red[((((sw * 2 + 1) * 2 + t) * 4 + r) << 6) + lane];
        }
    }
    __syncthreads();
  }
  if (jq != 0 || !live) return;  // (whole waves)
  const bool odd = (cl & 1) != 0;  // an even lane holds the real part's column 2j, its neighbour the imaginary part's 2j + 1
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double z[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const double qn = __shfl_xor(accQ[t][r], 1);  // (every lane of the wave takes part: in front of the row test)
      z[t] = odd ? accP[t][r] + qn : accP[t][r] - qn;
    }
    const int row = 16 * strip + kq + 4 * r;
    if (row >= nrows) continue;
    double *dst = ((gridDim.y > 1) ? part + (((int64_t)ksp * nrows_pad + row) << 7) : Out + ((int64_t)(rowmap ? rowmap[row] : row) << 7)) + col0;
#pragma unroll
    for (int t = 0; t < NT; ++t) dst[16 * t + cl] = z[t];
  }
}

// NCT = 1 carries BOTH bodies: the two-tile one for the full groups in front (blockIdx.z + 1 < gridDim.z) and the one-tile
// one for the last group, chosen by a branch that is uniform over the workgroup.  That is why k_top_gemm_z<1> is the
// larger code object of the two (98 VGPRs against 96 of <2>, whose single body the compiler sees alone); a batch of
// <= 8 columns has one group and runs the one-tile body only.
template <int NCT>
__global__ void __launch_bounds__(1024) k_top_gemm_z(int nrows, int kvalid, int kper /* K range per split, multiple of 64 */,
                                                     const double *__restrict__ A, int lda, const double *__restrict__ X,
                                                     const int32_t *__restrict__ rowmap, double *__restrict__ Out,
                                                     double *__restrict__ part, int nrows_pad) {
  extern __shared__ double tgz_lds[];  // two chunks of 64 panel rows at stride 80; reused for the reduction
  if (NCT == 2 || blockIdx.z + 1 < gridDim.z)  // (uniform over the workgroup)
    top_gemm_z_body<2>(nrows, kvalid, kper, A, lda, X, rowmap, Out, part, nrows_pad, tgz_lds);
  else
    top_gemm_z_body<1>(nrows, kvalid, kper, A, lda, X, rowmap, Out, part, nrows_pad, tgz_lds);
}

// the K splits of k_top_gemm_z, added in split order: a row of the real view has 128 columns, ncols of them in use
__global__ void __launch_bounds__(256) k_top_reduce_z(int nrows, int nks, const double *__restrict__ part, int nrows_pad,
                                                      const int32_t *__restrict__ rowmap, double *__restrict__ Out, int ncols) {
  const int col = threadIdx.x & 127;
  const int row = blockIdx.x * 2 + (threadIdx.x >> 7);
  if (row >= nrows || col >= ncols) return;
  double sacc = part[((int64_t)row << 7) + col];
  for (int q = 1; q < nks; ++q) sacc += part[(((int64_t)q * nrows_pad + row) << 7) + col];
  Out[((int64_t)(rowmap ? rowmap[row] : row) << 7) + col] = sacc;
}

// ---------------------------------------------------------------------------------------------
// Block-dense thin bands, step (2): Out[rowmap[r]] = sum_{k<=r} Tinv(r,k) X[k] for one diagonal block
// (nb rows), Tinv = explicit inverse of the block's unit lower triangle, strip-major with
// lda = nb rounded up to 32 (zero padded; everything right of the diagonal is zero too).
// The product is MFMA-bound on gfx950 (v_mfma_f64_16x16x4_f64 occupies a SIMD for 64 cycles) and the
// triangle makes strip s cost s+1 units, so workgroup p owns the PAIR of strips (p, S-1-p): every
// workgroup then carries the same S+1 units and the grid is (pairs) x (16-column tiles) -- 256
// workgroups for a 2048-row block at 64 columns, one per compute unit.  The NW waves deal the
// pair's 32-k operand sets round-robin (split-K); a set is 8 A- and 8 B-fragments kept in registers,
// one set in flight while the previous one is multiplied, two accumulators per strip so that
// consecutive MFMAs do not wait for each other.  Partial tiles are summed through LDS in a fixed
// order (deterministic).  X must have nb rounded up to 32 readable rows (padding rows are masked).
// ---------------------------------------------------------------------------------------------
template <int NW>
__global__ void __launch_bounds__(NW * 64) k_tri_gemm_d(int nb, const double *__restrict__ A, int lda,
                                                        const double *__restrict__ X, int logR,
                                                        const int32_t *__restrict__ rowmap,
                                                        double *__restrict__ Out,
                                                        const double *__restrict__ dscale,
                                                        double *__restrict__ Out2) {
  __shared__ double red[NW - 1][2][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int S = (nb + 15) >> 4;
  const int sA = blockIdx.x, sB = S - 1 - (int)blockIdx.x;
  const bool two = sB > sA;
  const int R = 1 << logR;
  const int colx = blockIdx.y * 16 + (lane & 15);
  const bool col_ok = colx < R;
  const int colc = col_ok ? colx : 0;
  const int kq = lane >> 4;
  const int nsA = (min(nb, 16 * (sA + 1)) + 31) >> 5;
  const int nsB = two ? (min(nb, 16 * (sB + 1)) + 31) >> 5 : 0;
  const int nsets = nsA + nsB;
  const double *Xl = X + colc;
  const double *A_a = A + ((int64_t)sA * lda) * 16 + (lane & 15);
  const double *A_b = A + ((int64_t)(two ? sB : sA) * lda) * 16 + (lane & 15);
  v4f64 accA0 = v4f64{0.0, 0.0, 0.0, 0.0}, accA1 = accA0, accB0 = accA0, accB1 = accA0;
  constexpr int KU = 8;
  double a0[KU], b0[KU], a1[KU], b1[KU];
#define HIFAMD_TG_LOAD(aa, bb, t_)                                                   \
  {                                                                                  \
    const bool isB_ = (t_) >= nsA;                                                   \
    const int kb_ = 32 * (isB_ ? (t_) - nsA : (t_)) + kq;                            \
    const double *ap_ = (isB_ ? A_b : A_a) + (int64_t)kb_ * 16;                      \
    const double *xp_ = Xl + ((int64_t)kb_ << logR);                                 \
    _Pragma("unroll") for (int u = 0; u < KU; ++u) {                                 \
      aa[u] = ap_[u * 64];                                                           \
      const double xv_ = xp_[(int64_t)(4 * u) << logR];                              \
      bb[u] = (kb_ + 4 * u < nb) ? xv_ : 0.0;                                        \
    }                                                                                \
  }
#define HIFAMD_TG_MFMA(aa, bb, t_)                                                                 \
  if ((t_) >= nsA) {                                                                               \
    _Pragma("unroll") for (int u = 0; u < KU; u += 2) {                                            \
      accB0 = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[u], bb[u], accB0, 0, 0, 0);                  \
      accB1 = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[u + 1], bb[u + 1], accB1, 0, 0, 0);          \
    }                                                                                              \
  } else {                                                                                         \
    _Pragma("unroll") for (int u = 0; u < KU; u += 2) {                                            \
      accA0 = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[u], bb[u], accA0, 0, 0, 0);                  \
      accA1 = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[u + 1], bb[u + 1], accA1, 0, 0, 0);          \
    }                                                                                              \
  }
  int t = wave;
  if (t < nsets) HIFAMD_TG_LOAD(a0, b0, t)
  while (t < nsets) {
    const int t1 = t + NW;
    if (t1 < nsets) HIFAMD_TG_LOAD(a1, b1, t1)
    HIFAMD_TG_MFMA(a0, b0, t)
    if (t1 >= nsets) break;
    const int t2 = t1 + NW;
    if (t2 < nsets) HIFAMD_TG_LOAD(a0, b0, t2)
    HIFAMD_TG_MFMA(a1, b1, t1)
    t = t2;
  }
#undef HIFAMD_TG_LOAD
#undef HIFAMD_TG_MFMA
  const v4f64 accA = accA0 + accA1, accB = accB0 + accB1;
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      red[wave - 1][0][r][lane] = accA[r];
      red[wave - 1][1][r][lane] = accB[r];
    }
  }
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (h == 1 && !two) break;
    const int i0 = 16 * (h ? sB : sA);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double val = h ? accB[r] : accA[r];
#pragma unroll
      for (int w = 0; w < NW - 1; ++w) val += red[w][h][r][lane];
      const int row = i0 + kq + 4 * r;
      if (col_ok && row < nb) {
        const int orow = rowmap ? rowmap[row] : row;
        Out[((int64_t)orow << logR) + colx] = val;
        if (Out2) Out2[((int64_t)orow << logR) + colx] = val / dscale[orow];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Component-dense band (host.hpp plan_bands_cd), R = 64, real data.  Workgroup wg0 + blockIdx.x owns the components
// (groups) [wg_grp_ptr[g], wg_grp_ptr[g+1]); a component is a set of <= cd_rows rows that depend only on each other and
// on rows finished by EARLIER launches.  Per component (descriptor: host.hpp build_cd_streams):
//   phase 1  t[r] = rhs[r] - (the row's nonzeros whose sources lie outside the component and were not carried by the
//            previous launch).  Those nonzeros of ALL rows form one packed stream (column, value, local row); every wave
//            owns a contiguous chunk of rows and of the stream: it puts its rows' right-hand sides into LDS (all loads in
//            flight at once), then walks its entries as items of 64 with eight gathers per batch -- across row
//            boundaries, the running row's sum in a register, LDS touched once per row change.  No flags, no polling;
//   phase 2  x = Tinv_c * t on the f64 matrix cores: Tinv_c is the explicit inverse of the component's own unit
//            triangle (strip-major, built on the host), the B operand comes from LDS.  A unit is one 16-row strip x two
//            16-column tiles (an A fragment feeds two MFMAs); units go to the waves heaviest first in snake order over
//            the four SIMDs; operand sets of 8 k-steps are double buffered.
// No dependent step survives inside a launch, whatever the depth of the component.  Workgroups beyond n_band run the
// carried prefix of the NEXT band, exactly as in k_trsv_band_p.  The summation order differs from the reference's
// (tolerance-level, like every block-dense band); exact mode never plans such bands.
// ---------------------------------------------------------------------------------------------
// Development probe (make CSPROBE=1): every workgroup of k_band_cs / k_band_cd records wall-clock stamps (100 MHz) of its
// phases into a global buffer (engine.hip dumps it to HIFIR_AMD_CSPROBE_OUT); compiled out by default.
#ifdef HIFAMD_CSPROBE
__device__ unsigned long long *g_csprobe = nullptr;
__device__ unsigned g_csprobe_cap = 0, g_csprobe_cnt = 0;
#define HIFAMD_CSP_DECL unsigned long long csp_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define HIFAMD_CSP(k) \
  if (threadIdx.x == 0) csp_[k] = wall_clock64();
#define HIFAMD_CSP_FLUSH(kind, a, b)                                                   \
  if (threadIdx.x == 0 && g_csprobe) {                                                 \
    const unsigned slot_ = atomicAdd(&g_csprobe_cnt, 1u);                              \
    if (slot_ < g_csprobe_cap) {                                                       \
      unsigned long long *r_ = g_csprobe + (size_t)slot_ * 12;                         \
      for (int k_ = 0; k_ < 8; ++k_) r_[k_] = csp_[k_];                                \
      r_[8] = ((unsigned long long)(kind) << 32) | blockIdx.x;                         \
      r_[9] = ((unsigned long long)gridDim.x << 32) | (unsigned)(a);                   \
      r_[10] = (unsigned long long)(b);                                                \
      r_[11] = __builtin_amdgcn_s_getreg((4 << 11) | (0 << 6) | 20) /* HW_REG_XCC_ID */; \
    }                                                                                  \
  }
#else
#define HIFAMD_CSP_DECL
#define HIFAMD_CSP(k)
#define HIFAMD_CSP_FLUSH(kind, a, b)
#endif

// ---- what the heads of the component-band kernels share ---------------------------------------------------------------
// The array at byte offset `off` of the kernel's LDS layout (band_lds.hpp), reached from the array in front of it (`prev`,
// at `prev_off`).  The step is taken in ELEMENTS of `prev`: the compiler then folds each scaled size into the uses, as it
// does for pointer arithmetic, instead of keeping every byte offset in a scalar register from the kernel's head on
// (k_band_ls and k_band_us have none to spare).  tests/cpp/band_lds_test.cpp checks that every step is a whole number
// of elements.
template <class E, class P>
__device__ __forceinline__ E *lds_next(P *prev, int32_t prev_off, int32_t off) {
  return reinterpret_cast<E *>(prev + (off - prev_off) / (int32_t)sizeof(P));
}
// the carried prefix of the NEXT band over the sources older than this band: the launch's extra workgroups, wave pw of nwaves
template <bool LOWER>
__device__ __forceinline__ void band_carried_prefix(int32_t pw, int32_t nwaves, int32_t ps0, int32_t ps1, const int32_t *__restrict__ ptr,
                                                    const int32_t *__restrict__ split, const int32_t *__restrict__ col,
                                                    const double *__restrict__ val, const int32_t *__restrict__ rowid,
                                                    const double *__restrict__ d, double *w, double *v, int lane,
                                                    const FirstL<double> &fl) {
  const double *pf_bin = (LOWER && fl.on()) ? fl.bin.get() : nullptr;
  trsv_stream_r64<double, 0, LOWER, true>(ps0 + pw, ps1, nwaves, ptr, split, col, val, nullptr, rowid, d, LOWER ? w : v, w, lane,
                                          nullptr, 0, nullptr, true, nullptr, 0, 0, pf_bin, &fl);
}
// the components [c_first, c_last) of band workgroup bw.  single_c0 >= 0: every workgroup of this band owns exactly ONE
// component, number single_c0 + bw (saves the dependent load of the workgroup's group range)
__device__ __forceinline__ void band_components(int32_t single_c0, const int32_t *__restrict__ wg_grp_ptr, int32_t wg0, int32_t bw,
                                                int32_t &c_first, int32_t &c_last) {
  if (single_c0 >= 0) {
    c_first = single_c0 + bw;
    c_last = c_first + 1;
  } else {
    c_first = wg_grp_ptr[wg0 + bw];
    c_last = wg_grp_ptr[wg0 + bw + 1];
  }
}
// where a band's rows start from.  div_u: the kernel that touches a U row first starts it from w[i] / d[i]; first_l (S1
// fused, FirstL): a band that touches its L rows first takes rhs[i] = s[p[i]] * b[p[i]] from the level's input
template <class D>
struct BandRhs {
  bool div_u, first_l;
  const D *rhs;
  int64_t rstride;
  __device__ __forceinline__ int col(int c, const FirstL<D> &fl) const { return first_l ? min(c, fl.nrhs - 1) : c; }
};
template <bool LOWER, class D>
__device__ __forceinline__ BandRhs<D> band_rhs(int first_u, const FirstL<D> &fl, D *w, D *x) {
  BandRhs<D> r;
  r.div_u = !LOWER && first_u;
  r.first_l = LOWER && first_u && fl.on();
  r.rhs = r.div_u ? (const D *)w : (r.first_l ? fl.bin.get() : (const D *)x);
  r.rstride = r.first_l ? fl.ldb : 64;
  return r;
}

template <bool LOWER, bool SPARSE>
__global__ void __launch_bounds__(1024) k_band_cd(int32_t wg0, const int32_t *__restrict__ wg_grp_ptr,
                                                  const int32_t *__restrict__ cd_desc, const int32_t *__restrict__ ptr,
                                                  const int32_t *__restrict__ split, const int32_t *__restrict__ col,
                                                  const double *__restrict__ val, const int32_t *__restrict__ rowid,
                                                  const double *__restrict__ d, double *w, double *v,
                                                  const double *__restrict__ tinv, const int32_t *__restrict__ mid_col,
                                                  const double *__restrict__ mid_val, const uint8_t *__restrict__ mid_lrow,
                                                  int first_u, int32_t n_band, int32_t ps0, int32_t ps1, int32_t single_c0,
                                                  int32_t lds_rows, int32_t own_cap, int dbg, FirstL<double> fl,
                                                  const double *__restrict__ own_val, const uint8_t *__restrict__ own_lsrc,
                                                  const uint16_t *__restrict__ own_rptr, const uint8_t *__restrict__ own_lvl,
                                                  LastU<double> lu, RowSkip rs) {
  extern __shared__ double cd_tbuf[];  // [lds_rows][64] right-hand sides, then lds_rows row ids
  HIFAMD_CSP_DECL
  HIFAMD_CSP(0)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = blockDim.x >> 6;
  if ((int32_t)blockIdx.x >= n_band) {  // carried prefix of the next band over the sources older than this band
    const int32_t pw = __builtin_amdgcn_readfirstlane(((int32_t)blockIdx.x - n_band) * nw + wave);
    if (dbg & 4) return;
    band_carried_prefix<LOWER>(pw, ((int32_t)gridDim.x - n_band) * nw, ps0, ps1, ptr, split, col, val, rowid, d, w, v, lane, fl);
    HIFAMD_CSP(6)
    HIFAMD_CSP_FLUSH(2 + (LOWER ? 0 : 4) + 16, n_band, 0)
    return;
  }
  double *x = LOWER ? w : v;
  const BandRhs<double> br = band_rhs<LOWER>(first_u, fl, w, x);
  const bool div_u = br.div_u, first_l = br.first_l;
  const double *rhs = br.rhs;
  const int64_t rstride = br.rstride;
  const int rlane = br.col(lane, fl);
  int32_t c_first, c_last;
  band_components(single_c0, wg_grp_ptr, wg0, (int32_t)blockIdx.x, c_first, c_last);
  const int kq = lane >> 4;
  const BandCdLds lay(lds_rows, SPARSE, own_cap);  // (own_cap: multiple of 64, host: the plan's maximum)
  int32_t *cd_rowid = lds_next<int32_t>(cd_tbuf, lay.tb, lay.rowid);  // the component's row ids, for phase 2
  // SPARSE: the component's own nonzeros (value, local source row), their row offsets and the depth levels
  double *ow_val = lds_next<double>(cd_rowid, lay.rowid, lay.ow_val);
  uint8_t *ow_src = lds_next<uint8_t>(ow_val, lay.ow_val, lay.ow_src);
  uint16_t *ow_rptr = lds_next<uint16_t>(ow_src, lay.ow_src, lay.ow_rptr);
  uint8_t *ow_lvl = lds_next<uint8_t>(ow_rptr, lay.ow_rptr, lay.ow_lvl);
  // fused S7 (LastU): output row and scale of every row of the component, behind everything else
  const bool last_u = !LOWER && lu.on();
  double *cd_ot = SPARSE ? lds_next<double>(ow_lvl, lay.ow_lvl, lay.ot) : lds_next<double>(ow_val, lay.ow_val, lay.ot);
  int32_t *cd_oi = lds_next<int32_t>(cd_ot, lay.ot, lay.oi);
  double *yout = last_u ? lu.out.get() : nullptr;
  for (int32_t c = c_first; c < c_last; ++c) {
    const int32_t *dsc = cd_desc + (int64_t)c * 28;
    const int32_t s0 = dsc[0], nb = dsc[1], mid0 = dsc[2];
    const int64_t inv_off = ((int64_t)(uint32_t)dsc[5] << 32) | (uint32_t)dsc[4];
    const uint8_t *wrow = reinterpret_cast<const uint8_t *>(dsc + 6);
    const uint16_t *wmid = reinterpret_cast<const uint16_t *>(dsc + 11);
    const int r0 = wrow[wave], nr = (int)wrow[wave + 1] - r0;
    const int32_t e0 = mid0 + (int32_t)wmid[wave], e1 = mid0 + (int32_t)wmid[wave + 1];
    // phase 2's first operand set is requested NOW: it does not depend on phase 1 and its latency hides behind it
    const int lda = (nb + 31) & ~31;
    const double *Ac = tinv + inv_off;
    const int S = (nb + 15) >> 4, nunits = S * 2;
    const int wrow4 = wave >> 2, wcol4 = wave & 3;
    const int q_first = wrow4 * 4 + ((wrow4 & 1) ? 3 - wcol4 : wcol4);  // snake order over the SIMDs (wave % 4)
    constexpr int KU = 8;
    double a0[KU], a1[KU];
    if (SPARSE) {  // own nonzeros, row offsets and levels into LDS (coalesced, in flight during phase 1)
      const int32_t own0 = dsc[20], nown = dsc[21], orp0 = dsc[22], lvl0 = dsc[23], nlvl = dsc[24];
      for (int32_t t = (int32_t)threadIdx.x; t < nown; t += (int32_t)blockDim.x) {
        ow_val[t] = own_val[own0 + t];
        ow_src[t] = own_lsrc[own0 + t];
      }
      for (int32_t t = (int32_t)threadIdx.x; t <= nb; t += (int32_t)blockDim.x) ow_rptr[t] = own_rptr[orp0 + t];
      for (int32_t t = (int32_t)threadIdx.x; t <= nlvl; t += (int32_t)blockDim.x) ow_lvl[t] = own_lvl[lvl0 + t];
    }
    if (!SPARSE && q_first < nunits) {
      const double *ap_ = Ac + ((int64_t)(S - 1 - (q_first >> 1)) * lda) * 16 + (lane & 15) + (int64_t)kq * 16;
#pragma unroll
      for (int u = 0; u < KU; ++u) a0[u] = ap_[u * 64];
    }
    // ---- phase 1a: right-hand sides of this wave's rows into LDS (row ids one per lane, eight loads in flight)
    int32_t h_i = 0, h_p = LOWER ? 0 : -1;
    double h_d = 1.0;  // (U: the pivot; fused S1: the row's scale)
    double h_s = 0.0;  // (U, rowflag bit 1: the row's scale)
    const bool from_b = !LOWER && SPARSE && div_u && rs.flag != nullptr;
    const double *bsrc = from_b ? fl.bin.get() : nullptr;
    if (lane < nr) {
      h_i = rowid[s0 + r0 + lane];
      const int hf = (SPARSE && rs.flag) ? (int)rs.flag[s0 + r0 + lane] : 0;
      cd_rowid[r0 + lane] = (hf & 1) ? ~h_i : h_i;  // (negative: not stored)
      if (div_u) h_d = d[h_i];
      if (from_b && (hf & 2)) {
        h_p = fl.p[h_i];
        h_s = fl.s[h_p];
      }
      if (first_l) {
        h_p = fl.p[h_i];
        h_d = fl.s[h_p];
      }
      if (last_u) {
        const int32_t oi = lu.q[h_i];
        cd_oi[r0 + lane] = oi;
        cd_ot[r0 + lane] = lu.t[oi];
      }
    }
    // first item of the wave's entry stream: requested before the right-hand sides are waited for
    int32_t colv = 0, lrv = 0;
    double valv = 0.0;
    if (e0 + lane < e1) {
      colv = mid_col[e0 + lane];
      valv = mid_val[e0 + lane];
      lrv = mid_lrow[e0 + lane];
    }
    for (int j = 0; j < nr; j += 8) {
      double t_[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int32_t i = rl32(first_l ? h_p : h_i, min(j + q, 63));
        const double *src = rhs + (int64_t)i * rstride + rlane;
        if (from_b) {
          const int32_t pb = rl32(h_p, min(j + q, 63));  // (wave-uniform)
          if (pb >= 0) src = bsrc + (int64_t)pb * fl.ldb + min(lane, fl.nrhs - 1);
        }
        t_[q] = (j + q < nr) ? *src : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (j + q < nr) {
          const double hd = rl64(h_d, min(j + q, 63));
          double tq = t_[q];
          if (from_b && rl32(h_p, min(j + q, 63)) >= 0) tq = lane < fl.nrhs ? rl64(h_s, min(j + q, 63)) * tq : 0.0;
          cd_tbuf[((r0 + j + q) << 6) + lane] = div_u ? tq / hd : (first_l ? (lane < fl.nrhs ? hd * tq : 0.0) : tq);
        }
    }
    HIFAMD_CSP(3)
    // ---- phase 1b: the wave's entries, items of 64, eight gathers per batch; the running row's sum stays in a register
    int cur_r = -1;
    double acc = 0.0;
    for (int32_t e = e0; e < ((dbg & 1) ? e0 : e1); e += 64) {
      const int cnt = min(64, e1 - e);
      int32_t colv2 = 0, lrv2 = 0;
      double valv2 = 0.0;
      if (e + 64 + lane < e1) {
        colv2 = mid_col[e + 64 + lane];
        valv2 = mid_val[e + 64 + lane];
        lrv2 = mid_lrow[e + 64 + lane];
      }
      for (int t = 0; t < cnt; t += 8) {
        int32_t j_[8], r_[8];
        double a_[8], xv_[8];
#pragma unroll
        for (int b2 = 0; b2 < 8; ++b2) {
          const int idx = min(t + b2, 63);
          j_[b2] = rl32(colv, idx);
          a_[b2] = rl64(valv, idx);
          r_[b2] = rl32(lrv, idx);
        }
#pragma unroll
        for (int b2 = 0; b2 < 8; ++b2)
          if (t + b2 < cnt) xv_[b2] = x[((int64_t)j_[b2] << 6) + lane];
#pragma unroll
        for (int b2 = 0; b2 < 8; ++b2)
          if (t + b2 < cnt) {
            if (r_[b2] != cur_r) {  // (wave-uniform)
              if (cur_r >= 0) cd_tbuf[(cur_r << 6) + lane] = acc;
              cur_r = r_[b2];
              acc = cd_tbuf[(cur_r << 6) + lane];
            }
            acc = acc - a_[b2] * xv_[b2];
          }
      }
      colv = colv2;
      valv = valv2;
      lrv = lrv2;
    }
    if (cur_r >= 0) cd_tbuf[(cur_r << 6) + lane] = acc;
    // (the inverse product reads whole operand sets of 32 rows: rows nb .. lda - 1 are zero; lds_rows is a multiple of 32)
    if (!SPARSE)
      for (int t = nb * 64 + (int)threadIdx.x; t < lda * 64; t += (int)blockDim.x) cd_tbuf[t] = 0.0;
    HIFAMD_CSP(4)
    __syncthreads();
    HIFAMD_CSP(5)
    if (SPARSE) {
      // ---- phase 2, sparse: substitution inside LDS, depth level by depth level.  The rows of a level are independent;
      // every own source sits in an earlier level (host.hpp build_cd_streams).  A wave takes a row at a time: the row's
      // (value, source) pairs come from LDS, so do the source rows -- no global access on the dependent path.
      const int nlvl = dsc[24];
      if (dbg & 512) {  // (timing experiments: rows stored as they are, no substitution -- WRONG results)
        for (int r = wave; r < nb; r += nw) {
          const double a2 = cd_tbuf[(r << 6) + lane];
          if (last_u) {
            if (lane < lu.nrhs) yout[(int64_t)cd_oi[r] * lu.ldy + lane] = cd_ot[r] * a2;
          } else if (cd_rowid[r] >= 0) {
            x[((int64_t)cd_rowid[r] << 6) + lane] = a2;
          }
        }
        __syncthreads();
        continue;
      }
      for (int lv = 0; lv < nlvl; ++lv) {
        const int r_lo = ow_lvl[lv], r_hi = ow_lvl[lv + 1];
        for (int r = r_lo + wave; r < r_hi; r += nw) {
          double a2 = cd_tbuf[(r << 6) + lane];
          const int eb = ow_rptr[r], ee = ow_rptr[r + 1];
          for (int e = eb; e < ee; ++e) a2 = a2 - ow_val[e] * cd_tbuf[((int)ow_src[e] << 6) + lane];
          if (ee > eb) cd_tbuf[(r << 6) + lane] = a2;
          if (last_u) {
            if (lane < lu.nrhs) yout[(int64_t)cd_oi[r] * lu.ldy + lane] = cd_ot[r] * a2;
          } else {
            const int32_t rid = cd_rowid[r];
            if (rid >= 0) x[((int64_t)rid << 6) + lane] = a2;
          }
        }
        __syncthreads();
      }
      continue;
    }
    // ---- phase 2: x = Tinv * t (units are handed out heaviest first)
    for (int q = q_first; q < ((dbg & 2) ? 0 : nunits); q += nw) {
      const int strip = S - 1 - (q >> 1), ch = q & 1;
      const int kend = min(nb, 16 * (strip + 1));
      const int nsets = (kend + 31) >> 5;
      const double *Ap = Ac + ((int64_t)strip * lda) * 16 + (lane & 15);
      const double *Bp = cd_tbuf + ch * 32 + (lane & 15);
      v4f64 acc0 = v4f64{0.0, 0.0, 0.0, 0.0}, acc1 = acc0;
#define HIFAMD_CD_LOAD(aa, t_)                                          \
  {                                                                     \
    const double *ap_ = Ap + (int64_t)(32 * (t_) + kq) * 16;            \
    _Pragma("unroll") for (int u = 0; u < KU; ++u) aa[u] = ap_[u * 64]; \
  }
#define HIFAMD_CD_MFMA(aa, t_)                                                    \
  {                                                                               \
    const int kb_ = 32 * (t_) + kq;                                               \
    _Pragma("unroll") for (int u = 0; u < KU; ++u) {                              \
      const double b0_ = Bp[(kb_ + 4 * u) << 6];                                  \
      const double b1_ = Bp[((kb_ + 4 * u) << 6) + 16];                           \
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[u], b0_, acc0, 0, 0, 0);     \
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[u], b1_, acc1, 0, 0, 0);     \
    }                                                                             \
  }
      int t = 0;
      if (q != q_first) HIFAMD_CD_LOAD(a0, 0)  // (the first unit's first set was requested before phase 1)
      while (t < nsets) {
        if (t + 1 < nsets) HIFAMD_CD_LOAD(a1, t + 1)
        HIFAMD_CD_MFMA(a0, t)
        if (t + 1 >= nsets) break;
        if (t + 2 < nsets) HIFAMD_CD_LOAD(a0, t + 2)
        HIFAMD_CD_MFMA(a1, t + 1)
        t += 2;
      }
#undef HIFAMD_CD_LOAD
#undef HIFAMD_CD_MFMA
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * strip + kq + 4 * r;
        if (row < nb) {
          if (last_u) {
            const int cc = ch * 32 + (lane & 15);
            double *yo = yout + (int64_t)cd_oi[row] * lu.ldy + cc;
            const double tt = cd_ot[row];
            if (cc < lu.nrhs) yo[0] = tt * acc0[r];
            if (cc + 16 < lu.nrhs) yo[16] = tt * acc1[r];
          } else {
            double *xo = x + ((int64_t)cd_rowid[row] << 6) + ch * 32 + (lane & 15);
            xo[0] = acc0[r];
            xo[16] = acc1[r];
          }
        }
      }
    }
    __syncthreads();  // (the next component overwrites the LDS block)
  }
  HIFAMD_CSP(6)
  HIFAMD_CSP_FLUSH(1 + (LOWER ? 0 : 4) + (SPARSE ? 8 : 0) + 16, n_band, 0)
}

// ---------------------------------------------------------------------------------------------
// Sparse-own U band with streamed sinks (round 4; host.hpp build_us_plan).  One component per workgroup (1,024 threads), R = 64.
//   phase 0  descriptors, the component's own entries / row offsets / black levels into LDS; output rows of a fused S7
//   phase A  the BLACK rows' right-hand sides (w / d, or -- RowSkip -- s b[p] / d) minus their outside entries -> LDS;
//            the first batch of sink right-hand sides is requested here too and arrives during phase B
//   phase B  the black rows level by level in LDS, a wave per row (k_band_cd<false, sparse>'s loop); results stored
//   phase C  the sinks, a wave per row, eight rows of a wave in flight: right-hand side, outside entries, own entries
//            gathered from the black rows in LDS, result stored -- a sink never touches LDS
// Per row: the operations of k_band_cd in the same order -- the same bits (width independence is tested against the slice
// kernel k_band_cs, which narrow batches keep).  LDS: black rows x 512 B + the own entries: two workgroups per compute unit
// on the reference's hierarchies (<= 64 VGPRs), the occupancy the level-0 bands are bound by.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8)))
    k_band_us(int32_t c0, const int32_t *__restrict__ desc, const int32_t *__restrict__ rowid, const int32_t *__restrict__ oslot,
              const int32_t *__restrict__ mptr, const int32_t *__restrict__ mcol, const double *__restrict__ mval,
              const double *__restrict__ own_val, const uint8_t *__restrict__ own_src, const uint16_t *__restrict__ own_rptr,
              const uint8_t *__restrict__ own_lvl, const double *__restrict__ d, const double *__restrict__ w, double *v,
              int32_t lds_black, int32_t own_cap, FirstL<double> fl, LastU<double> lu, RowSkip rs) {
  extern __shared__ double us_tb[];  // [lds_black][64] black rows; then own values, row ids, S7 rows, own sources, offsets, levels
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  constexpr int NW = 16;
  const int32_t *dsc = desc + (int64_t)(c0 + (int32_t)blockIdx.x) * 8;
  const int32_t s0 = dsc[0], nb = dsc[1], nbk = dsc[2], own0 = dsc[3], orp0 = dsc[4], lvl0 = dsc[5], nlvl = dsc[6];
  const BandUsLds lay(lds_black, own_cap);
  double *ow_val = lds_next<double>(us_tb, lay.tb, lay.ow_val);
  double *s_ot = lds_next<double>(ow_val, lay.ow_val, lay.ot);
  int32_t *s_rowid = lds_next<int32_t>(s_ot, lay.ot, lay.rowid);
  int32_t *s_oi = lds_next<int32_t>(s_rowid, lay.rowid, lay.oi);
  uint16_t *ow_rptr = lds_next<uint16_t>(s_oi, lay.oi, lay.ow_rptr);
  uint8_t *ow_src = lds_next<uint8_t>(ow_rptr, lay.ow_rptr, lay.ow_src);
  uint8_t *ow_lvl = lds_next<uint8_t>(ow_src, lay.ow_src, lay.ow_lvl);
  const bool last_u = lu.on();
  const bool from_b = rs.flag != nullptr;
  const double *bsrc = from_b ? fl.bin.get() : nullptr;
  double *yout = last_u ? lu.out.get() : nullptr;
  // ---- phase 0
  const int32_t nown = own_rptr[orp0 + nb];
  for (int32_t t = (int32_t)threadIdx.x; t < nown; t += 1024) {
    ow_val[t] = own_val[own0 + t];
    ow_src[t] = own_src[own0 + t];
  }
  for (int32_t t = (int32_t)threadIdx.x; t <= nb; t += 1024) ow_rptr[t] = own_rptr[orp0 + t];
  for (int32_t t = (int32_t)threadIdx.x; t <= nlvl; t += 1024) ow_lvl[t] = own_lvl[lvl0 + t];
  for (int32_t t = (int32_t)threadIdx.x; t < nb; t += 1024) {
    const int32_t i = rowid[s0 + t];
    const int hf = from_b ? (int)rs.flag[oslot[s0 + t]] : 0;
    s_rowid[t] = (hf & 1) ? ~i : i;  // (negative: not stored)
    if (last_u) {
      const int32_t oi = lu.q[i];
      s_oi[t] = oi;
      s_ot[t] = lu.t[oi];
    }
  }
  // one row's right-hand side as k_band_cd forms it: w[i] / d[i], or (RowSkip bit 1) (s[p[i]] * b[p[i]]) / d[i]
  // lane k of a wave holds the scalars of the wave's k-th row of the batch
  auto row_scalars = [&](int32_t r, bool valid, int32_t &h_i, int32_t &h_p, double &h_d, double &h_s, int32_t &h_m0, int32_t &h_m1) {
    h_i = 0, h_p = -1, h_d = 1.0, h_s = 0.0, h_m0 = 0, h_m1 = 0;
    if (valid) {
      h_i = rowid[s0 + r];
      h_m0 = mptr[s0 + r];
      h_m1 = mptr[s0 + r + 1];
      h_d = d[h_i];
      if (from_b && (rs.flag[oslot[s0 + r]] & 2)) {
        h_p = fl.p[h_i];
        h_s = fl.s[h_p];
      }
    }
  };
  // ---- phase A: black rows w, w + 16, ... (at most 16 per wave: 256 rows / 16 waves), eight at a time
  for (int32_t kb = 0; wave + NW * kb < nbk; kb += 8) {
    int32_t h_i, h_p, h_m0, h_m1;
    double h_d, h_s;
    const int32_t myr = wave + NW * (kb + lane);
    row_scalars(myr, lane < 8 && myr < nbk, h_i, h_p, h_d, h_s, h_m0, h_m1);
    double t_[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int32_t i = rl32(h_i, q), pb = rl32(h_p, q);
      const double *src = (pb >= 0) ? bsrc + (int64_t)pb * fl.ldb + min(lane, fl.nrhs - 1) : w + ((int64_t)i << 6) + lane;
      t_[q] = (wave + NW * (kb + q) < nbk) ? *src : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int32_t r = wave + NW * (kb + q);
      if (r < nbk) {
        double tq = t_[q];
        if (rl32(h_p, q) >= 0) tq = lane < fl.nrhs ? rl64(h_s, q) * tq : 0.0;
        double acc = tq / rl64(h_d, q);
        const int32_t m0 = rl32(h_m0, q), m1 = rl32(h_m1, q);  // (outside entries: few rows of level 0 have any)
        for (int32_t e = m0; e < m1; ++e) acc = acc - mval[e] * v[((int64_t)mcol[e] << 6) + lane];
        us_tb[(r << 6) + lane] = acc;
      }
    }
  }
  // the first batch of sinks: rows nbk + w, nbk + w + 16, ... requested NOW (nothing of the black solve feeds their loads)
  int32_t g_i, g_p, g_m0, g_m1;
  double g_d, g_s;
  double st_[8];
  {
    const int32_t myr = nbk + wave + NW * lane;
    row_scalars(myr, lane < 8 && myr < nb, g_i, g_p, g_d, g_s, g_m0, g_m1);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int32_t i = rl32(g_i, q), pb = rl32(g_p, q);
      const double *src = (pb >= 0) ? bsrc + (int64_t)pb * fl.ldb + min(lane, fl.nrhs - 1) : w + ((int64_t)i << 6) + lane;
      st_[q] = (nbk + wave + NW * q < nb) ? *src : 0.0;
    }
  }
  __syncthreads();
  // ---- phase B: the black rows, depth level by depth level
  for (int lv = 0; lv < nlvl; ++lv) {
    const int r_lo = ow_lvl[lv], r_hi = ow_lvl[lv + 1];
    for (int r = r_lo + wave; r < r_hi; r += NW) {
      double a2 = us_tb[(r << 6) + lane];
      const int eb = ow_rptr[r], ee = ow_rptr[r + 1];
      for (int e = eb; e < ee; ++e) a2 = a2 - ow_val[e] * us_tb[((int)ow_src[e] << 6) + lane];
      if (ee > eb) us_tb[(r << 6) + lane] = a2;
      if (last_u) {
        if (lane < lu.nrhs) yout[(int64_t)s_oi[r] * lu.ldy + lane] = s_ot[r] * a2;
      } else {
        const int32_t rid = s_rowid[r];
        if (rid >= 0) v[((int64_t)rid << 6) + lane] = a2;
      }
    }
    __syncthreads();
  }
  // ---- phase C: the sinks (eight rows of this wave per batch; the first batch is already in registers)
  for (int32_t kb = 0; nbk + wave + NW * kb < nb; kb += 8) {
    if (kb) {
      const int32_t myr = nbk + wave + NW * (kb + lane);
      row_scalars(myr, lane < 8 && myr < nb, g_i, g_p, g_d, g_s, g_m0, g_m1);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int32_t i = rl32(g_i, q), pb = rl32(g_p, q);
        const double *src = (pb >= 0) ? bsrc + (int64_t)pb * fl.ldb + min(lane, fl.nrhs - 1) : w + ((int64_t)i << 6) + lane;
        st_[q] = (nbk + wave + NW * (kb + q) < nb) ? *src : 0.0;
      }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int32_t r = nbk + wave + NW * (kb + q);
      if (r < nb) {
        double tq = st_[q];
        if (rl32(g_p, q) >= 0) tq = lane < fl.nrhs ? rl64(g_s, q) * tq : 0.0;
        double a2 = tq / rl64(g_d, q);
        const int32_t m0 = rl32(g_m0, q), m1 = rl32(g_m1, q);
        for (int32_t e = m0; e < m1; ++e) a2 = a2 - mval[e] * v[((int64_t)mcol[e] << 6) + lane];
        const int eb = ow_rptr[r], ee = ow_rptr[r + 1];
        for (int e = eb; e < ee; ++e) a2 = a2 - ow_val[e] * us_tb[((int)ow_src[e] << 6) + lane];
        if (last_u) {
          if (lane < lu.nrhs) yout[(int64_t)s_oi[r] * lu.ldy + lane] = s_ot[r] * a2;
        } else {
          const int32_t rid = s_rowid[r];
          if (rid >= 0) v[((int64_t)rid << 6) + lane] = a2;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Sparse-own L band with streamed sources (host.hpp build_ls_plan).  One component per workgroup (1,024 threads), R = 64.
// The component's rows are its DEPENDENT rows (they have entries inside the component; new local index < nd) and its
// SOURCES (they have none: their value is final once their outside entries are subtracted).  Wave w owns the dependent
// rows w, w + 16, ... and the sources nd + w + 16 q (register slot q < CW * NCH; chunk q / CW of C = 16 CW rows).
//   phase 0  the component's own entries / segment offsets / levels into LDS; the dependent rows' ids
//   phase 1  every row load of the wave is requested up front (dependent rows and all source slots; clamped rows, no
//            conditional global access); the dependent rows' right-hand sides minus their outside entries go to LDS
//            (k_band_cd's walk: items of 64, eight gathers per batch, the running row's sum in a register); the sources are
//            formed in registers the same way and stored (unless RowSkip says nobody reads them from memory)
//   phase 2  chunk by chunk: the waves deposit their slots of chunk k, barrier, every dependent row subtracts its entries
//            into the chunk (segment k of its own list), barrier
//   phase 3  the dependent rows level by level in LDS over the last segment (k_band_cd<true, sparse>'s loop); stored as
//            they finish
// Per row: right-hand side, outside entries, own entries to sources by ascending source, own entries to dependent rows --
// the order host.hpp ls_reorder_own gives the lists k_band_cd / k_band_cs walk: the same bits at every batch width.
// LDS: (dependent rows + C) x 512 B + the own entries: two workgroups per compute unit (<= 64 VGPRs without scratch up to
// nine register slots: the instances engine.hip ls_kernel lists).
// ---------------------------------------------------------------------------------------------
template <int CW, int NCH>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8)))
    k_band_ls(int32_t c0, const int32_t *__restrict__ desc, const int32_t *__restrict__ rowid, const int32_t *__restrict__ oslot,
              const int32_t *__restrict__ ebase, const uint16_t *__restrict__ ewptr, const int32_t *__restrict__ ecol,
              const double *__restrict__ eval, const uint8_t *__restrict__ etag, const double *__restrict__ own_val,
              const uint8_t *__restrict__ own_src, const uint16_t *__restrict__ own_rptr, const uint8_t *__restrict__ own_lvl,
              double *w, int32_t lds_dep, int32_t own_cap, int32_t rptr_cap, FirstL<double> fl, RowSkip rs) {
  extern __shared__ double ls_tb[];  // [lds_dep][64] dependent rows, [16 CW][64] chunk; own values, row ids, offsets, own sources, levels
  constexpr int NS = CW * NCH, C = 16 * CW;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int32_t comp = c0 + (int32_t)blockIdx.x;
  const int32_t *dsc = desc + (int64_t)comp * 8;
  const int32_t s0 = dsc[0], nb = dsc[1], nd = dsc[2], own0 = dsc[3], orp0 = dsc[4], lvl0 = dsc[5], nlvl = dsc[6], nch = dsc[7];
  const BandLsLds lay(lds_dep, C, own_cap, rptr_cap);
  double *chunk = lds_next<double>(ls_tb, lay.tb, lay.chunk);
  double *ow_val = lds_next<double>(chunk, lay.chunk, lay.ow_val);
  int32_t *s_rowid = lds_next<int32_t>(ow_val, lay.ow_val, lay.rowid);
  uint16_t *ow_rptr = lds_next<uint16_t>(s_rowid, lay.rowid, lay.ow_rptr);
  uint8_t *ow_src = lds_next<uint8_t>(ow_rptr, lay.ow_rptr, lay.ow_src);
  uint8_t *ow_lvl = lds_next<uint8_t>(ow_src, lay.ow_src, lay.ow_lvl);
  const bool first_l = fl.on();
  const double *rhs = first_l ? fl.bin.get() : (const double *)w;
  const int64_t rstride = first_l ? fl.ldb : 64;
  const int rlane = first_l ? min(lane, fl.nrhs - 1) : lane;
  // ---- phase 0
  const int32_t nseg = (nch + 1) * nd;
  const int32_t nown = own_rptr[orp0 + nseg];
  for (int32_t t = (int32_t)threadIdx.x; t < nown; t += 1024) {
    ow_val[t] = own_val[own0 + t];
    ow_src[t] = own_src[own0 + t];
  }
  for (int32_t t = (int32_t)threadIdx.x; t <= nseg; t += 1024) ow_rptr[t] = own_rptr[orp0 + t];
  for (int32_t t = (int32_t)threadIdx.x; t <= nlvl; t += 1024) ow_lvl[t] = own_lvl[lvl0 + t];
  // ---- phase 1: lane j holds the scalars of the wave's j-th dependent row (j < 16) and of its source slot j (j < NS)
  const int32_t dr = min(wave + 16 * lane, nb - 1), sr = min(nd + wave + 16 * lane, nb - 1);  // (clamped: every load is valid)
  const int32_t g_rid = rowid[s0 + sr];
  int32_t d_i = rowid[s0 + dr], g_i = g_rid;
  const int d_f = rs.flag ? (int)rs.flag[oslot[s0 + dr]] : 0, g_f = rs.flag ? (int)rs.flag[oslot[s0 + sr]] : 0;
  if (wave + 16 * lane < nd) s_rowid[dr] = (d_f & 1) ? ~d_i : d_i;  // (negative: not stored)
  const bool g_store = !(g_f & 1);
  double d_s = 1.0, g_s = 1.0;
  if (first_l) {
    d_i = fl.p[d_i], g_i = fl.p[g_i];
    d_s = fl.s[d_i], g_s = fl.s[g_i];
  }
  const int32_t eb0 = ebase[comp];
  const uint16_t *wp = ewptr + (int64_t)comp * 33 + 2 * wave;
  const int32_t ed0 = eb0 + (int32_t)wp[0], es0 = eb0 + (int32_t)wp[1], es1 = eb0 + (int32_t)wp[2];
  // first items of the wave's two entry runs: requested before the right-hand sides are waited for
  const int32_t ad = min(ed0 + lane, max(es0 - 1, ed0)), as = min(es0 + lane, max(es1 - 1, es0));  // (the arrays are padded)
  int32_t colv = ecol[ad], lrv = etag[ad];
  double valv = eval[ad];
  int32_t scol = ecol[as], stag = etag[as];
  double sval = eval[as];
  // the source slots' right-hand sides: all in flight from here on
  double t_[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) t_[q] = rhs[(int64_t)rl32(g_i, q) * rstride + rlane];
  // the dependent rows' right-hand sides into LDS, four at a time
  for (int j = 0; wave + 16 * j < nd; j += 4) {
    double u_[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) u_[q] = rhs[(int64_t)rl32(d_i, min(j + q, 15)) * rstride + rlane];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = wave + 16 * (j + q);
      if (r < nd) ls_tb[(r << 6) + lane] = first_l ? (lane < fl.nrhs ? rl64(d_s, min(j + q, 15)) * u_[q] : 0.0) : u_[q];
    }
  }
  // the dependent rows' outside entries (k_band_cd phase 1b)
  {
    int cur_r = -1;
    double acc = 0.0;
    for (int32_t e = ed0; e < es0; e += 64) {
      const int cnt = min(64, es0 - e);
      const int32_t an = min(e + 64 + lane, es0 - 1);
      const int32_t colv2 = ecol[an], lrv2 = etag[an];
      const double valv2 = eval[an];
      for (int t = 0; t < cnt; t += 8) {
        int32_t j_[8], r_[8];
        double a_[8], xv_[8];
#pragma unroll
        for (int b2 = 0; b2 < 8; ++b2) {
          const int idx = min(t + b2, cnt - 1);
          j_[b2] = rl32(colv, idx);
          a_[b2] = rl64(valv, idx);
          r_[b2] = rl32(lrv, idx);
        }
#pragma unroll
        for (int b2 = 0; b2 < 8; ++b2) xv_[b2] = w[((int64_t)j_[b2] << 6) + lane];
#pragma unroll
        for (int b2 = 0; b2 < 8; ++b2)
          if (t + b2 < cnt) {
            if (r_[b2] != cur_r) {  // (wave-uniform)
              if (cur_r >= 0) ls_tb[(cur_r << 6) + lane] = acc;
              cur_r = r_[b2];
              acc = ls_tb[(cur_r << 6) + lane];
            }
            acc = acc - a_[b2] * xv_[b2];
          }
      }
      colv = colv2, valv = valv2, lrv = lrv2;
    }
    if (cur_r >= 0) ls_tb[(cur_r << 6) + lane] = acc;
  }
  // the sources: scale, outside entries (the same walk, the sums in the slots' registers), store
  if (first_l) {
#pragma unroll
    for (int q = 0; q < NS; ++q) t_[q] = lane < fl.nrhs ? rl64(g_s, q) * t_[q] : 0.0;
  }
  for (int32_t e = es0; e < es1; e += 64) {
    const int cnt = min(64, es1 - e);
    const int32_t an = min(e + 64 + lane, es1 - 1);
    const int32_t scol2 = ecol[an], stag2 = etag[an];
    const double sval2 = eval[an];
    for (int t = 0; t < cnt; t += 8) {
      int32_t j_[8], r_[8];
      double a_[8], xv_[8];
#pragma unroll
      for (int b2 = 0; b2 < 8; ++b2) {
        const int idx = min(t + b2, cnt - 1);
        j_[b2] = rl32(scol, idx);
        a_[b2] = rl64(sval, idx);
        r_[b2] = (t + b2 < cnt) ? rl32(stag, idx) : -1;
      }
#pragma unroll
      for (int b2 = 0; b2 < 8; ++b2) xv_[b2] = w[((int64_t)j_[b2] << 6) + lane];
#pragma unroll
      for (int b2 = 0; b2 < 8; ++b2) {
        const double pr = a_[b2] * xv_[b2];
#pragma unroll
        for (int q = 0; q < NS; ++q)
          if (r_[b2] == q) t_[q] = t_[q] - pr;  // (wave-uniform)
      }
    }
    scol = scol2, sval = sval2, stag = stag2;
  }
#pragma unroll
  for (int q = 0; q < NS; ++q) {
    const bool st = rl32((int32_t)g_store, q) != 0 && nd + wave + 16 * q < nb;  // (wave-uniform)
    if (st) w[((int64_t)rl32(g_rid, q) << 6) + lane] = t_[q];
  }
  // ---- phase 2: the sources pass through the chunk buffer
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    if (k < nch) {  // (workgroup-uniform)
#pragma unroll
      for (int j = 0; j < CW; ++j) chunk[((wave + 16 * j) << 6) + lane] = t_[k * CW + j];
      __syncthreads();
      for (int r = wave; r < nd; r += 16) {
        const int eb = ow_rptr[k * nd + r], ee = ow_rptr[k * nd + r + 1];
        if (ee > eb) {
          double a2 = ls_tb[(r << 6) + lane];
          for (int e = eb; e < ee; ++e) a2 = a2 - ow_val[e] * chunk[((int)ow_src[e] << 6) + lane];
          ls_tb[(r << 6) + lane] = a2;
        }
      }
      __syncthreads();
    }
  }
  if (nch == 0) __syncthreads();  // (a component without dependent rows: nothing follows, but phase 0 wrote LDS)
  // ---- phase 3: the dependent rows, depth level by depth level
  const uint16_t *rp3 = ow_rptr + nch * nd;
  for (int lv = 0; lv < nlvl; ++lv) {
    const int r_lo = ow_lvl[lv], r_hi = ow_lvl[lv + 1];
    for (int r = r_lo + wave; r < r_hi; r += 16) {
      double a2 = ls_tb[(r << 6) + lane];
      const int eb = rp3[r], ee = rp3[r + 1];
      for (int e = eb; e < ee; ++e) a2 = a2 - ow_val[e] * ls_tb[((int)ow_src[e] << 6) + lane];
      if (ee > eb) ls_tb[(r << 6) + lane] = a2;
      const int32_t rid = s_rowid[r];
      if (rid >= 0) w[((int64_t)rid << 6) + lane] = a2;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// Column-sliced component band (round 3).  The same plan, descriptors and packed streams as k_band_cd, but a workgroup
// solves ONE component for a SLICE of 16 right-hand-side columns: blockIdx.x = component-workgroup * nsl + slice, and
// every step of the solve is column-separable, so the nsl slices of a component never talk to each other.  Why:
//   * a narrow band (tens to a few hundred components: everything above the leaves of a triangle) lasts as long as ONE
//     compute unit needs for its heaviest component -- sliced four ways, that component's gathers, its inverse product
//     and its loads / stores run on four units at once (the critical path shrinks, the launch count does not change);
//   * a batch of fewer than 49 columns launches only the slices it has: nrhs <= 16 moves a quarter of the vector bytes
//     and issues a quarter of the gathers of the 64-column kernel (BASELINE configs[1] and [4]).
// Mapping: 4 waves; a wave is four ROWS of 16 lanes (lane = 16 g + c: column cbase + c).  Lane group q = 4 wave + g
// takes chunk q of the descriptor's sixteen row / entry chunks (k_band_cd gives chunk q to wave q): it loads its rows'
// right-hand sides into LDS, then walks ITS entries -- (column, value, local row) fetched 16 at a time with one
// coalesced load per lane group and broadcast inside the 16 lanes with DPP row_newbcast (a VALU move: no LDS, no
// scalar round trip), eight 128-byte gathers per lane group in flight, the four lane groups of a wave in lock step.
// Arithmetic per row and column is EXACTLY k_band_cd's (rhs, then the entries subtracted one by one in stream order;
// the inverse product accumulated over k in steps of four from k = 0): both kernels give the same bits, whatever
// the slicing -- a column's result does not depend on the width of the batch it travels in.
// Workgroups beyond n_band * nsl run the carried prefix of the next band (full 64-column rows, as in k_band_cd).
// ---------------------------------------------------------------------------------------------
template <int IDX>
__device__ __forceinline__ int32_t bc16(int32_t v) {  // lane IDX of every 16-lane row, to all lanes of that row
  return __builtin_amdgcn_update_dpp(0, v, 0x150 + IDX, 0xf, 0xf, false);
}
template <int IDX>
__device__ __forceinline__ double bc16(double v) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)bc16<IDX>((int32_t)(b & 0xffffffffLL));
  const unsigned hi = (unsigned)bc16<IDX>((int32_t)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>());
    static_for<I + 1, N>(f);
  }
}
__device__ __forceinline__ int wave_max4(int v) {  // max over the four 16-lane rows of a wave (v uniform inside a row)
  return max(max(rl32(v, 0), rl32(v, 16)), max(rl32(v, 32), rl32(v, 48)));
}

// eight entries of every lane group (positions T0 .. T0+7 of the current item), see k_band_cs phase 1b
template <int T0>
__device__ __forceinline__ void cs_batch(int32_t colv, double valv, int32_t lrv, int32_t left, const double *__restrict__ x,
                                         int cc, int l16, double *tb, int &cur, double &acc) {
  int32_t j_[8], r_[8];
  double a_[8], xv_[8], rv_[8];
  bool nw_[8];
  static_for<0, 8>([&](auto ic) {
    constexpr int u = decltype(ic)::value;
    j_[u] = bc16<T0 + u>(colv);
    a_[u] = bc16<T0 + u>(valv);
    r_[u] = bc16<T0 + u>(lrv);
  });
#pragma unroll
  for (int u = 0; u < 8; ++u) xv_[u] = (T0 + u < left) ? x[((int64_t)j_[u] << 6) + cc] : 0.0;
  // right-hand sides of the rows that START in this batch: requested beside the gathers (a lane group meets its rows
  // once, in order, and nobody else touches them in this phase)
  int prev = cur;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    nw_[u] = (T0 + u < left) && r_[u] != prev;
    rv_[u] = nw_[u] ? tb[(r_[u] << 4) + l16] : 0.0;
    if (T0 + u < left) prev = r_[u];
  }
#pragma unroll
  for (int u = 0; u < 8; ++u)
    if (T0 + u < left) {
      if (nw_[u]) {
        if (cur >= 0) tb[(cur << 4) + l16] = acc;
        cur = r_[u];
        acc = rv_[u];
      }
      acc = acc - a_[u] * xv_[u];
    }
}

template <bool LOWER, bool SPARSE>
__global__ void __launch_bounds__(256) k_band_cs(int32_t wg0, const int32_t *__restrict__ wg_grp_ptr,
                                                 const int32_t *__restrict__ cd_desc, const int32_t *__restrict__ ptr,
                                                 const int32_t *__restrict__ split, const int32_t *__restrict__ col,
                                                 const double *__restrict__ val, const int32_t *__restrict__ rowid,
                                                 const double *__restrict__ d, double *w, double *v,
                                                 const double *__restrict__ tinv, const int32_t *__restrict__ mid_col,
                                                 const double *__restrict__ mid_val, const uint8_t *__restrict__ mid_lrow,
                                                 int first_u, int32_t n_band, int32_t nsl, int32_t ps0, int32_t ps1,
                                                 int32_t single_c0, int32_t lds_rows, int32_t own_cap, int dbg, FirstL<double> fl,
                                                 const double *__restrict__ own_val, const uint8_t *__restrict__ own_lsrc,
                                                 const uint16_t *__restrict__ own_rptr, const uint8_t *__restrict__ own_lvl,
                                                 LastU<double> lu, RowSkip rs) {
  extern __shared__ double cs_buf[];
  HIFAMD_CSP_DECL
  HIFAMD_CSP(0)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int32_t nbw = n_band * nsl;
  if (dbg & 8) return;  // (timing experiments: the bare launch)
  if ((int32_t)blockIdx.x >= nbw) {  // carried prefix of the next band over the sources older than this band
    const int32_t pw = __builtin_amdgcn_readfirstlane(((int32_t)blockIdx.x - nbw) * 4 + wave);
    if (dbg & 4) return;
    band_carried_prefix<LOWER>(pw, ((int32_t)gridDim.x - nbw) * 4, ps0, ps1, ptr, split, col, val, rowid, d, w, v, lane, fl);
    HIFAMD_CSP(6)
    HIFAMD_CSP_FLUSH(2 + (LOWER ? 0 : 4), n_band, nsl)
    return;
  }
  const int32_t bw = (int32_t)blockIdx.x / nsl, slice = (int32_t)blockIdx.x - bw * nsl;
  const int grp = lane >> 4, l16 = lane & 15, gq = wave * 4 + grp;  // lane group gq of 16 owns chunk gq
  const int cc = slice * 16 + l16;                                   // this lane's column of the 64-column arena
  double *x = LOWER ? w : v;
  const BandRhs<double> br = band_rhs<LOWER>(first_u, fl, w, x);
  const bool div_u = br.div_u, first_l = br.first_l;
  const double *rhs = br.rhs;
  const int64_t rstride = br.rstride;
  const int rcol = br.col(cc, fl);
  int32_t c_first, c_last;
  band_components(single_c0, wg_grp_ptr, wg0, bw, c_first, c_last);
  // LDS: right-hand sides [lds_rows][16], then per row: pivot / scale, output scale, row id, input row, output row;
  // sparse-own plans: the component's own nonzeros (value, local source), row offsets, depth levels
  const BandCsLds lay(lds_rows, SPARSE, own_cap);
  double *tb = cs_buf;
  double *s_hd = lds_next<double>(tb, lay.tb, lay.hd);
  double *s_ot = lds_next<double>(s_hd, lay.hd, lay.ot);
  double *ow_val = lds_next<double>(s_ot, lay.ot, lay.ow_val);
  int32_t *s_rowid = lds_next<int32_t>(ow_val, lay.ow_val, lay.rowid);
  int32_t *s_hp = lds_next<int32_t>(s_rowid, lay.rowid, lay.hp);
  int32_t *s_oi = lds_next<int32_t>(s_hp, lay.hp, lay.oi);
  uint16_t *ow_rptr = lds_next<uint16_t>(s_oi, lay.oi, lay.ow_rptr);
  uint8_t *ow_src = lds_next<uint8_t>(ow_rptr, lay.ow_rptr, lay.ow_src);
  uint8_t *ow_lvl = lds_next<uint8_t>(ow_src, lay.ow_src, lay.ow_lvl);
  const bool last_u = !LOWER && lu.on();
  double *yout = last_u ? lu.out.get() : nullptr;
  const int kq = grp;
  // (RowSkip: a row of the U solve whose right-hand side comes from the level's input keeps p[i] in s_hp -- -1 otherwise --
  // and its scale in s_ot; the fused S7 never meets the flags: they belong to a level's first solve)
  const bool from_b = !LOWER && SPARSE && div_u && rs.flag != nullptr;
  const double *bsrc = from_b ? fl.bin.get() : nullptr;
  for (int32_t c = c_first; c < c_last; ++c) {
    const int32_t *dsc = cd_desc + (int64_t)c * 28;
    const int32_t s0 = dsc[0], nb = dsc[1], mid0 = dsc[2];
    const int64_t inv_off = ((int64_t)(uint32_t)dsc[5] << 32) | (uint32_t)dsc[4];
    const uint8_t *wrow = reinterpret_cast<const uint8_t *>(dsc + 6);
    const uint16_t *wmid = reinterpret_cast<const uint16_t *>(dsc + 11);
    const int r0 = wrow[gq], nr = (int)wrow[gq + 1] - r0;
    const int32_t e0 = mid0 + (int32_t)wmid[gq], ne = (int32_t)wmid[gq + 1] - (int32_t)wmid[gq];
    const int lda = (nb + 31) & ~31;
    const double *Ac = tinv + inv_off;
    const int S = (nb + 15) >> 4;
    constexpr int KU = 8;
    double a0[KU], a1[KU];
    // ---- phase 0: the component's row ids and per-row scalars (coalesced), sparse: its own nonzeros
    for (int32_t t = (int32_t)threadIdx.x; t < nb; t += 256) {
      const int32_t i = rowid[s0 + t];
      const int hf = (SPARSE && rs.flag) ? (int)rs.flag[s0 + t] : 0;
      s_rowid[t] = (hf & 1) ? ~i : i;  // (negative: not stored)
      if (div_u) s_hd[t] = d[i];
      if (from_b) {
        int32_t pp = -1;
        if (hf & 2) {
          pp = fl.p[i];
          s_ot[t] = fl.s[pp];
        }
        s_hp[t] = pp;
      }
      if (first_l) {
        const int32_t pp = fl.p[i];
        s_hp[t] = pp;
        s_hd[t] = fl.s[pp];
      }
      if (last_u) {
        const int32_t oi = lu.q[i];
        s_oi[t] = oi;
        s_ot[t] = lu.t[oi];
      }
    }
    if (SPARSE) {
      const int32_t own0 = dsc[20], nown = dsc[21], orp0 = dsc[22], lvl0 = dsc[23], nlvl = dsc[24];
      for (int32_t t = (int32_t)threadIdx.x; t < nown; t += 256) {
        ow_val[t] = own_val[own0 + t];
        ow_src[t] = own_lsrc[own0 + t];
      }
      for (int32_t t = (int32_t)threadIdx.x; t <= nb; t += 256) ow_rptr[t] = own_rptr[orp0 + t];
      for (int32_t t = (int32_t)threadIdx.x; t <= nlvl; t += 256) ow_lvl[t] = own_lvl[lvl0 + t];
    }
    // phase 2's first operand set and phase 1b's first item do not depend on anything computed here: requested now
    if (!SPARSE && wave < S) {
      const double *ap_ = Ac + ((int64_t)(S - 1 - wave) * lda) * 16 + l16 + (int64_t)kq * 16;
#pragma unroll
      for (int u = 0; u < KU; ++u) a0[u] = ap_[u * 64];
    }
    int32_t colv = 0, lrv = 0;
    double valv = 0.0;
    if (l16 < ne) {
      colv = mid_col[e0 + l16];
      valv = mid_val[e0 + l16];
      lrv = mid_lrow[e0 + l16];
    }
    HIFAMD_CSP(1)
    __syncthreads();
    HIFAMD_CSP(2)
    if (dbg & 16) return;  // (timing experiments: descriptor + row ids only)
    // ---- phase 1a: right-hand sides of this lane group's rows into LDS, eight rows in flight
    const int nrmax = wave_max4(nr);
    for (int j = 0; j < nrmax; j += 8) {
      double t_[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int r = r0 + min(j + q, max(nr - 1, 0));
        const int32_t rid = s_rowid[r];
        const int32_t i = first_l ? s_hp[r] : (rid < 0 ? ~rid : rid);
        const double *src = rhs + (int64_t)i * rstride + rcol;
        if (from_b) {
          const int32_t pb = s_hp[r];
          if (pb >= 0) src = bsrc + (int64_t)pb * fl.ldb + min(cc, fl.nrhs - 1);
        }
        t_[q] = (j + q < nr) ? *src : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (j + q < nr) {
          const double hd = s_hd[r0 + j + q];
          double tq = t_[q];
          if (from_b && s_hp[r0 + j + q] >= 0) tq = cc < fl.nrhs ? s_ot[r0 + j + q] * tq : 0.0;
          tb[((r0 + j + q) << 4) + l16] = div_u ? tq / hd : (first_l ? (cc < fl.nrhs ? hd * tq : 0.0) : tq);
        }
    }
    HIFAMD_CSP(3)
    if (dbg & 32) return;  // (timing experiments: ... + right-hand sides)
    // ---- phase 1b: this lane group's entries, items of 16, eight gathers per batch, the running row's value in a register
    int cur = -1;
    double acc = 0.0;
    const int32_t nemax = (dbg & 1) ? 0 : wave_max4(ne);
    for (int32_t base = 0; base < nemax; base += 16) {
      int32_t colv2 = 0, lrv2 = 0;
      double valv2 = 0.0;
      if (base + 16 + l16 < ne) {
        colv2 = mid_col[e0 + base + 16 + l16];
        valv2 = mid_val[e0 + base + 16 + l16];
        lrv2 = mid_lrow[e0 + base + 16 + l16];
      }
      const int32_t left = ne - base;  // entries of this lane group from `base` on (may be <= 0)
      cs_batch<0>(colv, valv, lrv, left, x, cc, l16, tb, cur, acc);
      if (base + 8 < nemax) cs_batch<8>(colv, valv, lrv, left, x, cc, l16, tb, cur, acc);
      colv = colv2;
      valv = valv2;
      lrv = lrv2;
    }
    if (cur >= 0) tb[(cur << 4) + l16] = acc;
    if (!SPARSE)  // (rows nb .. lda - 1 are zero for the inverse product; lds_rows is a multiple of 32)
      for (int t = nb * 16 + (int)threadIdx.x; t < lda * 16; t += 256) tb[t] = 0.0;
    HIFAMD_CSP(4)
    __syncthreads();
    HIFAMD_CSP(5)
    if (SPARSE) {
      // ---- phase 2, sparse: substitution inside LDS, depth level by depth level; a lane group takes a row at a time
      const int nlvl = dsc[24];
      for (int lv = 0; lv < nlvl; ++lv) {
        const int r_lo = ow_lvl[lv], r_hi = ow_lvl[lv + 1];
        for (int r = r_lo + gq; r < r_hi; r += 16) {
          double a2 = tb[(r << 4) + l16];
          const int eb = ow_rptr[r], ee = ow_rptr[r + 1];
          for (int e = eb; e < ee; ++e) a2 = a2 - ow_val[e] * tb[((int)ow_src[e] << 4) + l16];
          if (ee > eb) tb[(r << 4) + l16] = a2;
          if (last_u) {
            if (cc < lu.nrhs) yout[(int64_t)s_oi[r] * lu.ldy + cc] = s_ot[r] * a2;
          } else {
            const int32_t rid = s_rowid[r];
            if (rid >= 0) x[((int64_t)rid << 6) + cc] = a2;
          }
        }
        __syncthreads();
      }
      continue;
    }
    // ---- phase 2: x = Tinv * t on the matrix cores, one 16-row strip x this slice's 16 columns per step; strips are
    // dealt heaviest first in snake order over the four waves
    for (int rnd = 0;; ++rnd) {
      const int q = 4 * rnd + ((rnd & 1) ? 3 - wave : wave);
      if (q >= ((dbg & 2) ? 0 : S)) {
        if (4 * rnd >= S) break;
        continue;
      }
      const int strip = S - 1 - q;
      const int kend = min(nb, 16 * (strip + 1));
      const int nsets = (kend + 31) >> 5;
      const double *Ap = Ac + ((int64_t)strip * lda) * 16 + l16;
      const double *Bp = tb + l16;
      v4f64 acc0 = v4f64{0.0, 0.0, 0.0, 0.0};
#define HIFAMD_CS_LOAD(aa, t_)                                          \
  {                                                                     \
    const double *ap_ = Ap + (int64_t)(32 * (t_) + kq) * 16;            \
    _Pragma("unroll") for (int u = 0; u < KU; ++u) aa[u] = ap_[u * 64]; \
  }
#define HIFAMD_CS_MFMA(aa, t_)                                                \
  {                                                                           \
    const int kb_ = 32 * (t_) + kq;                                           \
    _Pragma("unroll") for (int u = 0; u < KU; ++u) {                          \
      const double b0_ = Bp[(kb_ + 4 * u) << 4];                              \
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[u], b0_, acc0, 0, 0, 0); \
    }                                                                         \
  }
      int t = 0;
      if (rnd != 0) HIFAMD_CS_LOAD(a0, 0)  // (the first strip's first set was requested before phase 1)
      while (t < nsets) {
        if (t + 1 < nsets) HIFAMD_CS_LOAD(a1, t + 1)
        HIFAMD_CS_MFMA(a0, t)
        if (t + 1 >= nsets) break;
        if (t + 2 < nsets) HIFAMD_CS_LOAD(a0, t + 2)
        HIFAMD_CS_MFMA(a1, t + 1)
        t += 2;
      }
#undef HIFAMD_CS_LOAD
#undef HIFAMD_CS_MFMA
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * strip + kq + 4 * r;
        if (row < nb) {
          if (last_u) {
            if (cc < lu.nrhs) yout[(int64_t)s_oi[row] * lu.ldy + cc] = s_ot[row] * acc0[r];
          } else {
            x[((int64_t)s_rowid[row] << 6) + cc] = acc0[r];
          }
        }
      }
    }
    __syncthreads();  // (the next component overwrites the LDS block)
  }
  HIFAMD_CSP(6)
  HIFAMD_CSP_FLUSH(1 + (LOWER ? 0 : 4) + (SPARSE ? 8 : 0), n_band, nsl)
}

// ---------------------------------------------------------------------------------------------
// Component band on coefficient TILES (round 4; host.hpp build_ct_tiles).  Same plan, same launch shape as k_band_cs
// (blockIdx.x = component-workgroup * nsl + slice of 16 columns, four waves, carried-prefix workgroups behind), but the
// entries a component reads from rows finished by earlier launches are not walked one by one: per 16-row strip of the
// component the host has cut the strip's distinct sources into groups of four and written the 16 x 4 coefficient tile of
// every group; a wave owns whole strips (descriptor words 22 / 23) and spends ONE v_mfma_f64_16x16x4 per tile,
//     acc[16 rows][16 columns] += coef[16 x 4] * x[4 gathered source rows][16 columns],
// -- a dozen entries per matrix instruction on the reference's 1M-row hierarchies instead of a dozen instructions per
// entry -- with the tile's four source rows gathered once (a lane loads the 8 bytes of ITS source row k = lane / 16,
// column lane % 16: the B operand needs no shuffle, no LDS).  The wave then forms t = rhs - acc for its strips (S1 /
// the pivot division fused as in k_band_cd) straight into LDS; phase 2, the product with the component's explicit
// inverse, makes k_band_cs's sums in k_band_cs's order (its operand sets are requested two ahead, across the strips of
// a wave).  Column-separable like every kernel here: a column's bits do not depend on the batch width,
// so this kernel serves narrow batches (nsl < 4) and full ones alike.  Summation order: tile by tile (tolerance-level).
// ---------------------------------------------------------------------------------------------
// AHEAD (on unless bit 2048 of the development switch is set, engine.hip kDbgCtPlain): phase 1 keeps a strip's source ids two batches, its gathers and coefficient
// tiles one batch ahead of the products (below); off: ids and coefficients one batch ahead, the gathers of a batch
// requested in front of its own products.  The same sums in the same order: the same bits.
// amdgpu_waves_per_eu: the occupancy the register budget is made for (three waves per SIMD; all four column tiles: two).
// Without it the allocator takes what 256 threads allow and keeps the accumulators in AGPRs, with copies around every trip.
template <bool LOWER, int NCT, bool AHEAD>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NCT == 4 ? 2 : 3)))
k_band_ct(int32_t wg0, const int32_t *__restrict__ wg_grp_ptr,
                                                 const int32_t *__restrict__ ct_desc, const int32_t *__restrict__ ptr,
                                                 const int32_t *__restrict__ split, const int32_t *__restrict__ col,
                                                 const double *__restrict__ val, const int32_t *__restrict__ rowid,
                                                 const double *__restrict__ d, double *w, double *v,
                                                 const double *__restrict__ tinv, const int32_t *__restrict__ ct_sptr,
                                                 const int32_t *__restrict__ ct_src, const double *__restrict__ ct_coef,
                                                 int first_u, int32_t n_band, int32_t nsl, int32_t ps0, int32_t ps1,
                                                 int32_t single_c0, int32_t lds_rows, int dbg, FirstL<double> fl,
                                                 LastU<double> lu) {
  extern __shared__ double cs_buf[];
  HIFAMD_CSP_DECL
  HIFAMD_CSP(0)
  constexpr int W = 16 * NCT;           // columns of this workgroup's slice
  constexpr int BU = NCT == 1 ? 8 : (NCT == 2 ? 4 : 2);  // tiles per batch (one batch in flight ahead of the one being multiplied)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // blocks [0, nbp): component-workgroup x slice, laid out so that the slices of a component sit 8 blocks apart (blocks
  // are dealt round-robin over the eight XCDs: the slices then share one L2 -- the component's tiles and inverse are
  // fetched from HBM once; placement is a speed matter only)
  const int32_t nbp = ((n_band + 7) >> 3) * 8 * nsl;
  // (dbg & 128: the carried workgroups take the FIRST block numbers instead of the last)
  const int32_t ncar = (int32_t)gridDim.x - nbp;
  const bool car_first = (dbg & 128) != 0;
  const int32_t bx = car_first ? (int32_t)blockIdx.x - ncar : (int32_t)blockIdx.x;
  if (car_first ? bx < 0 : bx >= nbp) {  // carried prefix of the next band over the sources older than this band
    const int32_t pw = __builtin_amdgcn_readfirstlane((car_first ? (int32_t)blockIdx.x : bx - nbp) * 4 + wave);
    if (dbg & 4) return;
    band_carried_prefix<LOWER>(pw, ncar * 4, ps0, ps1, ptr, split, col, val, rowid, d, w, v, lane, fl);
    HIFAMD_CSP(6)
    HIFAMD_CSP_FLUSH(2 + (LOWER ? 0 : 4) + 32, n_band, nsl)
    return;
  }
  const int32_t bgrp = bx / (8 * nsl), brem = bx - bgrp * 8 * nsl;
  const int32_t slice = brem >> 3, bw = bgrp * 8 + (brem & 7);
  if (bw >= n_band) return;
  const int kq = lane >> 4, l16 = lane & 15;
  const int cc = slice * W + l16;  // this lane's column of the 64-column arena (first column tile)
  double *x = LOWER ? w : v;
  const BandRhs<double> br = band_rhs<LOWER>(first_u, fl, w, x);
  const bool div_u = br.div_u, first_l = br.first_l;
  const double *rhs = br.rhs;
  const int64_t rstride = br.rstride;
  // The batch's input and output blocks arrive as pointers read from memory (IoPtr): the compiler takes them for generic
  // addresses, and ONE generic access anywhere in the kernel makes every later wait for a load a wait for ALL loads (a
  // generic access may return out of order) -- phase 2's counted waits would be lost.  Both blocks are device memory:
  typedef __attribute__((address_space(1))) double gdouble;
  const gdouble *rhs_g = (const gdouble *)rhs;
  typedef __attribute__((address_space(1))) int32_t gint32;
  const gdouble *x_g = (const gdouble *)x, *coef_g = (const gdouble *)ct_coef;
  const gint32 *src_g = (const gint32 *)ct_src;
  int32_t c_first, c_last;
  band_components(single_c0, wg_grp_ptr, wg0, bw, c_first, c_last);
  // LDS: right-hand sides [lds_rows][W], per row: pivot / scale, output scale, row id, input row, output row; the
  // component's strip -> tile offsets
  const BandCtLds lay(lds_rows, NCT);
  double *tb = cs_buf;
  double *s_hd = lds_next<double>(tb, lay.tb, lay.hd);
  double *s_ot = lds_next<double>(s_hd, lay.hd, lay.ot);
  int32_t *s_rowid = lds_next<int32_t>(s_ot, lay.ot, lay.rowid);
  int32_t *s_hp = lds_next<int32_t>(s_rowid, lay.rowid, lay.hp);
  int32_t *s_oi = lds_next<int32_t>(s_hp, lay.hp, lay.oi);
  int32_t *s_sptr = lds_next<int32_t>(s_oi, lay.oi, lay.sptr);  // 17 entries (a component has at most 16 strips)
  const bool last_u = !LOWER && lu.on();
  gdouble *yout = last_u ? (gdouble *)lu.out.get() : nullptr;
  constexpr int KU = 8;
  for (int32_t c = c_first; c < c_last; ++c) {
    const int32_t *dsc = ct_desc + (int64_t)c * 28;
    const int32_t s0 = dsc[0], nb = dsc[1], sp0 = dsc[20];
    const int64_t inv_off = ((int64_t)(uint32_t)dsc[5] << 32) | (uint32_t)dsc[4];
    const uint32_t mword = (uint32_t)dsc[22 + (wave >> 1)];
    const uint32_t mymask = (wave & 1) ? (mword >> 16) : (mword & 0xffffu);  // the strips this wave owns
    const int lda = (nb + 31) & ~31;
    const double *Ac = tinv + inv_off;
    const int S = (nb + 15) >> 4;
    double a0[KU], a1[KU];
    // ---- phase 0: the component's row ids, per-row scalars and strip offsets (coalesced)
    for (int32_t t = (int32_t)threadIdx.x; t < nb; t += 256) {
      const int32_t i = rowid[s0 + t];
      s_rowid[t] = i;
      if (div_u) s_hd[t] = d[i];
      if (first_l) {
        const int32_t pp = fl.p[i];
        s_hp[t] = pp;
        s_hd[t] = fl.s[pp];
      }
      if (last_u) {
        const int32_t oi = lu.q[i];
        s_oi[t] = oi;
        s_ot[t] = lu.t[oi];
      }
    }
    if ((int32_t)threadIdx.x <= S) s_sptr[threadIdx.x] = ct_sptr[sp0 + (int32_t)threadIdx.x];
    // phase 2's first operand set does not depend on anything computed here: a narrow band (one 16-column slice per
    // workgroup) requests it NOW -- its launch is a chain of round trips, and this one then hides behind phase 1
    if (NCT == 1 && !(dbg & 256) && wave < S) {
      const double *ap_ = Ac + ((int64_t)(S - 1 - wave) * lda) * 16 + l16 + (int64_t)kq * 16;
#pragma unroll
      for (int u = 0; u < KU; ++u) a0[u] = ap_[u * 64];
    }
    HIFAMD_CSP(1)
    __syncthreads();
    HIFAMD_CSP(2)
    // ---- phase 1: this wave's strips -- right-hand sides requested first, then the strip's tiles BU at a time (the
    // next BU source ids and coefficient tiles are in flight while the current ones are gathered and multiplied)
    for (int s = 0; s < S; ++s) {
      if (!((mymask >> s) & 1u)) continue;  // (wave-uniform)
      double tr[NCT][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = min(16 * s + kq + 4 * j, nb - 1);
        const int32_t i = first_l ? s_hp[row] : s_rowid[row];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
          const int cx = cc + 16 * ct;
          tr[ct][j] = rhs_g[(int64_t)i * rstride + (first_l ? min(cx, fl.nrhs - 1) : cx)];
        }
      }
      const int32_t t0v = s_sptr[s], t1v = (dbg & 1) ? t0v : s_sptr[s + 1];
      v4f64 acc[NCT];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc[ct] = v4f64{0.0, 0.0, 0.0, 0.0};
      if (AHEAD && t0v < t1v) {
        // Batches of BU tiles; three request streams run ahead of the products, every load unconditional (a tile index
        // past the strip's last tile reads that tile again; its coefficient is replaced by zero where it is multiplied,
        // and a batch wholly past the end is never multiplied).  At the top of the step that multiplies batch b the ids
        // of batch b + 1 and the gathers and coefficients of batch b are in flight, in that order; the step requests the
        // ids of batch b + 2, then -- the ids of b + 1 have arrived, the wait leaves batch b's operands in flight -- the
        // gathers and coefficients of batch b + 1, and only then multiplies batch b: its wait leaves everything the step
        // requested in flight.  Two register sets of each kind rotate by name over a loop of two steps.
        // (the strip's tile range is wave-uniform: said so, tile indices and clamps are scalar work)
        const int32_t t0 = __builtin_amdgcn_readfirstlane(t0v), t1 = __builtin_amdgcn_readfirstlane(t1v);
        uint32_t ia[BU], ib[BU];  // (row ids are not negative: widened by zero, nothing waits for the load that early)
        double ca[BU], cb[BU], ga[NCT][BU], gb[NCT][BU];
#define HIFAMD_CT_IDS(ii, tb_)                                                                   \
  _Pragma("unroll") for (int u = 0; u < BU; ++u) ii[u] = (uint32_t)src_g[4 * (int64_t)min((tb_) + u, t1 - 1) + kq];
#define HIFAMD_CT_OPS(gg, cf, ii, tb_)                                                           \
  {                                                                                              \
    _Pragma("unroll") for (int u = 0; u < BU; ++u) {                                             \
      _Pragma("unroll") for (int ct = 0; ct < NCT; ++ct) gg[ct][u] = x_g[((uint64_t)ii[u] << 6) + (uint32_t)(cc + 16 * ct)]; \
    }                                                                                            \
    _Pragma("unroll") for (int u = 0; u < BU; ++u) cf[u] = coef_g[64 * (int64_t)min((tb_) + u, t1 - 1) + lane]; \
  }
#define HIFAMD_CT_MUL(gg, cf, tb_)                                                               \
  _Pragma("unroll") for (int u = 0; u < BU; ++u) {                                               \
    const double c_ = ((tb_) + u < t1) ? cf[u] : 0.0;                                            \
    _Pragma("unroll") for (int ct = 0; ct < NCT; ++ct)                                           \
      acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(c_, gg[ct][u], acc[ct], 0, 0, 0);           \
  }
        // ifree: the id set whose gathers are out; inext: the ids of the batch behind the one being multiplied
#define HIFAMD_CT_AHEAD_STEP(ifree, inext, gcur, ccur, gnew, cnew, tb_)                          \
  {                                                                                              \
    HIFAMD_CT_IDS(ifree, (tb_) + 2 * BU)                                                         \
    __builtin_amdgcn_sched_barrier(0); /* (the ids lead: the next step's wait for them is counted) */ \
    HIFAMD_CT_OPS(gnew, cnew, inext, (tb_) + BU)                                                 \
    __builtin_amdgcn_sched_barrier(0); /* (the requests stay in front of the products) */        \
    HIFAMD_CT_MUL(gcur, ccur, tb_)                                                               \
    _Pragma("unroll") for (int ct = 0; ct < NCT; ++ct) asm volatile("" : "+v"(acc[ct]));         \
  }
        HIFAMD_CT_IDS(ia, t0)
        HIFAMD_CT_IDS(ib, t0 + BU)
        // (the second id set is touched here, or its request sinks into the loop's entry, behind batch 0's operands: the
        // loop's first wait for ids would then be a wait for those operands, on every trip)
#pragma unroll
        for (int u = 0; u < BU; ++u) pin_here(ib[u]);
        HIFAMD_CT_OPS(ga, ca, ia, t0)
        int32_t t = t0;
        for (; t + BU < t1; t += 2 * BU) {  // (one exit, at the top; two batches per trip)
          HIFAMD_CT_AHEAD_STEP(ia, ib, ga, ca, gb, cb, t)
          HIFAMD_CT_AHEAD_STEP(ib, ia, gb, cb, ga, ca, t + BU)
        }
        if (t < t1) {  // the strip's last batch: in registers or on its way
          HIFAMD_CT_MUL(ga, ca, t)
        }
#undef HIFAMD_CT_AHEAD_STEP
#undef HIFAMD_CT_MUL
#undef HIFAMD_CT_OPS
#undef HIFAMD_CT_IDS
      }
      if (!AHEAD && t0v < t1v) {
        const int32_t t0 = t0v, t1 = t1v;
        int32_t sv[BU];
        double cv[BU];
#pragma unroll
        for (int u = 0; u < BU; ++u) {
          const int32_t tt = min(t0 + u, t1 - 1);
          sv[u] = ct_src[4 * (int64_t)tt + kq];
          cv[u] = ct_coef[64 * (int64_t)tt + lane];
          if (t0 + u >= t1) cv[u] = 0.0;
        }
        for (int32_t t = t0; t < t1; t += BU) {
          double bv[NCT][BU];
#pragma unroll
          for (int u = 0; u < BU; ++u)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) bv[ct][u] = x[((int64_t)sv[u] << 6) + cc + 16 * ct];
          int32_t sn[BU];
          double cn[BU];
#pragma unroll
          for (int u = 0; u < BU; ++u) {  // (clamped: the loads past the strip's last tile read that tile again, weight zero)
            const int32_t tt = min(t + BU + u, t1 - 1);
            sn[u] = ct_src[4 * (int64_t)tt + kq];
            cn[u] = ct_coef[64 * (int64_t)tt + lane];
            if (t + BU + u >= t1) cn[u] = 0.0;
          }
#pragma unroll
          for (int u = 0; u < BU; ++u)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(cv[u], bv[ct][u], acc[ct], 0, 0, 0);
#pragma unroll
          for (int u = 0; u < BU; ++u) sv[u] = sn[u], cv[u] = cn[u];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = 16 * s + kq + 4 * j;
        if (row < nb) {
          const double hd = (div_u || first_l) ? s_hd[row] : 1.0;
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) {
            const double t_ = div_u ? tr[ct][j] / hd : (first_l ? (cc + 16 * ct < fl.nrhs ? hd * tr[ct][j] : 0.0) : tr[ct][j]);
            tb[row * W + 16 * ct + l16] = t_ - acc[ct][j];
          }
        }
      }
    }
    // (a wide band: requested behind phase 1, before the barrier -- there the registers buy more than the latency)
    // (unconditional where the instance decides it: a wave without a strip reads strip 0's first set, never multiplied --
    // a set that is requested under a branch holds its registers through all of phase 1)
    if (NCT != 1 || ((dbg & 256) && wave < S)) {
      const double *ap_ = Ac + ((int64_t)max(S - 1 - wave, 0) * lda) * 16 + l16 + (int64_t)kq * 16;
#pragma unroll
      for (int u = 0; u < KU; ++u) a0[u] = ap_[u * 64];
    }
    // ---- phase 2 (its requests start here): x = Tinv * t on the matrix cores, one 16-row strip x this slice's columns at
    // a time; strips are dealt heaviest first in snake order over the four waves (k_band_cs): this wave's strips are
    // S - 1 - q, q = 4 rnd + (rnd odd ? 3 - wave : wave) while q < S.  The product of a strip runs over its 32-k operand
    // sets, k ascending; the sets of ALL the wave's strips form ONE sequence of items, walked by two cursors: the
    // requests run two items ahead of the products, across strip boundaries (each set of the inverse is read once per
    // solve, from HBM: a round trip that nothing hid cost more than the set's eight matrix instructions).  Three register
    // sets rotate by name; every request is unconditional -- past the last item the cursor stays and reads that item
    // again, never multiplied -- so the wait in front of a set's products is COUNTED: it leaves the two younger sets
    // in flight (a load under a branch makes the compiler wait for everything at the merge)
    const int Sx = (dbg & 2) ? 0 : S;
    int nitems = 0;
    for (int r = 0;; ++r) {
      const int q = 4 * r + ((r & 1) ? 3 - wave : wave);
      if (q >= Sx) break;
      nitems += (min(nb, 16 * (S - q)) + 31) >> 5;
    }
    // a cursor: item index, round, set within the strip, sets of the strip, strip
#define HIFAMD_CT_NEXT(i_, rnd_, t_, ns_, strip_)                         \
  if (i_ + 1 < nitems) {                                                  \
    ++i_;                                                                 \
    if (t_ + 1 < ns_) {                                                   \
      ++t_;                                                               \
    } else {                                                              \
      ++rnd_;                                                             \
      t_ = 0;                                                             \
      strip_ = S - 1 - (4 * rnd_ + ((rnd_ & 1) ? 3 - wave : wave));       \
      ns_ = (min(nb, 16 * (strip_ + 1)) + 31) >> 5;                       \
    }                                                                     \
  }
#define HIFAMD_CT_LOAD(aa)                                                                       \
  {                                                                                              \
    const double *ap_ = Ac + ((int64_t)l_strip * lda) * 16 + l16 + (int64_t)(32 * l_t + kq) * 16; \
    _Pragma("unroll") for (int u = 0; u < KU; ++u) aa[u] = ap_[u * 64];                          \
    HIFAMD_CT_NEXT(l_i, l_rnd, l_t, l_ns, l_strip)                                               \
  }
    int l_i = 0, l_rnd = 0, l_t = 0, l_strip = max(S - 1 - wave, 0), l_ns = (min(nb, 16 * (S - wave)) + 31) >> 5;
    double a2[KU];
    // (item 0 is on its way; item 1 follows it before the barrier -- unconditionally: a wave without items reads strip
    // 0's first set)
    HIFAMD_CT_NEXT(l_i, l_rnd, l_t, l_ns, l_strip)
    HIFAMD_CT_LOAD(a1)
    // (rows nb .. lda - 1 are zero for the inverse product; lds_rows is a multiple of 32)
    for (int t = nb * W + (int)threadIdx.x; t < lda * W; t += 256) tb[t] = 0.0;
    HIFAMD_CSP(4)
    __syncthreads();
    HIFAMD_CSP(5)
    if (nitems > 0) {
      int m_i = 0, m_rnd = 0, m_t = 0, m_strip = S - 1 - wave, m_ns = (min(nb, 16 * (S - wave)) + 31) >> 5;
      const double *Bp = tb + l16;
      v4f64 acc0[NCT];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc0[ct] = v4f64{0.0, 0.0, 0.0, 0.0};
      // the products of the item under the product cursor; behind a strip's last set its rows go out
#define HIFAMD_CT_MFMA(aa)                                                                  \
  {                                                                                         \
    const int kb_ = 32 * m_t + kq;                                                          \
    _Pragma("unroll") for (int u = 0; u < KU; ++u) {                                        \
      _Pragma("unroll") for (int ct = 0; ct < NCT; ++ct) {                                  \
        const double b0_ = Bp[(kb_ + 4 * u) * W + 16 * ct];                                 \
        acc0[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[u], b0_, acc0[ct], 0, 0, 0);     \
      }                                                                                     \
    }                                                                                       \
    if (m_t + 1 == m_ns) {                                                                  \
      _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                       \
        const int row = 16 * m_strip + kq + 4 * r;                                          \
        if (row < nb) {                                                                     \
          _Pragma("unroll") for (int ct = 0; ct < NCT; ++ct) {                              \
            const int cx = cc + 16 * ct;                                                    \
            if (last_u) {                                                                   \
              if (cx < lu.nrhs) yout[(int64_t)s_oi[row] * lu.ldy + cx] = s_ot[row] * acc0[ct][r]; \
            } else {                                                                        \
              x[((int64_t)s_rowid[row] << 6) + cx] = acc0[ct][r];                           \
            }                                                                               \
          }                                                                                 \
        }                                                                                   \
      }                                                                                     \
      _Pragma("unroll") for (int ct = 0; ct < NCT; ++ct) acc0[ct] = v4f64{0.0, 0.0, 0.0, 0.0}; \
    }                                                                                       \
    HIFAMD_CT_NEXT(m_i, m_rnd, m_t, m_ns, m_strip)                                          \
  }
#define HIFAMD_CT_STEP(acur, anew)                                                          \
  {                                                                                         \
    HIFAMD_CT_LOAD(anew)                                                                    \
    __builtin_amdgcn_sched_barrier(0); /* (the requests stay in front of the products) */   \
    HIFAMD_CT_MFMA(acur)                                                                    \
  }
      int i = 0;
      for (; i + 3 <= nitems; i += 3) {  // (one exit, at the top: no break between a request and its use)
        HIFAMD_CT_STEP(a0, a2)
        HIFAMD_CT_STEP(a1, a0)
        HIFAMD_CT_STEP(a2, a1)
      }
      if (i < nitems) {  // the last one or two items: both are in registers or on their way
        HIFAMD_CT_MFMA(a0)
        if (i + 1 < nitems) HIFAMD_CT_MFMA(a1)
      }
#undef HIFAMD_CT_STEP
#undef HIFAMD_CT_MFMA
    }
#undef HIFAMD_CT_LOAD
#undef HIFAMD_CT_NEXT
    __syncthreads();  // (the next component overwrites the LDS block)
  }
  HIFAMD_CSP(6)
  HIFAMD_CSP_FLUSH(1 + (LOWER ? 0 : 4) + 32, n_band, nsl)
}

// ---------------------------------------------------------------------------------------------
// Column-sliced component band for COMPLEX data (round 3): k_band_cd_z for ONE slice of 16 complex columns per
// workgroup (blockIdx.x = component-workgroup * nsl + slice), the complex twin of k_band_cs.  A batch of at most 48
// columns launches only the slices it has: BASELINE config 5 (nrhs = 16) moves a quarter of the vector bytes and
// issues a quarter of the gathers of the 64-column kernel.  4 waves; lane group q = 4 wave + g (16 lanes = 16 complex
// columns) takes chunk q of the descriptor: its rows' right-hand sides go into two real LDS planes [rows][16], its
// entries are fetched 16 at a time per lane group and broadcast with DPP row_newbcast, four 256-byte gathers per lane
// group in flight; the inverse product is four real MFMA streams per 16-row strip (x_re = P_re t_re - P_im t_im,
// x_im = P_re t_im + P_im t_re), strips dealt heaviest first in snake order.  Per row and column the arithmetic and
// its order are k_band_cd_z's: the same bits.  No carried prefixes, no sparse-own variant (complex plans have neither).
// ---------------------------------------------------------------------------------------------
// SPARSE (round 4): sparse-own components of a complex triangle (level 0 of a PDE hierarchy: ~2 nonzeros per row) -- the
// component's own nonzeros (two real LDS arrays), row offsets and depth levels are staged in LDS and the component is
// solved level by level, a lane group per row, exactly as k_band_cs<*, true> does it for real data; no inverse exists.
template <bool LOWER, bool SPARSE>
__global__ void __launch_bounds__(256) k_band_cs_z(int32_t wg0, const int32_t *__restrict__ wg_grp_ptr,
                                                   const int32_t *__restrict__ cd_desc, const int32_t *__restrict__ rowid,
                                                   const cplx *__restrict__ d, cplx *w, cplx *v,
                                                   const double *__restrict__ tinv, const int32_t *__restrict__ mid_col,
                                                   const cplx *__restrict__ mid_val, const uint8_t *__restrict__ mid_lrow,
                                                   int first_u, int32_t nsl, int32_t lds_rows, FirstL<cplx> fl,
                                                   int32_t own_cap, const cplx *__restrict__ own_val,
                                                   const uint8_t *__restrict__ own_lsrc, const uint16_t *__restrict__ own_rptr,
                                                   const uint8_t *__restrict__ own_lvl, LastU<cplx> lu) {
  // (LDS: BandCszLds in band_lds.hpp states this layout for the host; the pointers keep their own derivation here -- the
  // code the compiler makes of this kernel moved with every other way to write it -- and tests/cpp/band_lds_test.cpp holds
  // the two together.  lds_rows is even: the host rounds up)
  extern __shared__ double cs_buf[];
  double *t_re = cs_buf, *t_im = cs_buf + (size_t)lds_rows * 16;
  double *s_hdx = t_im + (size_t)lds_rows * 16, *s_hdy = s_hdx + lds_rows;
  int32_t *s_rowid = reinterpret_cast<int32_t *>(s_hdy + lds_rows);
  int32_t *s_hp = s_rowid + lds_rows;
  // SPARSE: own nonzeros (re, im), their local sources, row offsets, depth levels
  double *ow_re = reinterpret_cast<double *>(s_hp + ((lds_rows + 1) & ~1));
  double *ow_im = ow_re + (SPARSE ? own_cap : 0);
  uint16_t *ow_rptr = reinterpret_cast<uint16_t *>(ow_im + (SPARSE ? own_cap : 0));
  uint8_t *ow_src = reinterpret_cast<uint8_t *>(ow_rptr + 260);
  uint8_t *ow_lvl = ow_src + (SPARSE ? own_cap : 0);
  // fused S7 (LastU, round 4 for complex data): output row and scale of every row, behind everything else
  double *s_ot = reinterpret_cast<double *>(ow_lvl + (SPARSE ? 264 : 0) + 8);
  s_ot = reinterpret_cast<double *>((reinterpret_cast<uintptr_t>(s_ot) + 7) & ~(uintptr_t)7);
  int32_t *s_oi = reinterpret_cast<int32_t *>(s_ot + lds_rows);
  const bool last_u = !LOWER && lu.on();
  cplx *yout = last_u ? lu.out.get() : nullptr;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int32_t bw = (int32_t)blockIdx.x / nsl, slice = (int32_t)blockIdx.x - bw * nsl;
  const int grp = lane >> 4, l16 = lane & 15, gq = wave * 4 + grp;
  const int cc = slice * 16 + l16;
  cplx *x = LOWER ? w : v;
  const bool div_u = !LOWER && first_u;
  const bool first_l = LOWER && first_u && fl.on();
  const cplx *rhs = div_u ? (const cplx *)w : (first_l ? fl.bin.get() : (const cplx *)x);
  const int64_t rstride = first_l ? fl.ldb : 64;
  const int rcol = first_l ? min(cc, fl.nrhs - 1) : cc;
  const int32_t c_first = wg_grp_ptr[wg0 + bw], c_last = wg_grp_ptr[wg0 + bw + 1];
  const int kq = grp;
  for (int32_t c = c_first; c < c_last; ++c) {
    const int32_t *dsc = cd_desc + (int64_t)c * 28;
    const int32_t s0 = dsc[0], nb = dsc[1], mid0 = dsc[2];
    const int64_t inv_off = ((int64_t)(uint32_t)dsc[5] << 32) | (uint32_t)dsc[4];
    const uint8_t *wrow = reinterpret_cast<const uint8_t *>(dsc + 6);
    const uint16_t *wmid = reinterpret_cast<const uint16_t *>(dsc + 11);
    const int r0 = wrow[gq], nr = (int)wrow[gq + 1] - r0;
    const int32_t e0 = mid0 + (int32_t)wmid[gq], ne = (int32_t)wmid[gq + 1] - (int32_t)wmid[gq];
    const int lda = (nb + 31) & ~31;
    // ---- phase 0: row ids and per-row scalars
    for (int32_t t = (int32_t)threadIdx.x; t < nb; t += 256) {
      const int32_t i = rowid[s0 + t];
      s_rowid[t] = i;
      if (div_u) {
        const cplx dd = d[i];
        s_hdx[t] = dd.x, s_hdy[t] = dd.y;
      }
      if (first_l) {
        const int32_t pp = fl.p[i];
        s_hp[t] = pp;
        s_hdx[t] = fl.s[pp];
      }
      if (last_u) {
        const int32_t oi = lu.q[i];
        s_oi[t] = oi;
        s_ot[t] = lu.t[oi];
      }
    }
    if (SPARSE) {
      const int32_t own0 = dsc[20], nown = dsc[21], orp0 = dsc[22], lvl0 = dsc[23], nlvl = dsc[24];
      for (int32_t t = (int32_t)threadIdx.x; t < nown; t += 256) {
        const cplx ov = own_val[own0 + t];
        ow_re[t] = ov.x, ow_im[t] = ov.y;
        ow_src[t] = own_lsrc[own0 + t];
      }
      for (int32_t t = (int32_t)threadIdx.x; t <= nb; t += 256) ow_rptr[t] = own_rptr[orp0 + t];
      for (int32_t t = (int32_t)threadIdx.x; t <= nlvl; t += 256) ow_lvl[t] = own_lvl[lvl0 + t];
    }
    int32_t colv = 0, lrv = 0;
    cplx valv = cplx{0.0, 0.0};
    if (l16 < ne) {
      colv = mid_col[e0 + l16];
      valv = mid_val[e0 + l16];
      lrv = mid_lrow[e0 + l16];
    }
    __syncthreads();
    // ---- phase 1a: right-hand sides of this lane group's rows into the two LDS planes, four rows in flight
    const int nrmax = wave_max4(nr);
    for (int j = 0; j < nrmax; j += 4) {
      cplx t_[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = r0 + min(j + q, max(nr - 1, 0));
        const int32_t i = first_l ? s_hp[r] : s_rowid[r];
        t_[q] = (j + q < nr) ? rhs[(int64_t)i * rstride + rcol] : cplx{0.0, 0.0};
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (j + q < nr) {
          const int r = r0 + j + q;
          cplx val = t_[q];
          if (div_u)
            val = vdiv(val, cplx{s_hdx[r], s_hdy[r]});
          else if (first_l)
            val = cc < fl.nrhs ? vscale(s_hdx[r], val) : cplx{0.0, 0.0};
          t_re[(r << 4) + l16] = val.x;
          t_im[(r << 4) + l16] = val.y;
        }
    }
    // ---- phase 1b: this lane group's entries, items of 16, four gathers per batch
    int cur = -1;
    cplx acc = cplx{0.0, 0.0};
    const int32_t nemax = wave_max4(ne);
    for (int32_t base = 0; base < nemax; base += 16) {
      int32_t colv2 = 0, lrv2 = 0;
      cplx valv2 = cplx{0.0, 0.0};
      if (base + 16 + l16 < ne) {
        colv2 = mid_col[e0 + base + 16 + l16];
        valv2 = mid_val[e0 + base + 16 + l16];
        lrv2 = mid_lrow[e0 + base + 16 + l16];
      }
      const int32_t left = ne - base;
      static_for<0, 4>([&](auto ib) {
        constexpr int T0 = 4 * decltype(ib)::value;
        if (T0 < nemax - base) {
          int32_t j_[4], r_[4];
          cplx a_[4], xv_[4];
          static_for<0, 4>([&](auto iu) {
            constexpr int u = decltype(iu)::value;
            j_[u] = bc16<T0 + u>(colv);
            a_[u] = cplx{bc16<T0 + u>(valv.x), bc16<T0 + u>(valv.y)};
            r_[u] = bc16<T0 + u>(lrv);
          });
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (T0 + u < left) xv_[u] = x[((int64_t)j_[u] << 6) + cc];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (T0 + u < left) {
              if (r_[u] != cur) {
                if (cur >= 0) {
                  t_re[(cur << 4) + l16] = acc.x;
                  t_im[(cur << 4) + l16] = acc.y;
                }
                cur = r_[u];
                acc = cplx{t_re[(cur << 4) + l16], t_im[(cur << 4) + l16]};
              }
              acc = vsub(acc, vmul(a_[u], xv_[u]));
            }
        }
      });
      colv = colv2;
      valv = valv2;
      lrv = lrv2;
    }
    if (cur >= 0) {
      t_re[(cur << 4) + l16] = acc.x;
      t_im[(cur << 4) + l16] = acc.y;
    }
    if (SPARSE) {
      __syncthreads();
      // ---- phase 2, sparse: substitution inside LDS, depth level by depth level; a lane group takes a row at a time
      const int nlvl = dsc[24];
      for (int lv = 0; lv < nlvl; ++lv) {
        const int r_lo = ow_lvl[lv], r_hi = ow_lvl[lv + 1];
        for (int r = r_lo + gq; r < r_hi; r += 16) {
          cplx a2 = cplx{t_re[(r << 4) + l16], t_im[(r << 4) + l16]};
          const int eb = ow_rptr[r], ee = ow_rptr[r + 1];
          for (int e = eb; e < ee; ++e) {
            const int sr = (int)ow_src[e];
            a2 = vsub(a2, vmul(cplx{ow_re[e], ow_im[e]}, cplx{t_re[(sr << 4) + l16], t_im[(sr << 4) + l16]}));
          }
          if (ee > eb) t_re[(r << 4) + l16] = a2.x, t_im[(r << 4) + l16] = a2.y;
          if (last_u) {
            if (cc < lu.nrhs) yout[(int64_t)s_oi[r] * lu.ldy + cc] = vscale(s_ot[r], a2);
          } else {
            x[((int64_t)s_rowid[r] << 6) + cc] = a2;
          }
        }
        __syncthreads();
      }
      continue;
    }
    // (rows nb .. lda - 1 are zero for the inverse product; lds_rows is a multiple of 32)
    for (int t = nb * 16 + (int)threadIdx.x; t < lda * 16; t += 256) t_re[t] = 0.0, t_im[t] = 0.0;
    __syncthreads();
    // ---- phase 2: x = Tinv * t on the real matrix cores, four products per strip
    const int S = (nb + 15) >> 4;
    const double *Are = tinv + inv_off, *Aim = Are + ((int64_t)((nb + 15) & ~15) * lda);  // plane_elems(nb, lda)
    for (int rnd = 0; 4 * rnd < S; ++rnd) {
      const int q = 4 * rnd + ((rnd & 1) ? 3 - wave : wave);
      if (q >= S) continue;
      const int strip = S - 1 - q;
      const int kend = min(nb, 16 * (strip + 1));
      const int nk = (kend + 3) >> 2;  // k-steps of four columns
      const double *Apr = Are + ((int64_t)strip * lda) * 16 + l16 + (int64_t)kq * 16;
      const double *Api = Aim + ((int64_t)strip * lda) * 16 + l16 + (int64_t)kq * 16;
      const double *Bre = t_re + l16, *Bim = t_im + l16;
      v4f64 a_rr = v4f64{0.0, 0.0, 0.0, 0.0}, a_ii = a_rr, a_ri = a_rr, a_ir = a_rr;
      constexpr int KU = 4;
      double pr0[KU], pi0[KU], pr1[KU], pi1[KU];
#define HIFAMD_CSZ_LOAD(pr, pi, t_)                                                       \
  _Pragma("unroll") for (int u = 0; u < KU; ++u) {                                        \
    pr[u] = Apr[(int64_t)(KU * (t_) + u) * 64];                                           \
    pi[u] = Api[(int64_t)(KU * (t_) + u) * 64];                                           \
  }
#define HIFAMD_CSZ_MFMA(pr, pi, t_)                                                       \
  _Pragma("unroll") for (int u = 0; u < KU; ++u) {                                        \
    const int kb_ = 4 * (KU * (t_) + u) + kq;                                             \
    const double br_ = Bre[kb_ << 4], bi_ = Bim[kb_ << 4];                                \
    a_rr = __builtin_amdgcn_mfma_f64_16x16x4f64(pr[u], br_, a_rr, 0, 0, 0);               \
    a_ii = __builtin_amdgcn_mfma_f64_16x16x4f64(pi[u], bi_, a_ii, 0, 0, 0);               \
    a_ri = __builtin_amdgcn_mfma_f64_16x16x4f64(pr[u], bi_, a_ri, 0, 0, 0);               \
    a_ir = __builtin_amdgcn_mfma_f64_16x16x4f64(pi[u], br_, a_ir, 0, 0, 0);               \
  }
      // (sets of KU = 4 k-steps = 16 columns: the operand planes and the LDS rows are zero padded up to lda, a multiple
      //  of 32, so a set never leaves the strip; k-steps past nk add exact zeros)
      const int nsets = (nk + KU - 1) / KU;
      int t = 0;
      HIFAMD_CSZ_LOAD(pr0, pi0, 0)
      while (t < nsets) {
        if (t + 1 < nsets) HIFAMD_CSZ_LOAD(pr1, pi1, t + 1)
        HIFAMD_CSZ_MFMA(pr0, pi0, t)
        if (t + 1 >= nsets) break;
        if (t + 2 < nsets) HIFAMD_CSZ_LOAD(pr0, pi0, t + 2)
        HIFAMD_CSZ_MFMA(pr1, pi1, t + 1)
        t += 2;
      }
#undef HIFAMD_CSZ_LOAD
#undef HIFAMD_CSZ_MFMA
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * strip + kq + 4 * r;
        if (row < nb) {
          const cplx res = cplx{a_rr[r] - a_ii[r], a_ri[r] + a_ir[r]};
          if (last_u) {
            if (cc < lu.nrhs) yout[(int64_t)s_oi[row] * lu.ldy + cc] = vscale(s_ot[row], res);
          } else {
            x[((int64_t)s_rowid[row] << 6) + cc] = res;
          }
        }
      }
    }
    __syncthreads();  // (the next component overwrites the LDS planes)
  }
}

// ---------------------------------------------------------------------------------------------
// Component band on coefficient tiles for COMPLEX data (round 4): k_band_ct's phase 1 (a wave owns whole strips; per tile
// the four source rows are gathered once -- 16 bytes (re, im) per lane -- and multiplied with the tile's two real
// coefficient planes by four real matrix instructions, rr / ii / ri / ir) in front of k_band_cs_z's phase 2 (the
// component's explicit inverse as two real planes).  One workgroup per (component, slice of 16 complex columns) at every
// batch width; column-separable: a column's bits do not depend on the batch it travels in.  LastU (fused S7) as in
// k_band_cs_z.
// ---------------------------------------------------------------------------------------------
template <bool LOWER>
__global__ void __launch_bounds__(256) k_band_ct_z(int32_t wg0, const int32_t *__restrict__ wg_grp_ptr,
                                                   const int32_t *__restrict__ ct_desc, const int32_t *__restrict__ rowid,
                                                   const cplx *__restrict__ d, cplx *w, cplx *v,
                                                   const double *__restrict__ tinv, const int32_t *__restrict__ ct_sptr,
                                                   const int32_t *__restrict__ ct_src, const double *__restrict__ ct_coef,
                                                   int first_u, int32_t nsl, int32_t lds_rows, int dbg, FirstL<cplx> fl,
                                                   LastU<cplx> lu) {
  extern __shared__ double cs_buf[];
  const BandCtzLds lay(lds_rows);
  double *t_re = cs_buf, *t_im = lds_next<double>(t_re, lay.t_re, lay.t_im);
  double *s_hdx = lds_next<double>(t_im, lay.t_im, lay.hdx), *s_hdy = lds_next<double>(s_hdx, lay.hdx, lay.hdy);
  double *s_ot = lds_next<double>(s_hdy, lay.hdy, lay.ot);
  int32_t *s_rowid = lds_next<int32_t>(s_ot, lay.ot, lay.rowid);
  int32_t *s_hp = lds_next<int32_t>(s_rowid, lay.rowid, lay.hp);
  int32_t *s_oi = lds_next<int32_t>(s_hp, lay.hp, lay.oi);
  int32_t *s_sptr = lds_next<int32_t>(s_oi, lay.oi, lay.sptr);  // 17 entries
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int32_t bw = (int32_t)blockIdx.x / nsl, slice = (int32_t)blockIdx.x - bw * nsl;
  const int kq = lane >> 4, l16 = lane & 15;
  const int cc = slice * 16 + l16;
  cplx *x = LOWER ? w : v;
  const BandRhs<cplx> br = band_rhs<LOWER>(first_u, fl, w, x);
  const bool div_u = br.div_u, first_l = br.first_l;
  const cplx *rhs = br.rhs;
  const int64_t rstride = br.rstride;
  const bool last_u = !LOWER && lu.on();
  cplx *yout = last_u ? lu.out.get() : nullptr;
  const int rcol = br.col(cc, fl);
  const int32_t c_first = wg_grp_ptr[wg0 + bw], c_last = wg_grp_ptr[wg0 + bw + 1];
  for (int32_t c = c_first; c < c_last; ++c) {
    const int32_t *dsc = ct_desc + (int64_t)c * 28;
    const int32_t s0 = dsc[0], nb = dsc[1], sp0 = dsc[20];
    const int64_t inv_off = ((int64_t)(uint32_t)dsc[5] << 32) | (uint32_t)dsc[4];
    const uint32_t mword = (uint32_t)dsc[22 + (wave >> 1)];
    const uint32_t mymask = (wave & 1) ? (mword >> 16) : (mword & 0xffffu);  // the strips this wave owns
    const int lda = (nb + 31) & ~31;
    const int S = (nb + 15) >> 4;
    // ---- phase 0: row ids, per-row scalars, strip offsets
    for (int32_t t = (int32_t)threadIdx.x; t < nb; t += 256) {
      const int32_t i = rowid[s0 + t];
      s_rowid[t] = i;
      if (div_u) {
        const cplx dd = d[i];
        s_hdx[t] = dd.x, s_hdy[t] = dd.y;
      }
      if (first_l) {
        const int32_t pp = fl.p[i];
        s_hp[t] = pp;
        s_hdx[t] = fl.s[pp];
      }
      if (last_u) {
        const int32_t oi = lu.q[i];
        s_oi[t] = oi;
        s_ot[t] = lu.t[oi];
      }
    }
    if ((int32_t)threadIdx.x <= S) s_sptr[threadIdx.x] = ct_sptr[sp0 + (int32_t)threadIdx.x];
    __syncthreads();
    // ---- phase 1: this wave's strips -- right-hand sides requested first, then the strip's tiles four at a time
    constexpr int BU = 4;
    for (int s = 0; s < S; ++s) {
      if (!((mymask >> s) & 1u)) continue;  // (wave-uniform)
      cplx tr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = min(16 * s + kq + 4 * j, nb - 1);
        const int32_t i = first_l ? s_hp[row] : s_rowid[row];
        tr[j] = rhs[(int64_t)i * rstride + rcol];
      }
      const int32_t t0 = s_sptr[s], t1 = (dbg & 1) ? t0 : s_sptr[s + 1];
      v4f64 a_rr = v4f64{0.0, 0.0, 0.0, 0.0}, a_ii = a_rr, a_ri = a_rr, a_ir = a_rr;
      if (t0 < t1) {
        int32_t sv[BU];
        double cr[BU], ci[BU];
#pragma unroll
        for (int u = 0; u < BU; ++u) {
          const int32_t tt = min(t0 + u, t1 - 1);
          sv[u] = ct_src[4 * (int64_t)tt + kq];
          cr[u] = ct_coef[128 * (int64_t)tt + lane];
          ci[u] = ct_coef[128 * (int64_t)tt + 64 + lane];
          if (t0 + u >= t1) cr[u] = 0.0, ci[u] = 0.0;
        }
        for (int32_t t = t0; t < t1; t += BU) {
          cplx bv[BU];
#pragma unroll
          for (int u = 0; u < BU; ++u) bv[u] = x[((int64_t)sv[u] << 6) + cc];
          int32_t sn[BU];
          double crn[BU], cin[BU];
#pragma unroll
          for (int u = 0; u < BU; ++u) {  // (clamped: the loads past the strip's last tile read that tile again, weight zero)
            const int32_t tt = min(t + BU + u, t1 - 1);
            sn[u] = ct_src[4 * (int64_t)tt + kq];
            crn[u] = ct_coef[128 * (int64_t)tt + lane];
            cin[u] = ct_coef[128 * (int64_t)tt + 64 + lane];
            if (t + BU + u >= t1) crn[u] = 0.0, cin[u] = 0.0;
          }
#pragma unroll
          for (int u = 0; u < BU; ++u) {
            a_rr = __builtin_amdgcn_mfma_f64_16x16x4f64(cr[u], bv[u].x, a_rr, 0, 0, 0);
            a_ii = __builtin_amdgcn_mfma_f64_16x16x4f64(ci[u], bv[u].y, a_ii, 0, 0, 0);
            a_ri = __builtin_amdgcn_mfma_f64_16x16x4f64(cr[u], bv[u].y, a_ri, 0, 0, 0);
            a_ir = __builtin_amdgcn_mfma_f64_16x16x4f64(ci[u], bv[u].x, a_ir, 0, 0, 0);
          }
#pragma unroll
          for (int u = 0; u < BU; ++u) sv[u] = sn[u], cr[u] = crn[u], ci[u] = cin[u];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = 16 * s + kq + 4 * j;
        if (row < nb) {
          cplx val = tr[j];
          if (div_u)
            val = vdiv(val, cplx{s_hdx[row], s_hdy[row]});
          else if (first_l)
            val = cc < fl.nrhs ? vscale(s_hdx[row], val) : cplx{0.0, 0.0};
          t_re[(row << 4) + l16] = val.x - (a_rr[j] - a_ii[j]);
          t_im[(row << 4) + l16] = val.y - (a_ri[j] + a_ir[j]);
        }
      }
    }
    // (rows nb .. lda - 1 are zero for the inverse product; lds_rows is a multiple of 32)
    for (int t = nb * 16 + (int)threadIdx.x; t < lda * 16; t += 256) t_re[t] = 0.0, t_im[t] = 0.0;
    __syncthreads();
    // ---- phase 2: x = Tinv * t on the real matrix cores, four products per strip (k_band_cs_z)
    const double *Are = tinv + inv_off, *Aim = Are + ((int64_t)((nb + 15) & ~15) * lda);  // plane_elems(nb, lda)
    for (int rnd = 0; 4 * rnd < S; ++rnd) {
      const int q = 4 * rnd + ((rnd & 1) ? 3 - wave : wave);
      if (q >= S) continue;
      const int strip = S - 1 - q;
      const int kend = min(nb, 16 * (strip + 1));
      const int nk = (kend + 3) >> 2;  // k-steps of four columns
      const double *Apr = Are + ((int64_t)strip * lda) * 16 + l16 + (int64_t)kq * 16;
      const double *Api = Aim + ((int64_t)strip * lda) * 16 + l16 + (int64_t)kq * 16;
      const double *Bre = t_re + l16, *Bim = t_im + l16;
      v4f64 a_rr = v4f64{0.0, 0.0, 0.0, 0.0}, a_ii = a_rr, a_ri = a_rr, a_ir = a_rr;
      constexpr int KU = 4;
      double pr0[KU], pi0[KU], pr1[KU], pi1[KU];
#define HIFAMD_CTZ_LOAD(pr, pi, t_)                                                       \
  _Pragma("unroll") for (int u = 0; u < KU; ++u) {                                        \
    pr[u] = Apr[(int64_t)(KU * (t_) + u) * 64];                                           \
    pi[u] = Api[(int64_t)(KU * (t_) + u) * 64];                                           \
  }
#define HIFAMD_CTZ_MFMA(pr, pi, t_)                                                       \
  _Pragma("unroll") for (int u = 0; u < KU; ++u) {                                        \
    const int kb_ = 4 * (KU * (t_) + u) + kq;                                             \
    const double br_ = Bre[kb_ << 4], bi_ = Bim[kb_ << 4];                                \
    a_rr = __builtin_amdgcn_mfma_f64_16x16x4f64(pr[u], br_, a_rr, 0, 0, 0);               \
    a_ii = __builtin_amdgcn_mfma_f64_16x16x4f64(pi[u], bi_, a_ii, 0, 0, 0);               \
    a_ri = __builtin_amdgcn_mfma_f64_16x16x4f64(pr[u], bi_, a_ri, 0, 0, 0);               \
    a_ir = __builtin_amdgcn_mfma_f64_16x16x4f64(pi[u], br_, a_ir, 0, 0, 0);               \
  }
      const int nsets = (nk + KU - 1) / KU;
      int t = 0;
      HIFAMD_CTZ_LOAD(pr0, pi0, 0)
      while (t < nsets) {
        if (t + 1 < nsets) HIFAMD_CTZ_LOAD(pr1, pi1, t + 1)
        HIFAMD_CTZ_MFMA(pr0, pi0, t)
        if (t + 1 >= nsets) break;
        if (t + 2 < nsets) HIFAMD_CTZ_LOAD(pr0, pi0, t + 2)
        HIFAMD_CTZ_MFMA(pr1, pi1, t + 1)
        t += 2;
      }
#undef HIFAMD_CTZ_LOAD
#undef HIFAMD_CTZ_MFMA
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * strip + kq + 4 * r;
        if (row < nb) {
          const cplx res = cplx{a_rr[r] - a_ii[r], a_ri[r] + a_ir[r]};
          if (last_u) {
            if (cc < lu.nrhs) yout[(int64_t)s_oi[row] * lu.ldy + cc] = vscale(s_ot[row], res);
          } else {
            x[((int64_t)s_rowid[row] << 6) + cc] = res;
          }
        }
      }
    }
    __syncthreads();  // (the next component overwrites the LDS planes)
  }
}

// ---------------------------------------------------------------------------------------------
// Component-dense band for COMPLEX data (gfx950 has no complex MFMA): the same scheme as k_band_cd<LOWER, false> --
// a dependency component per workgroup, LDS-resident, x_c = Tinv_c (rhs_c - older-source sums) -- with the component's
// right-hand sides kept as TWO real planes in LDS (re[rows][64], im[rows][64]) and the explicit inverse as two real
// planes in HBM (host.hpp build_dense_block: P_re, then P_im), so that the product is four real MFMA streams per
// output tile: x_re = P_re t_re - P_im t_im, x_im = P_re t_im + P_im t_re.  Rows are 1 KB (64 complex columns):
// cd_rows is capped at 96 for complex handles (96 KB of LDS).  No carried prefixes (complex plans do not fuse bands),
// no sparse-own variant, no staged top.  Units are (strip, 16-column tile): 4 per strip, heaviest strip first.
// ---------------------------------------------------------------------------------------------
template <bool LOWER>
__global__ void __launch_bounds__(1024) k_band_cd_z(int32_t wg0, const int32_t *__restrict__ wg_grp_ptr,
                                                    const int32_t *__restrict__ cd_desc, const int32_t *__restrict__ rowid,
                                                    const cplx *__restrict__ d, cplx *w, cplx *v,
                                                    const double *__restrict__ tinv, const int32_t *__restrict__ mid_col,
                                                    const cplx *__restrict__ mid_val, const uint8_t *__restrict__ mid_lrow,
                                                    int first_u, int32_t lds_rows, FirstL<cplx> fl) {
  // (LDS: BandCdzLds in band_lds.hpp states this layout for the host; tests/cpp/band_lds_test.cpp holds the two together)
  extern __shared__ double cd_tbuf[];  // re[lds_rows][64], im[lds_rows][64], then lds_rows row ids
  double *t_re = cd_tbuf, *t_im = cd_tbuf + (size_t)lds_rows * 64;
  int32_t *cd_rowid = reinterpret_cast<int32_t *>(cd_tbuf + (size_t)lds_rows * 128);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = blockDim.x >> 6;
  cplx *x = LOWER ? w : v;
  const bool div_u = !LOWER && first_u;
  const bool first_l = LOWER && first_u && fl.on();
  const cplx *rhs = div_u ? (const cplx *)w : (first_l ? fl.bin.get() : (const cplx *)x);
  const int64_t rstride = first_l ? fl.ldb : 64;
  const int rlane = first_l ? min(lane, fl.nrhs - 1) : lane;
  const int g = wg0 + (int)blockIdx.x;
  const int32_t c_first = wg_grp_ptr[g], c_last = wg_grp_ptr[g + 1];
  const int kq = lane >> 4;
  for (int32_t c = c_first; c < c_last; ++c) {
    const int32_t *dsc = cd_desc + (int64_t)c * 28;
    const int32_t s0 = dsc[0], nb = dsc[1], mid0 = dsc[2];
    const int64_t inv_off = ((int64_t)(uint32_t)dsc[5] << 32) | (uint32_t)dsc[4];
    const uint8_t *wrow = reinterpret_cast<const uint8_t *>(dsc + 6);
    const uint16_t *wmid = reinterpret_cast<const uint16_t *>(dsc + 11);
    const int r0 = wrow[wave], nr = (int)wrow[wave + 1] - r0;
    const int32_t e0 = mid0 + (int32_t)wmid[wave], e1 = mid0 + (int32_t)wmid[wave + 1];
    // ---- phase 1a: right-hand sides of this wave's rows into the two LDS planes
    int32_t h_i = 0, h_p = 0;
    cplx h_d = cplx{1.0, 0.0};  // (U: the pivot; fused S1: the row's real scale in .x)
    if (lane < nr) {
      h_i = rowid[s0 + r0 + lane];
      cd_rowid[r0 + lane] = h_i;
      if (div_u) h_d = d[h_i];
      if (first_l) {
        h_p = fl.p[h_i];
        h_d = cplx{fl.s[h_p], 0.0};
      }
    }
    int32_t colv = 0, lrv = 0;
    cplx valv = cplx{0.0, 0.0};
    if (e0 + lane < e1) {  // first item of the wave's entry stream
      colv = mid_col[e0 + lane];
      valv = mid_val[e0 + lane];
      lrv = mid_lrow[e0 + lane];
    }
    for (int j = 0; j < nr; j += 4) {
      cplx t_[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int32_t i = rl32(first_l ? h_p : h_i, min(j + q, 63));
        t_[q] = (j + q < nr) ? rhs[(int64_t)i * rstride + rlane] : cplx{0.0, 0.0};
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (j + q < nr) {
          const cplx hd = cplx{rl64(h_d.x, min(j + q, 63)), rl64(h_d.y, min(j + q, 63))};
          cplx val = t_[q];
          if (div_u)
            val = vdiv(val, hd);
          else if (first_l)
            val = lane < fl.nrhs ? vscale(hd.x, val) : cplx{0.0, 0.0};
          t_re[((r0 + j + q) << 6) + lane] = val.x;
          t_im[((r0 + j + q) << 6) + lane] = val.y;
        }
    }
    // ---- phase 1b: the wave's entries (sources finished by earlier launches), items of 64, four gathers per batch
    int cur_r = -1;
    cplx acc = cplx{0.0, 0.0};
    for (int32_t e = e0; e < e1; e += 64) {
      const int cnt = min(64, e1 - e);
      int32_t colv2 = 0, lrv2 = 0;
      cplx valv2 = cplx{0.0, 0.0};
      if (e + 64 + lane < e1) {
        colv2 = mid_col[e + 64 + lane];
        valv2 = mid_val[e + 64 + lane];
        lrv2 = mid_lrow[e + 64 + lane];
      }
      for (int t = 0; t < cnt; t += 4) {
        int32_t j_[4], r_[4];
        cplx a_[4], xv_[4];
#pragma unroll
        for (int b2 = 0; b2 < 4; ++b2) {
          const int idx = min(t + b2, 63);
          j_[b2] = rl32(colv, idx);
          a_[b2] = cplx{rl64(valv.x, idx), rl64(valv.y, idx)};
          r_[b2] = rl32(lrv, idx);
        }
#pragma unroll
        for (int b2 = 0; b2 < 4; ++b2)
          if (t + b2 < cnt) xv_[b2] = x[((int64_t)j_[b2] << 6) + lane];
#pragma unroll
        for (int b2 = 0; b2 < 4; ++b2)
          if (t + b2 < cnt) {
            if (r_[b2] != cur_r) {  // (wave-uniform)
              if (cur_r >= 0) {
                t_re[(cur_r << 6) + lane] = acc.x;
                t_im[(cur_r << 6) + lane] = acc.y;
              }
              cur_r = r_[b2];
              acc = cplx{t_re[(cur_r << 6) + lane], t_im[(cur_r << 6) + lane]};
            }
            acc = vsub(acc, vmul(a_[b2], xv_[b2]));
          }
      }
      colv = colv2;
      valv = valv2;
      lrv = lrv2;
    }
    if (cur_r >= 0) {
      t_re[(cur_r << 6) + lane] = acc.x;
      t_im[(cur_r << 6) + lane] = acc.y;
    }
    __syncthreads();
    // ---- phase 2: x = Tinv * t on the real matrix cores, four products per output tile
    const int lda = (nb + 31) & ~31;
    const int S = (nb + 15) >> 4, nunits = S * 4;
    const double *Are = tinv + inv_off, *Aim = Are + ((int64_t)((nb + 15) & ~15) * lda);  // plane_elems(nb, lda)
    for (int q = wave; q < nunits; q += nw) {
      const int strip = S - 1 - (q >> 2), ct = q & 3;
      const int kend = min(nb, 16 * (strip + 1));
      const int nk = (kend + 3) >> 2;  // k-steps of four columns
      const double *Apr = Are + ((int64_t)strip * lda) * 16 + (lane & 15) + (int64_t)kq * 16;
      const double *Api = Aim + ((int64_t)strip * lda) * 16 + (lane & 15) + (int64_t)kq * 16;
      const double *Bre = t_re + ct * 16 + (lane & 15), *Bim = t_im + ct * 16 + (lane & 15);
      v4f64 a_rr = v4f64{0.0, 0.0, 0.0, 0.0}, a_ii = a_rr, a_ri = a_rr, a_ir = a_rr;
      constexpr int KU = 2;
      double pr0[KU], pi0[KU], pr1[KU], pi1[KU];
#define HIFAMD_CDZ_LOAD(pr, pi, t_)                                                       \
  _Pragma("unroll") for (int u = 0; u < KU; ++u) {                                        \
    pr[u] = Apr[(int64_t)(KU * (t_) + u) * 64];                                           \
    pi[u] = Api[(int64_t)(KU * (t_) + u) * 64];                                           \
  }
#define HIFAMD_CDZ_MFMA(pr, pi, t_)                                                       \
  _Pragma("unroll") for (int u = 0; u < KU; ++u) {                                        \
    const int kb_ = 4 * (KU * (t_) + u) + kq;                                             \
    const bool ok_ = kb_ < nb;                                                            \
    const double br_ = ok_ ? Bre[kb_ << 6] : 0.0, bi_ = ok_ ? Bim[kb_ << 6] : 0.0;        \
    a_rr = __builtin_amdgcn_mfma_f64_16x16x4f64(pr[u], br_, a_rr, 0, 0, 0);               \
    a_ii = __builtin_amdgcn_mfma_f64_16x16x4f64(pi[u], bi_, a_ii, 0, 0, 0);               \
    a_ri = __builtin_amdgcn_mfma_f64_16x16x4f64(pr[u], bi_, a_ri, 0, 0, 0);               \
    a_ir = __builtin_amdgcn_mfma_f64_16x16x4f64(pi[u], br_, a_ir, 0, 0, 0);               \
  }
      // (the operand planes are zero padded in k up to lda, a multiple of 32: sets of KU k-steps never leave the strip)
      const int nsets = (nk + KU - 1) / KU;
      int t = 0;
      HIFAMD_CDZ_LOAD(pr0, pi0, 0)
      while (t < nsets) {
        if (t + 1 < nsets) HIFAMD_CDZ_LOAD(pr1, pi1, t + 1)
        HIFAMD_CDZ_MFMA(pr0, pi0, t)
        if (t + 1 >= nsets) break;
        if (t + 2 < nsets) HIFAMD_CDZ_LOAD(pr0, pi0, t + 2)
        HIFAMD_CDZ_MFMA(pr1, pi1, t + 1)
        t += 2;
      }
#undef HIFAMD_CDZ_LOAD
#undef HIFAMD_CDZ_MFMA
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * strip + kq + 4 * r;
        if (row < nb) x[((int64_t)cd_rowid[row] << 6) + ct * 16 + (lane & 15)] = cplx{a_rr[r] - a_ii[r], a_ri[r] + a_ir[r]};
      }
    }
    __syncthreads();  // (the next component overwrites the LDS planes)
  }
}

// Complex products on the real matrix cores: with X viewed as a real [rows][2R] block (re, im interleaved),
// T1 = A_re * X and T2 = A_im * X are two real MFMA products (k_dense_gemm_d / k_tri_gemm_d at logR + 1);
// this kernel recombines  out = (T1_re - T2_im) + i (T1_im + T2_re),  applies the output row permutation
// and the optional fused division (same epilogue as the real kernels).
__global__ void __launch_bounds__(256) k_zcombine(int64_t nrows, const double *__restrict__ T1,
                                                  const double *__restrict__ T2, int logR,
                                                  const int32_t *__restrict__ rowmap, cplx *__restrict__ Out,
                                                  const cplx *__restrict__ dscale, cplx *__restrict__ Out2) {
  const LaneMap lm = lane_map(logR);
  const int64_t wave = ((int64_t)xcd_block() * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave * lm.G + lm.g; i < nrows; i += nwaves * lm.G) {
    const int64_t o = (i << (logR + 1)) + 2 * lm.c;
    const cplx val{T1[o] - T2[o + 1], T1[o + 1] + T2[o]};
    const int64_t orow = rowmap ? rowmap[i] : i;
    Out[(orow << logR) + lm.c] = val;
    if (Out2) Out2[(orow << logR) + lm.c] = vdiv(val, dscale[orow]);
  }
}

// ---------------------------------------------------------------------------------------------
// Set-up (hifamd_finalize): the explicit inverses of the diagonal blocks of the block-dense and component-dense bands,
// formed ON THE DEVICE straight in operand layout -- host.hpp build_dense_block restated (forward substitution on the
// identity; the host version computes 16 columns side by side, here a lane owns a column): the same operations per
// column in the same order, the same bits (tests compare the two through hifamd_debug_checksums).  30 GB of operators
// for the 16.8 M-row hierarchy took the host threads 21 s and the PCIe link; this takes the factors that are on the
// device anyway.  Block q = rows [slot0, slot1) of the slot-ordered triangle; element (r, c) of its inverse lives at
// ((r >> 4) * ldk + c) * 16 + (r & 15) (complex: imaginary parts one plane behind); a lane reads back what it wrote
// (y_c of an earlier row c), everything above the diagonal stays the zero it was set to.  growth[q] = largest |entry|
// (NaN when a nonzero of the block is not finite: the host arithmetic would have produced NaN from inf * 0).
// grid (blocks, ceil(max rows / 256)), 256 threads.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double vabs(double a) { return fabs(a); }
__device__ __forceinline__ double vabs(cplx a) { return hypot(a.x, a.y); }
__device__ __forceinline__ bool vfinite(double a) { return isfinite(a); }
__device__ __forceinline__ bool vfinite(cplx a) { return isfinite(a.x) && isfinite(a.y); }
__device__ __forceinline__ double op_get(const double *ops, int64_t, int64_t idx, double) { return ops[idx]; }
__device__ __forceinline__ cplx op_get(const double *ops, int64_t plane, int64_t idx, cplx) { return cplx{ops[idx], ops[plane + idx]}; }
__device__ __forceinline__ void op_put(double *ops, int64_t, int64_t idx, double v) { ops[idx] = v; }
__device__ __forceinline__ void op_put(double *ops, int64_t plane, int64_t idx, cplx v) { ops[idx] = v.x, ops[plane + idx] = v.y; }
template <class T>
__global__ void __launch_bounds__(256) k_block_inverse(const int32_t *__restrict__ blk_slot0, const int32_t *__restrict__ blk_slot1,
                                                       const int64_t *__restrict__ blk_inv_off, const int32_t *__restrict__ ptr,
                                                       const int32_t *__restrict__ srcslot, const T *__restrict__ val, double *tinv,
                                                       unsigned long long *growth_bits) {
  const int q = (int)blockIdx.x;
  const int32_t r0 = blk_slot0[q], nb = blk_slot1[q] - r0;
  if ((int32_t)blockIdx.y * 256 >= nb) return;
  const int32_t j = (int32_t)blockIdx.y * 256 + (int32_t)threadIdx.x;  // this lane's column of the inverse
  const bool live = j < nb;
  if (__builtin_amdgcn_readfirstlane(j) >= nb) return;  // (a wave without a column)
  const int32_t c0 = j & ~15;  // (the host works on chunks of 16 columns: a column's sum starts at its chunk's first row)
  const int64_t ldk = ((int64_t)nb + 31) & ~(int64_t)31, plane = (((int64_t)nb + 15) / 16) * 16 * ldk;
  double *ops = tinv + blk_inv_off[q];
  double g = 1.0;
  if (live) op_put(ops, plane, (((int64_t)(j >> 4)) * ldk + j) * 16 + (j & 15), vfromreal(1.0, T()));
  const int32_t rbeg = __builtin_amdgcn_readfirstlane(c0) + 1;  // (the wave's first chunk; later chunks skip rows <= their c0)
  for (int32_t r = rbeg; r < nb; ++r) {
    const int32_t s = r0 + r;
    T acc = vfromreal(r == j ? 1.0 : 0.0, T());
    const bool mine = live && r > c0;
    for (int32_t k = ptr[s]; k < ptr[s + 1]; ++k) {
      const int32_t c = srcslot[k] - r0;
      if (c < 0) continue;  // (a source outside the block: the band kernel's business)
      const T a = val[k];
      if (!vfinite(a)) g = __builtin_nan("");
      if (mine && c >= c0) acc = vsub(acc, vmul(a, op_get(ops, plane, (((int64_t)(c >> 4)) * ldk + j) * 16 + (c & 15), T())));
    }
    if (mine && j <= r) {
      if (j < r) op_put(ops, plane, (((int64_t)(r >> 4)) * ldk + j) * 16 + (r & 15), acc);
      g = vfinite(acc) ? fmax(g, vabs(acc)) + (isnan(g) ? g : 0.0) : __builtin_nan("");
    }
  }
  // largest entry of the block: positive doubles order like their bit patterns; NaN (all ones in the exponent) wins
  if (live) atomicMax(&growth_bits[q], (unsigned long long)__double_as_longlong(isnan(g) ? __builtin_nan("") : g));
}

// ---------------------------------------------------------------------------------------------
// Device-resident breakdown-free block CG (Dubrulle's BCGrQ, preconditioned) for a Hermitian positive-definite pair
// (A, M), one tile of nc <= 64 columns in a shared block Krylov space (Engine::bcg_tile).  Vectors are [n][nc] contiguous;
// a block of rank r < nc keeps its columns >= r exactly zero.  Three kinds of kernel:
//   k_bcg_gram            partials of X^H Y, rows as the K dimension of v_mfma_f64_16x16x4_f64
//   k_bcg_xq / k_bcg_qp   the two row-local passes: a 16-row strip of [n][nc] times coefficient matrices of at most 64 x 64
//                         that every workgroup stages in LDS once
//   k_bcg_small           one workgroup: Cholesky factors, inverses and every decision (blockcg_small.hpp, shared with the host)
// Lane maps of the instruction: A: lane l holds A[i = l & 15][k = l >> 4]; B: B[k = l >> 4][j = l & 15]; C / D: col = l & 15,
// row = (l >> 4) + 4 reg.  A complex handle runs the same kernels on its real planes: four instructions per tile pair into
// a real and an imaginary accumulator.  Partials are summed in a fixed order (waves of a block in wave order, blocks in block
// order by k_bcg_sum): no atomics, and the same inputs give the same bits.  Unlike k_cg_*, a column's bits DO depend on the
// other columns of its tile: that is what a shared Krylov space means.
// ---------------------------------------------------------------------------------------------
constexpr int kBcgBlocks = 256;  // workgroups of 4 waves of every pass (one per compute unit) and partial matrices per Gram

template <class T>
using BcgState = bcg::Small<T>;  // (C, E1, E2, G, relres, deftol beside the KrylovState: blockcg_small.hpp)

template <class T>
struct BcgAcc;
template <>
struct BcgAcc<double> {
  v4f64 re;
};
template <>
struct BcgAcc<cplx> {
  v4f64 re, im;
};
__device__ __forceinline__ void bcg_clear(BcgAcc<double> &c) { c.re = v4f64{0.0, 0.0, 0.0, 0.0}; }
__device__ __forceinline__ void bcg_clear(BcgAcc<cplx> &c) { c.re = c.im = v4f64{0.0, 0.0, 0.0, 0.0}; }
// c += A B for the operand values of this lane
__device__ __forceinline__ void bcg_mma(BcgAcc<double> &c, double a, double b) {
  c.re = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c.re, 0, 0, 0);
}
__device__ __forceinline__ void bcg_mma(BcgAcc<cplx> &c, cplx a, cplx b) {
  c.re = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, c.re, 0, 0, 0);
  c.re = __builtin_amdgcn_mfma_f64_16x16x4f64(-a.y, b.y, c.re, 0, 0, 0);
  c.im = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.y, c.im, 0, 0, 0);
  c.im = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.x, c.im, 0, 0, 0);
}
__device__ __forceinline__ double bcg_get(const BcgAcc<double> &c, int reg) { return c.re[reg]; }
__device__ __forceinline__ cplx bcg_get(const BcgAcc<cplx> &c, int reg) { return cplx{c.re[reg], c.im[reg]}; }

// element (row, col) of an [n][nc] block, an exact zero outside it; the load itself is unconditional (a clamped address)
template <class T>
__device__ __forceinline__ T bcg_load(const T *__restrict__ x, int64_t n, int nc, int64_t row, int col) {
  const bool ok = row < n && col < nc;
  const T v = x[ok ? row * nc + col : 0];
  return ok ? v : vzero(T());
}

// Adds the 4 x 4 accumulator tiles of the four waves of a block in wave order and writes the nt x nt tiles in use to
// out ([64][64]).  lds: 64 x 64 values, free to use from the barrier this function starts with.
template <class T>
__device__ __forceinline__ void bcg_block_partial_at(BcgAcc<T> (&acc)[4][4], int nt, T *lds, T *__restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, kq = lane >> 4;
  for (int w = 1; w < 4; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) lds[(16 * ti + kq + 4 * reg) * 64 + 16 * tj + ci] = bcg_get(acc[ti][tj], reg);
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const T v = lds[(16 * ti + kq + 4 * reg) * 64 + 16 * tj + ci];
            if constexpr (std::is_same<T, cplx>::value)
              acc[ti][tj].re[reg] += v.x, acc[ti][tj].im[reg] += v.y;
            else
              acc[ti][tj].re[reg] += v;
          }
    }
  }
  if (wave != 0) return;
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
      if (ti < nt && tj < nt) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) out[(16 * ti + kq + 4 * reg) * 64 + 16 * tj + ci] = bcg_get(acc[ti][tj], reg);
      }
}
// (the same to partial[blockIdx.x] of a one-dimensional grid)
template <class T>
__device__ __forceinline__ void bcg_block_partial(BcgAcc<T> (&acc)[4][4], int nt, T *lds, T *__restrict__ partial) {
  bcg_block_partial_at(acc, nt, lds, partial + (int64_t)blockIdx.x * 64 * 64);
}

// partial[blockIdx.x] = the block's share of X^H Y: wave w of block b owns the row groups g = 4 b + w + k * 4 gridDim.x
// (rows 4 g .. 4 g + 3, one K step of the instruction each)
template <class T>
__global__ void __launch_bounds__(256) k_bcg_gram(int64_t n, int nc, const T *__restrict__ X, const T *__restrict__ Y,
                                                  T *__restrict__ partial /* [gridDim.x][64][64] */) {
  __shared__ T lds[64 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, kq = lane >> 4;
  const int nt = (nc + 15) >> 4;
  BcgAcc<T> acc[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) bcg_clear(acc[ti][tj]);
  const int64_t stride = (int64_t)gridDim.x * 4;
  // (two row groups per turn, all their loads issued before the first product; a group past the last row loads zeros)
  for (int64_t g = (int64_t)blockIdx.x * 4 + wave; 4 * g < n; g += 2 * stride) {
    T a[2][4], b[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        a[u][t] = vconj(bcg_load(X, n, nc, 4 * (g + u * stride) + kq, 16 * t + ci));
        b[u][t] = bcg_load(Y, n, nc, 4 * (g + u * stride) + kq, 16 * t + ci);
      }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
          if (ti < nt && tj < nt) bcg_mma(acc[ti][tj], a[u][ti], b[u][tj]);
  }
  bcg_block_partial(acc, nt, lds, partial);
}

// G[i][j] = the partials of entry (i, j), i, j < m, in block order (bcg::sum_partials; one thread per entry)
struct BcgGridTeam {
  __device__ int rank() const { return blockIdx.x * blockDim.x + threadIdx.x; }
  __device__ int size() const { return gridDim.x * blockDim.x; }
  __device__ void sync() const {}
};
template <class T>
__global__ void __launch_bounds__(256) k_bcg_sum(const T *__restrict__ partial, int nb, int m, T *__restrict__ G) {
  bcg::sum_partials(partial, nb, m, G, BcgGridTeam{});
}

// stages the two 64 x 64 coefficient matrices of a row pass in LDS (e1 | e2)
template <class T>
__device__ __forceinline__ void bcg_stage(const T *__restrict__ E1, const T *__restrict__ E2, T *e1, T *e2) {
  for (int e = threadIdx.x; e < 64 * 64; e += blockDim.x) e1[e] = E1[e], e2[e] = E2[e];
  __syncthreads();
}

// Step 3 in one pass over the rows: X += P E1 (E1 = alpha C diag(beta)), Q -= Tm E2 (E2 = alpha), and the block's share of
// H = Q^H Q of the new Q.  A wave owns the 16-row strips 4 b + w + k * 4 gridDim.x; the new Q of a strip is, register by
// register, already the operand of the Gram instruction (rows 4 reg .. 4 reg + 3 of the strip are one K step).
template <class T>
__global__ void __launch_bounds__(256) k_bcg_xq(int64_t n, int nc, T *__restrict__ X, int64_t ldx, T *__restrict__ Q,
                                                const T *__restrict__ P, const T *__restrict__ Tm,
                                                const T *__restrict__ E1, const T *__restrict__ E2,
                                                T *__restrict__ partial /* [gridDim.x][64][64] */) {
  extern __shared__ double bcg_lds_raw[];
  T *e1 = (T *)bcg_lds_raw, *e2 = e1 + 64 * 64;
  bcg_stage(E1, E2, e1, e2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, kq = lane >> 4;
  const int nt = (nc + 15) >> 4;
  BcgAcc<T> h[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) bcg_clear(h[ti][tj]);
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t st = (int64_t)blockIdx.x * 4 + wave; 16 * st < n; st += stride) {
    const int64_t r0 = 16 * st;
    BcgAcc<T> ax[4], aq[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) bcg_clear(ax[t]), bcg_clear(aq[t]);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
      if (kk < 4 * nt) {
        const T p = bcg_load(P, n, nc, r0 + ci, 4 * kk + kq), t = bcg_load(Tm, n, nc, r0 + ci, 4 * kk + kq);
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
          if (tj < nt) {
            bcg_mma(ax[tj], p, e1[(4 * kk + kq) * 64 + 16 * tj + ci]);
            bcg_mma(aq[tj], t, e2[(4 * kk + kq) * 64 + 16 * tj + ci]);
          }
      }
    T qn[4][4];
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t row = r0 + kq + 4 * reg;
        const int col = 16 * tj + ci;
        qn[tj][reg] = vzero(T());
        if (tj < nt && row < n && col < nc) {
          X[row * ldx + col] = vadd(X[row * ldx + col], bcg_get(ax[tj], reg));
          qn[tj][reg] = vsub(Q[row * nc + col], bcg_get(aq[tj], reg));
          Q[row * nc + col] = qn[tj][reg];
        }
      }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
          if (ti < nt && tj < nt) bcg_mma(h[ti][tj], vconj(qn[ti][reg]), qn[tj][reg]);
  }
  bcg_block_partial(h, nt, e1, partial);
}

// Step 6 in one pass: Q <- Q E1 and P <- W E1 + P E2 in place (E1 = I[:, piv] inv(S[:, piv]), E2 = S^H).  A wave reads its
// 16-row strip of Q, W and P once, as operands, before it writes any of it; W E1 is never stored.
template <class T>
__global__ void __launch_bounds__(256) k_bcg_qp(int64_t n, int nc, T *__restrict__ Q, const T *__restrict__ W,
                                                T *__restrict__ P, const T *__restrict__ E1, const T *__restrict__ E2) {
  extern __shared__ double bcg_lds_raw[];
  T *e1 = (T *)bcg_lds_raw, *e2 = e1 + 64 * 64;
  bcg_stage(E1, E2, e1, e2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, kq = lane >> 4;
  const int nt = (nc + 15) >> 4;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t st = (int64_t)blockIdx.x * 4 + wave; 16 * st < n; st += stride) {
    const int64_t r0 = 16 * st;
    T q[16], w[16], p[16];
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      q[kk] = w[kk] = p[kk] = vzero(T());
      if (kk < 4 * nt) {
        q[kk] = bcg_load((const T *)Q, n, nc, r0 + ci, 4 * kk + kq);
        w[kk] = bcg_load(W, n, nc, r0 + ci, 4 * kk + kq);
        p[kk] = bcg_load((const T *)P, n, nc, r0 + ci, 4 * kk + kq);
      }
    }
    BcgAcc<T> aq[4], ap[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) bcg_clear(aq[t]), bcg_clear(ap[t]);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
      if (kk < 4 * nt) {
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
          if (tj < nt) {
            const T b1 = e1[(4 * kk + kq) * 64 + 16 * tj + ci], b2 = e2[(4 * kk + kq) * 64 + 16 * tj + ci];
            bcg_mma(aq[tj], q[kk], b1);
            bcg_mma(ap[tj], w[kk], b1);
            bcg_mma(ap[tj], p[kk], b2);
          }
      }
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t row = r0 + kq + 4 * reg;
        const int col = 16 * tj + ci;
        if (tj < nt && row < n && col < nc) {
          Q[row * nc + col] = bcg_get(aq[tj], reg);
          P[row * nc + col] = bcg_get(ap[tj], reg);
        }
      }
  }
}

struct BcgTeam {
  __device__ int rank() const { return threadIdx.x; }
  __device__ int size() const { return blockDim.x; }
  __device__ void sync() const { __syncthreads(); }
};

// The start's scalars from the kCgBlocks partials of |b_j|^2 (k_cg_dot): the sums, then bcg::start_columns (beta_j, which
// columns enter the block, the flags of those that do not).  One workgroup of 1024 threads.
template <class T>
__global__ void __launch_bounds__(1024) k_bcg_beta(const T *__restrict__ partial, int nc, BcgState<T> S) {
  __shared__ T sm[16 * 64];
  const T tot = cg_sum_partials(partial, nc, sm);
  double *b2 = (double *)sm;  // (the partials have been read)
  __syncthreads();
  if (threadIdx.x < nc) b2[threadIdx.x] = vreal(tot);
  __syncthreads();
  bcg::start_columns(S, nc, b2, BcgTeam{});
}

// R[:, c] = R[:, c] / beta_c for a column of the block, an exact zero otherwise (selected, not multiplied: a NaN stays out)
template <class T>
__global__ void __launch_bounds__(256) k_bcg_norm(int64_t n, int nc, T *__restrict__ R, const double *__restrict__ beta,
                                                  const int *__restrict__ active) {
  const int64_t total = n * nc;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % nc);
    const T v = R[e];
    R[e] = active[c] ? vdivr(v, beta[c]) : vzero(T());
  }
}

// One workgroup of 256 threads on the summed Gram S.G of step k (1-based): blockcg_small.hpp's modes (the arithmetic and every
// decision; a host program replays them) on two 64 x 64 working matrices in LDS.  1: the start's G = R^H Z, 2: Sigma = P^H A P,
// 3: H = Q^H Q and the residual test, 4: G = Q^H W and the next block.  A tile that is over (ctl[0] == 0) is left alone.
template <class T>
__global__ void __launch_bounds__(256) k_bcg_small(int mode, int k, int s, BcgState<T> S) {
  extern __shared__ double bcg_lds_raw[];
  const bcg::Work<T> W = bcg::Work<T>::carve(bcg_lds_raw);
  const BcgTeam tm;
  if (mode == 1) bcg::start_factor(S, W, s, tm);
  if (mode == 2) bcg::step_alpha(S, W, s, k, tm);
  if (mode == 3) bcg::step_test(S, W, s, k, tm);
  if (mode == 4) bcg::step_next(S, W, s, k, tm);
}

// ---------------------------------------------------------------------------------------------
// Device-resident restarted block GCR for a general pair (A, M) (block GMRES(m) with right preconditioning in exact
// arithmetic), one tile of nc <= 64 columns (Engine::bgcr_tile).  The direction blocks Q_i = A P_i of a cycle are kept
// orthonormal in a stack ([slot] elements apart); the residual is kept factored, relative residual = Rh C with Rh^H Rh = I.
// On top of block CG's kernels (k_bcg_gram, k_bcg_sum, k_bcg_xq, k_bcg_beta, k_bcg_norm, the lane maps above):
//   k_bgcr_gram   C_i = Q_i^H W for every stored i < j in ONE launch (k_bgcr_sum adds the partials in block order)
//   k_bgcr_proj   W -= sum Q_i C_i, Z -= sum P_i C_i and the partials of the new W^H W in one pass over the rows
//   k_bgcr_rmul   one or two blocks times the same 64 x 64 matrix, in place
//   k_bgcr_rho / k_bgcr_small   one workgroup: every decision and the small matrices (blockgcr_small.hpp, shared with the host)
// A complex handle runs the same kernels on its real planes, as block CG does.  Sums run in a fixed order, no atomics.
// ---------------------------------------------------------------------------------------------
template <class T>
struct BgcrState : bgcr::Small<T> {  // (rho, tres, mu, live, aux beside block CG's state: blockgcr_small.hpp)
  T *Cs;  // [restart][64][64]  the coefficient matrices C_i of a step
};

__device__ __forceinline__ void bcg_put(BcgAcc<double> &c, int reg, double v) { c.re[reg] = v; }
__device__ __forceinline__ void bcg_put(BcgAcc<cplx> &c, int reg, cplx v) { c.re[reg] = v.x, c.im[reg] = v.y; }

// The coefficient matrices of a stack that k_bgcr_proj holds in LDS together: 128 KB of the 160 KB (4 real, 2 complex)
template <class T>
constexpr int kBgcrGroup = (int)(131072 / (64 * 64 * sizeof(T)));

// partial[i][blockIdx.y] = block (i = blockIdx.x, blockIdx.y)'s share of Q_i^H W, Q_i = Qs + i * slot.  The stack index
// runs fastest over the grid, so the workgroups that are resident together read the same rows of W; the row groups of a
// block are dealt as in k_bcg_gram, over gridDim.y blocks per stack entry.
template <class T>
__global__ void __launch_bounds__(256) k_bgcr_gram(int64_t n, int nc, const T *__restrict__ Qs, int64_t slot,
                                                   const T *__restrict__ W,
                                                   T *__restrict__ partial /* [gridDim.x][gridDim.y][64][64] */) {
  __shared__ T lds[64 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, kq = lane >> 4;
  const int nt = (nc + 15) >> 4;
  const T *__restrict__ X = Qs + (int64_t)blockIdx.x * slot;
  BcgAcc<T> acc[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) bcg_clear(acc[ti][tj]);
  const int64_t stride = (int64_t)gridDim.y * 4;
  for (int64_t g = (int64_t)blockIdx.y * 4 + wave; 4 * g < n; g += 2 * stride) {
    T a[2][4], b[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        a[u][t] = vconj(bcg_load(X, n, nc, 4 * (g + u * stride) + kq, 16 * t + ci));
        b[u][t] = bcg_load(W, n, nc, 4 * (g + u * stride) + kq, 16 * t + ci);
      }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
          if (ti < nt && tj < nt) bcg_mma(acc[ti][tj], a[u][ti], b[u][tj]);
  }
  bcg_block_partial_at(acc, nt, lds, partial + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * 64 * 64);
}

// Cs[i] = the nb partials of stack entry i = blockIdx.y in block order (bcg::sum_partials, as k_bcg_sum)
template <class T>
__global__ void __launch_bounds__(256) k_bgcr_sum(const T *__restrict__ partial, int nb, int m, T *__restrict__ Cs) {
  bcg::sum_partials(partial + (int64_t)blockIdx.y * nb * 64 * 64, nb, m, Cs + (int64_t)blockIdx.y * 64 * 64, BcgGridTeam{});
}

// Block classical Gram-Schmidt of step j in one pass over the rows: W -= sum_{i < j} Q_i C_i, Z -= sum_{i < j} P_i C_i (the
// C_i all from the W before any update) and the block's share of the new W^H W.  A wave owns 16-row strips of W and Z and
// keeps both in accumulator registers while the strips of Q_i and P_i stream through as A operands; the -C_i are staged in
// LDS kBgcrGroup at a time (a stack deeper than one group re-stages per round of strips, from L2).  The updated W strip is,
// register by register, the operand of the Gram instruction, as in k_bcg_xq.  j == 0: the Gram alone, nothing is written.
// The four waves of a block walk their rounds together (the barriers of the staging), a strip past the last row loads zeros.
template <class T>
__global__ void __launch_bounds__(256) k_bgcr_proj(int64_t n, int nc, int j, const T *__restrict__ Qs,
                                                   const T *__restrict__ Ps, int64_t slot, const T *__restrict__ Cs,
                                                   T *__restrict__ W, T *__restrict__ Z,
                                                   T *__restrict__ partial /* [gridDim.x][64][64] */) {
  extern __shared__ double bcg_lds_raw[];
  T *cl = (T *)bcg_lds_raw;
  constexpr int GRP = kBgcrGroup<T>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, kq = lane >> 4;
  const int nt = (nc + 15) >> 4;
  BcgAcc<T> h[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) bcg_clear(h[ti][tj]);
  int staged = -1;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t st0 = (int64_t)blockIdx.x * 4; 16 * st0 < n; st0 += stride) {
    const int64_t r0 = 16 * (st0 + wave);
    BcgAcc<T> aw[4], az[4];
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        bcg_put(aw[tj], reg, bcg_load((const T *)W, n, nc, r0 + kq + 4 * reg, 16 * tj + ci));
        bcg_put(az[tj], reg, j > 0 ? bcg_load((const T *)Z, n, nc, r0 + kq + 4 * reg, 16 * tj + ci) : vzero(T()));
      }
    for (int g0 = 0; g0 < j; g0 += GRP) {
      const int cnt = (j - g0 < GRP) ? j - g0 : GRP;
      if (staged != g0) {
        __syncthreads();  // (every wave is done with the group before)
        for (int e = threadIdx.x; e < cnt * 64 * 64; e += blockDim.x) cl[e] = vsub(vzero(T()), Cs[(int64_t)g0 * 64 * 64 + e]);
        __syncthreads();
        staged = g0;
      }
      for (int u = 0; u < cnt; ++u) {
        const T *__restrict__ Qi = Qs + (int64_t)(g0 + u) * slot, *__restrict__ Pi = Ps + (int64_t)(g0 + u) * slot;
        const T *c = cl + u * 64 * 64;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
          if (kk < 4 * nt) {
            const T q = bcg_load(Qi, n, nc, r0 + ci, 4 * kk + kq), p = bcg_load(Pi, n, nc, r0 + ci, 4 * kk + kq);
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
              if (tj < nt) {
                const T b = c[(4 * kk + kq) * 64 + 16 * tj + ci];
                bcg_mma(aw[tj], q, b);
                bcg_mma(az[tj], p, b);
              }
          }
      }
    }
    T wn[4][4];
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t row = r0 + kq + 4 * reg;
        const int col = 16 * tj + ci;
        wn[tj][reg] = vzero(T());
        if (tj < nt && row < n && col < nc) {
          wn[tj][reg] = bcg_get(aw[tj], reg);
          if (j > 0) {
            W[row * nc + col] = wn[tj][reg];
            Z[row * nc + col] = bcg_get(az[tj], reg);
          }
        }
      }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
          if (ti < nt && tj < nt) bcg_mma(h[ti][tj], vconj(wn[ti][reg]), wn[tj][reg]);
  }
  bcg_block_partial(h, nt, cl, partial);
}

// X1 <- X1 E and, where X2 is not null, X2 <- X2 E in place, E (64 x 64, zero outside its block) staged in LDS.  A wave
// reads its 16-row strip of a block once, as operands, before it writes any of it.
template <class T>
__global__ void __launch_bounds__(256) k_bgcr_rmul(int64_t n, int nc, T *X1, T *X2, const T *__restrict__ E) {
  extern __shared__ double bcg_lds_raw[];
  T *e1 = (T *)bcg_lds_raw;
  for (int e = threadIdx.x; e < 64 * 64; e += blockDim.x) e1[e] = E[e];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, kq = lane >> 4;
  const int nt = (nc + 15) >> 4;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t st = (int64_t)blockIdx.x * 4 + wave; 16 * st < n; st += stride) {
    const int64_t r0 = 16 * st;
    for (int which = 0; which < 2; ++which) {
      T *X = which ? X2 : X1;
      if (!X) continue;
      T x[16];
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) x[kk] = kk < 4 * nt ? bcg_load((const T *)X, n, nc, r0 + ci, 4 * kk + kq) : vzero(T());
      BcgAcc<T> ax[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) bcg_clear(ax[t]);
#pragma unroll
      for (int kk = 0; kk < 16; ++kk)
        if (kk < 4 * nt) {
#pragma unroll
          for (int tj = 0; tj < 4; ++tj)
            if (tj < nt) bcg_mma(ax[tj], x[kk], e1[(4 * kk + kq) * 64 + 16 * tj + ci]);
        }
#pragma unroll
      for (int tj = 0; tj < 4; ++tj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int64_t row = r0 + kq + 4 * reg;
          const int col = 16 * tj + ci;
          if (tj < nt && row < n && col < nc) X[row * nc + col] = bcg_get(ax[tj], reg);
        }
    }
  }
}

// A cycle's start from the kCgBlocks partials of |r_j|^2 of the true residual (k_cg_dot): rho, rho / beta and the three
// tests that can end the tile (bgcr::cycle_start).  One workgroup of 1024 threads.
template <class T>
__global__ void __launch_bounds__(1024) k_bgcr_rho(const T *__restrict__ partial, int nc, int cycle, int steps, BgcrState<T> S) {
  __shared__ T sm[16 * 64];
  const T tot = cg_sum_partials(partial, nc, sm);
  if (S.ctl[0] == 0) return;
  __syncthreads();
  if (threadIdx.x < nc) S.rho[threadIdx.x] = vreal(tot);
  __syncthreads();
  bgcr::cycle_start(S, nc, cycle, steps, BcgTeam{});
}

// One workgroup of 256 threads on the summed Gram S.G, with blockgcr_small.hpp's modes on two 64 x 64 working matrices in LDS:
//   mode 1: cycle start: G = Rn^H Rn -> rank r, E1 (Rh = Rn E1), C        (flag: the tile's first cycle)
//   mode 2: G = W^H W -> rank q, E1 (Q_j = W E1, P_j = Z E1)
//   mode 3: G = Q_j^H Rh = D -> E1 = D C diag(beta), E2 = D
//   mode 4: G = Rh^H Rh -> rel_j, the end of the cycle, or rank r', E1 (Rh <- Rh E1), C <- S C   (flag: the cycle's last step)
// steps: the tile's completed steps.  A tile that is over, or a cycle that has ended, is left alone.
template <class T>
__global__ void __launch_bounds__(256) k_bgcr_small(int mode, int steps, int flag, int s, BgcrState<T> S) {
  extern __shared__ double bcg_lds_raw[];
  const bcg::Work<T> W = bcg::Work<T>::carve(bcg_lds_raw);
  const BcgTeam tm;
  if (mode == 1) bgcr::cycle_factor(S, W, s, flag != 0, steps, tm);
  if (mode == 2) bgcr::step_basis(S, W, s, steps, tm);
  if (mode == 3) bgcr::step_coeff(S, W, s, tm);
  if (mode == 4) bgcr::step_test(S, W, s, steps, flag != 0, tm);
}

// ---------------------------------------------------------------------------------------------
// Device-resident LOBPCG for the smallest eigenpairs of a Hermitian pair (A, M) (Engine::lobpcg_tile): k <= 16 candidates,
// the basis S = [X W P] and its image AS = [AX AW AP] as two [n][ld] blocks (ld = s = 3 k <= 48 columns, X at column 0, W at
// k, P at 2 k), the residual R as [n][k].  The generalized problem A x = lambda B x (GEN, or NB = 3) has a third [n][ld]
// block BS = [BX BW BP] beside them and is the same kernels instantiated for three blocks: one lane map, one row ownership
// and one order of summation, so that an explicit identity B (BS a bitwise copy of S) reproduces the standard iterates bit
// for bit.  Per step:
//   k_lob_resid<GEN>   R = AX - X diag(lambda) and the partials of |r_j|^2; GEN: R = AX - BX diag(lambda), and the partials
//                      of |x_j|^2 as well
//   k_lob_lock         exact zeros in the columns of R that the test found converged (so that W = M^{-1} R is zero there)
//   k_lob_gram<GEN>    partials of GB = S^H S (GEN: S^H BS) and GA = S^H AS in one pass, upper block triangle,
//                      v_mfma_f64_16x16x4_f64
//   k_lob_update<NB>   X, P <- S [C Cp], AX, AP <- AS [C Cp] (NB = 3: and BX, BP <- BS [C Cp]) on the matrix cores, [C Cp]
//                      staged in LDS
//   k_lob_small        one workgroup: the residual test (the generalized one where LobState says so), the Rayleigh-Ritz step
//                      (lobpcg_small.hpp, shared with the host; it sees GB whichever product it is), every decision and flag
// Lane maps, complex handles on real planes, fixed-order partials (k_bcg_sum adds the blocks): as block CG above.
// ---------------------------------------------------------------------------------------------
constexpr int kLobResBlocks = 1024;  // workgroups (and partials per column) of k_lob_resid

template <class T>
struct LobState : KrylovState {
  // rtol holds tol; active: 1 for a column that the last test did not find converged; iter: the completed steps
  // ctl: [0] 1 while the tile runs, [1] rank of the basis in the last step, [2] largest Jacobi sweep count,
  //      [3] the start's verdict (lob::kStart*)
  T *GB, *GA, *CC, *X1, *X2, *X3;  // [64][64] each: the summed Grams, [C Cp] of the next row pass, scratch of the small kernel
  double *lam, *res;               // [64]  Ritz values; the scaled ||r_j|| of the last test
  double deftol, anorm, b_inf;     // b_inf: ||B||_inf of the generalized problem (KrylovState's bnorm is the [64] slot)
  int k, nev;
  bool gen;                        // the generalized problem: mode 2 of k_lob_small runs the generalized test
};

// element (row, col) of an [n][ld] block whose first s columns are in use, an exact zero outside; the load is unconditional
template <class T>
__device__ __forceinline__ T lob_load(const T *__restrict__ x, int64_t n, int ld, int s, int64_t row, int col) {
  const bool ok = row < n && col < s;
  const T v = x[ok ? row * ld + col : 0];
  return ok ? v : vzero(T());
}

// partial[0][blockIdx.x] and partial[1][blockIdx.x] ([64][64] each) = the block's share of S^H S (GEN: S^H BS) and S^H AS,
// tiles (ti <= tj) only.  Wave w of block b owns the row groups g = 4 b + w + k * 4 gridDim.x (rows 4 g .. 4 g + 3, one K
// step each), two of them in flight; the conjugated strip of S is loaded once and is the left operand of both products --
// and, where there is no BS (!GEN: BS is not read), the right operand of the first.
template <class T, bool GEN>
__global__ void __launch_bounds__(256) k_lob_gram(int64_t n, int ld, int s, const T *__restrict__ S, const T *__restrict__ BS,
                                                  const T *__restrict__ AS, T *__restrict__ partial /* [2][gridDim.x][64][64] */) {
  __shared__ T lds[12 * 4 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, kq = lane >> 4;
  const int nt = (s + 15) >> 4;
  BcgAcc<T> acc[2][6];  // tile (ti, tj), ti <= tj < 3, at index 3 ti + tj - ti (ti + 1) / 2
#pragma unroll
  for (int w = 0; w < 2; ++w)
#pragma unroll
    for (int t = 0; t < 6; ++t) bcg_clear(acc[w][t]);
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t g = (int64_t)blockIdx.x * 4 + wave; 4 * g < n; g += 2 * stride) {
    T a[2][3], b[2][3], c[2][3];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const T x = lob_load(S, n, ld, s, 4 * (g + u * stride) + kq, 16 * t + ci);
        a[u][t] = vconj(x);
        b[u][t] = x;
        if constexpr (GEN) b[u][t] = lob_load(BS, n, ld, s, 4 * (g + u * stride) + kq, 16 * t + ci);
        c[u][t] = lob_load(AS, n, ld, s, 4 * (g + u * stride) + kq, 16 * t + ci);
      }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int ti = 0; ti < 3; ++ti)
#pragma unroll
        for (int tj = ti; tj < 3; ++tj)
          if (tj < nt) {
            bcg_mma(acc[0][3 * ti + tj - ti * (ti + 1) / 2], a[u][ti], b[u][tj]);
            bcg_mma(acc[1][3 * ti + tj - ti * (ti + 1) / 2], a[u][ti], c[u][tj]);
          }
  }
  // the four waves of the block in wave order
  for (int w = 1; w < 4; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) lds[((m * 6 + t) * 4 + reg) * 64 + lane] = bcg_get(acc[m][t], reg);
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const T v = lds[((m * 6 + t) * 4 + reg) * 64 + lane];
            if constexpr (std::is_same<T, cplx>::value)
              acc[m][t].re[reg] += v.x, acc[m][t].im[reg] += v.y;
            else
              acc[m][t].re[reg] += v;
          }
    }
  }
  if (wave != 0) return;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    T *__restrict__ out = partial + ((int64_t)m * gridDim.x + blockIdx.x) * 64 * 64;
#pragma unroll
    for (int ti = 0; ti < 3; ++ti)
#pragma unroll
      for (int tj = ti; tj < 3; ++tj)
        if (tj < nt) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg)
            out[(16 * ti + kq + 4 * reg) * 64 + 16 * tj + ci] = bcg_get(acc[m][3 * ti + tj - ti * (ti + 1) / 2], reg);
        }
  }
}

// X <- S C, P <- S Cp, and the same for AS (AX, AP) and, NB = 3, for BS (BX, BP; NB = 2: BS is not touched), in place: CC
// [64][64] holds C in its columns 0 .. 15 and Cp in 16 .. 31 (rows >= s and columns >= k of either are zero), staged in LDS
// once per workgroup.  A wave owns the 16-row strips 4 b + w + j * 4 gridDim.x and reads its strip of all NB blocks
// completely, as operands, before it writes any of it.  Inside a K step the products go block by block: S, AS[, BS].
template <class T, int NB>
__global__ void __launch_bounds__(256) k_lob_update(int64_t n, int ld, int s, int k, T *__restrict__ S, T *__restrict__ AS,
                                                    T *__restrict__ BS, const T *__restrict__ CC) {
  static_assert(NB == 2 || NB == 3, "two blocks (S, AS) or three (S, AS, BS)");
  __shared__ T cc[48 * 32];
  for (int e = threadIdx.x; e < 48 * 32; e += blockDim.x) cc[e] = CC[(e >> 5) * 64 + (e & 31)];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, kq = lane >> 4;
  const int nt = (s + 15) >> 4;
  const int64_t stride = (int64_t)gridDim.x * 4;
  T *const blk[3] = {S, AS, BS};
  for (int64_t st = (int64_t)blockIdx.x * 4 + wave; 16 * st < n; st += stride) {
    const int64_t r0 = 16 * st;
    T x[NB][12];
#pragma unroll
    for (int kk = 0; kk < 12; ++kk) {
#pragma unroll
      for (int m = 0; m < NB; ++m) x[m][kk] = vzero(T());
      if (kk < 4 * nt) {
#pragma unroll
        for (int m = 0; m < NB; ++m) x[m][kk] = lob_load((const T *)blk[m], n, ld, s, r0 + ci, 4 * kk + kq);
      }
    }
    BcgAcc<T> acc[NB][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int m = 0; m < NB; ++m) bcg_clear(acc[m][t]);
#pragma unroll
    for (int kk = 0; kk < 12; ++kk)
      if (kk < 4 * nt) {
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
          const T b = cc[(4 * kk + kq) * 32 + 16 * tj + ci];
#pragma unroll
          for (int m = 0; m < NB; ++m) bcg_mma(acc[m][tj], x[m][kk], b);
        }
      }
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t row = r0 + kq + 4 * reg;
        if (row < n && ci < k) {
#pragma unroll
          for (int m = 0; m < NB; ++m) blk[m][row * ld + 2 * k * tj + ci] = bcg_get(acc[m][tj], reg);
        }
      }
  }
}

// R = AX - X diag(lambda) (GEN: AX - BX diag(lambda)) ([n][k]; X, AX and BX are the first k columns of their [n][ld] blocks;
// !GEN: BS is not read) and the block's share of |r_j|^2: thread t owns column t & 15 of the rows
// 16 b + (t >> 4) + j * 16 gridDim.x in that order, the sixteen row classes of a block are added in order:
// partial[blockIdx.x][16].  GEN: the share of |x_j|^2 as well, same rows and order: partial[blockIdx.x][32], |r_j|^2 at j
// and |x_j|^2 at 16 + j.
template <class T, bool GEN>
__global__ void __launch_bounds__(256) k_lob_resid(int64_t n, int ld, int k, const T *__restrict__ S, const T *__restrict__ AS,
                                                   const T *__restrict__ BS, const double *__restrict__ lam, T *__restrict__ R,
                                                   double *__restrict__ partial /* [gridDim.x][GEN ? 32 : 16] */) {
  constexpr int np = GEN ? 32 : 16;
  __shared__ double sm[16 * np];
  const int c = threadIdx.x & 15, sub = threadIdx.x >> 4;
  const T *__restrict__ X = GEN ? BS : S;  // what lambda multiplies
  double acc = 0.0, accx = 0.0;
  if (c < k) {
    const double l = lam[c];
    for (int64_t i = (int64_t)blockIdx.x * 16 + sub; i < n; i += (int64_t)gridDim.x * 16) {
      const T r = vsub(AS[i * ld + c], vscale(l, X[i * ld + c]));
      R[i * k + c] = r;
      acc += vabs2(r);
      if constexpr (GEN) accx += vabs2(S[i * ld + c]);
    }
  }
  sm[threadIdx.x] = acc;
  if constexpr (GEN) sm[256 + threadIdx.x] = accx;
  __syncthreads();
  if (threadIdx.x < np) {
    const int j = threadIdx.x & 15, base = threadIdx.x < 16 ? 0 : 256;
    double tot = sm[base + j];
    for (int u = 1; u < 16; ++u) tot += sm[base + 16 * u + j];
    partial[blockIdx.x * np + threadIdx.x] = tot;
  }
}

// exact zeros in the columns of R ([n][k]) that the last test found converged (active[c] == 0); nothing else is written
template <class T>
__global__ void __launch_bounds__(256) k_lob_lock(int64_t n, int k, T *__restrict__ R, const int *__restrict__ active) {
  const int64_t total = n * k;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x)
    if (!active[e % k]) R[e] = vzero(T());
}

// One workgroup of 256 threads, with lobpcg_small.hpp's arithmetic and decisions on two 64 x 64 working matrices in LDS (three
// more, of the state, in HBM).  step: the completed steps.
//   mode 0: lob::start_factor  (X0^H X0 -> CC = [E 0], or the start's refusal)
//   mode 1: lob::ritz_step at the start  (X^H A X = V Theta V^H -> CC = [V 0], lambda)
//   mode 2: lob::residual_test on the kLobResBlocks partials of |r_j|^2; S.gen: the generalized test, on those of |r_j|^2
//           and |x_j|^2
//   mode 3: lob::ritz_step  (GB, GA -> CC = [C Cp], lambda, rank; or the breakdown)
template <class T>
__global__ void __launch_bounds__(256) k_lob_small(int mode, int step, const double *__restrict__ partial, LobState<T> S) {
  extern __shared__ double bcg_lds_raw[];
  const lob::RitzScratch<T> W = lob::RitzScratch<T>::carve(bcg_lds_raw, S.X1, S.X2, S.X3);
  const lob::Small<T> Sm{S.GB, S.GA, S.CC, S.lam, S.res, S.flag, S.iter, S.active, S.ctl, S.rtol, S.deftol, S.anorm, S.maxit, S.k, S.nev, S.b_inf};
  const BcgTeam tm;
  if (mode == 2) {  // (first and apart: behind the Ritz modes the complex instantiation takes one VGPR past five waves)
    if (S.gen)
      lob::residual_test_gen(Sm, partial, kLobResBlocks, step, tm);
    else
      lob::residual_test(Sm, partial, kLobResBlocks, step, tm);
    return;
  }
  if (mode == 0) lob::start_factor(Sm, W, tm);
  if (mode == 1 || mode == 3) lob::ritz_step(Sm, W, mode == 1, step, tm);
}

// ---------------------------------------------------------------------------------------------
// The B-orthogonal projector of the locked LOBPCG sweeps (Engine::eig_project, Engine::eigs_dev): W <- W - Y C with
// C = (BY)^H W for a block Y of m <= 128 locked, B-orthonormal vectors ([n][m], row stride ldy; BY the same shape, and on the
// standard problem the same pointer) and a block W of kw <= 16 columns with any row stride (the W block of S in the driver).
//   k_eig_cgram   partials of C ([128][16] per workgroup), rows as the K dimension of v_mfma_f64_16x16x4_f64: the conjugated
//                 strip of BY is the left operand, the strip of W the right one, one accumulator per 16-column tile of BY
//   k_eig_csum    C = the partials in block order (one thread per entry, as k_bcg_sum)
//   k_eig_cproj   the row-local product [n][m] . [m][16] subtracted from W in place, C staged in LDS
// Lane maps, complex handles on real planes, partials in wave order, then block order, no atomics: as block CG above.  A
// column of W that is exactly zero gives an exactly zero column of C and keeps its bits; a column's values depend on no
// other column of W.
// ---------------------------------------------------------------------------------------------
constexpr int kEigMaxM = 128;  // widest block of locked vectors
constexpr int kEigTiles = kEigMaxM / 16;

// element (row, col) of an [n][ld] block whose first `cols` columns are in use, an exact zero outside; the load is unconditional
template <class T>
__device__ __forceinline__ T eig_load(const T *__restrict__ x, int64_t n, int64_t ld, int cols, int64_t row, int col) {
  const bool ok = row < n && col < cols;
  const T v = x[ok ? row * ld + col : 0];
  return ok ? v : vzero(T());
}

// partial[blockIdx.x] ([128][16]; rows < 16 ceil(m / 16) are written) = the block's share of (BY)^H W.  Wave w of block b
// owns the row groups g = 4 b + w + j * 4 gridDim.x (rows 4 g .. 4 g + 3, one K step each), two of them in flight; only the
// tiles that m needs are loaded and multiplied.
template <class T>
__global__ void __launch_bounds__(256) k_eig_cgram(int64_t n, int m, const T *__restrict__ BY, int64_t ldy, int kw,
                                                   const T *__restrict__ W, int64_t ldw,
                                                   T *__restrict__ partial /* [gridDim.x][128][16] */) {
  __shared__ T lds[kEigMaxM * 16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, kq = lane >> 4;
  const int nt = (m + 15) >> 4;
  BcgAcc<T> acc[kEigTiles];
#pragma unroll
  for (int t = 0; t < kEigTiles; ++t) bcg_clear(acc[t]);
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t g = (int64_t)blockIdx.x * 4 + wave; 4 * g < n; g += 2 * stride) {
    T a[2][kEigTiles], b[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t row = 4 * (g + u * stride) + kq;
      b[u] = eig_load(W, n, ldw, kw, row, ci);
#pragma unroll
      for (int t = 0; t < kEigTiles; ++t) {
        a[u][t] = vzero(T());
        if (t < nt) a[u][t] = vconj(eig_load(BY, n, ldy, m, row, 16 * t + ci));
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int t = 0; t < kEigTiles; ++t)
        if (t < nt) bcg_mma(acc[t], a[u][t], b[u]);
  }
  // the four waves of the block in wave order
  for (int w = 1; w < 4; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int t = 0; t < kEigTiles; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) lds[(16 * t + kq + 4 * reg) * 16 + ci] = bcg_get(acc[t], reg);
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int t = 0; t < kEigTiles; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const T v = lds[(16 * t + kq + 4 * reg) * 16 + ci];
          if constexpr (std::is_same<T, cplx>::value)
            acc[t].re[reg] += v.x, acc[t].im[reg] += v.y;
          else
            acc[t].re[reg] += v;
        }
    }
  }
  if (wave != 0) return;
  T *__restrict__ out = partial + (int64_t)blockIdx.x * kEigMaxM * 16;
#pragma unroll
  for (int t = 0; t < kEigTiles; ++t)
    if (t < nt) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) out[(16 * t + kq + 4 * reg) * 16 + ci] = bcg_get(acc[t], reg);
    }
}

// C[e] = partial[0][e] + partial[1][e] + ... in block order, e < 16 rows (rows = 16 ceil(m / 16)); one thread per entry
template <class T>
__global__ void __launch_bounds__(256) k_eig_csum(const T *__restrict__ partial, int nb, int rows, T *__restrict__ C /* [128][16] */) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= rows * 16) return;
  const T *p = partial + e;
  T acc = p[0];
  int b = 1;
  for (; b + 8 <= nb; b += 8) {  // (eight loads in flight; the additions keep their order)
    T v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(b + u) * kEigMaxM * 16];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = vadd(acc, v[u]);
  }
  for (; b < nb; ++b) acc = vadd(acc, p[(int64_t)b * kEigMaxM * 16]);
  C[e] = acc;
}

// W <- W - Y C in place: C ([128][16]; rows >= 16 ceil(m / 16) are not read) is staged in LDS once per workgroup.  A wave
// owns the 16-row strips 4 b + w + j * 4 gridDim.x and reads its strip of Y (as the left operand, four columns a K step) and
// of W completely before it writes.
template <class T>
__global__ void __launch_bounds__(256) k_eig_cproj(int64_t n, int m, const T *__restrict__ Y, int64_t ldy, int kw,
                                                   T *__restrict__ W, int64_t ldw, const T *__restrict__ C) {
  __shared__ T cc[kEigMaxM * 16];
  const int nt = (m + 15) >> 4;
  for (int e = threadIdx.x; e < nt * 256; e += blockDim.x) cc[e] = C[e];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ci = lane & 15, kq = lane >> 4;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t st = (int64_t)blockIdx.x * 4 + wave; 16 * st < n; st += stride) {
    const int64_t r0 = 16 * st;
    T y[4 * kEigTiles], w[4];
#pragma unroll
    for (int kk = 0; kk < 4 * kEigTiles; ++kk) {
      y[kk] = vzero(T());
      if (kk < 4 * nt) y[kk] = eig_load(Y, n, ldy, m, r0 + ci, 4 * kk + kq);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) w[reg] = eig_load((const T *)W, n, ldw, kw, r0 + kq + 4 * reg, ci);
    BcgAcc<T> acc;
    bcg_clear(acc);
#pragma unroll
    for (int kk = 0; kk < 4 * kEigTiles; ++kk)
      if (kk < 4 * nt) bcg_mma(acc, y[kk], cc[(4 * kk + kq) * 16 + ci]);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t row = r0 + kq + 4 * reg;
      if (row < n && ci < kw) W[row * ldw + ci] = vsub(w[reg], bcg_get(acc, reg));
    }
  }
}

}  // namespace hifamd
