// engine.hip -- device residency of the hierarchy, the per-level kernel sequence of one apply
// (captured once per batch shape into a hipGraph), batched iterative refinement, and the C ABI
// of include/hifir_amd.h.  One handle = one HIP device + one stream + one work arena.
//
// Reference control flow restated: hif::prec_solve, src/hif/alg/prec_solve.hpp:332-412 (stages
// S1..S7 of SURVEY 3.1), HIF::solve builder.hpp:409-423, IterRefine::iter_refine
// alg/IterRefine.hpp:77-165.  There is NO host fallback: every compute path needs a HIP device.
#include <hip/hip_runtime.h>

#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <type_traits>

#include "../../include/hifir_amd.h"
#include "host.hpp"
#include "import.hpp"
#include "kernels.hip.hpp"
#include "options.hpp"

namespace hifamd {

static thread_local std::string g_err;
static thread_local bool g_has_err = false;

static void set_err(const std::string &m) {
  g_err = m;
  g_has_err = true;
}

#define HIP_OK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      throw Error(HIFAMD_HIFIR_ERROR, std::string("HIP error: ") + hipGetErrorString(e_) + " at " \
                                          #expr + " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
  } while (0)

template <class T>
struct DevT;
template <>
struct DevT<double> {
  typedef double type;
};
template <>
struct DevT<zdouble> {
  typedef cplx type;
};

static_assert(kMaxWgRows == HIFAMD_TAIL_MAX, "a thin band's rows must fit the LDS flags of k_trsv_band's sequential workgroup");

// -------------------------------------------------------------------------------------------
// Transfers never touch the legacy default stream: while ANOTHER host thread captures a graph on its
// handle's stream, ROCm rejects any legacy-stream operation in the process ("would make the legacy
// stream depend on a capturing blocking stream"), and handles are meant to be usable from distinct
// threads.  One non-blocking transfer stream per device, always synchronised before returning.
// -------------------------------------------------------------------------------------------
static hipStream_t xfer_stream() {
  static std::mutex mx;
  static hipStream_t s[64] = {};
  int d = 0;
  HIP_OK(hipGetDevice(&d));
  std::lock_guard<std::mutex> lk(mx);
  if (!s[d & 63]) HIP_OK(hipStreamCreateWithFlags(&s[d & 63], hipStreamNonBlocking));
  return s[d & 63];
}
static void copy_h2d(void *dst, const void *src, size_t n) {
  if (!n) return;
  hipStream_t xs = xfer_stream();
  HIP_OK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, xs));
  HIP_OK(hipStreamSynchronize(xs));
}
static void copy_d2h(void *dst, const void *src, size_t n) {
  if (!n) return;
  hipStream_t xs = xfer_stream();
  HIP_OK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, xs));
  HIP_OK(hipStreamSynchronize(xs));
}
static void zero_dev(void *p, size_t n) {
  if (!n) return;
  hipStream_t xs = xfer_stream();
  HIP_OK(hipMemsetAsync(p, 0, n, xs));
  HIP_OK(hipStreamSynchronize(xs));
}

// -------------------------------------------------------------------------------------------
// device containers
// -------------------------------------------------------------------------------------------
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  bool owner = true;  // false: a view of another engine's read-only data (see Engine::twin)
  void alias(const DevBuf &o) {
    release();
    p = o.p;
    bytes = o.bytes;
    owner = false;
  }
  void view(const DevBuf &o, size_t offset, size_t b) {  // a window of another buffer (not owned)
    release();
    p = (char *)o.p + offset;
    bytes = b;
    owner = false;
  }
  void alloc(size_t b) {
    release();
    bytes = b;
    if (b) HIP_OK(hipMalloc(&p, b));
  }
  template <class V>
  void upload(const std::vector<V> &h, size_t pad_elems = 0) {
    alloc((h.size() + pad_elems) * sizeof(V));
    // ONE blocking copy covers the whole buffer (zero padding included): no asynchronous memset is left
    // pending behind it (a hipMemset queued before a small blocking hipMemcpy was seen to land after it)
    if (pad_elems) {
      std::vector<V> padded(h.size() + pad_elems);
      std::copy(h.begin(), h.end(), padded.begin());
      std::fill(padded.begin() + (std::ptrdiff_t)h.size(), padded.end(), V());
      copy_h2d(p, padded.data(), bytes);
    } else if (!h.empty()) {
      copy_h2d(p, h.data(), bytes);
    }
  }
  void release() {
    if (p && owner) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    owner = true;
  }
  ~DevBuf() { release(); }
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  template <class V>
  V *as() const {
    return (V *)p;
  }
};

struct DevCsr {
  int64_t nrows = 0, ncols = 0, nnz = 0;
  DevBuf ptr, col, val, rowid;
  // band plan of a triangle (host.hpp BandPlan); empty for E, F, A
  DevBuf srcslot, split, wg_grp_ptr, grp_slot_ptr;
  DevBuf wg_slot;  // first slot of every workgroup (+ end): grp_slot_ptr[wg_grp_ptr[g]], one load level less at kernel start
  DevBuf csplit, grp_inv_off, cd_desc, mid_col, mid_val, mid_lrow;  // component-dense bands (host.hpp plan_bands_cd)
  DevBuf own_val, own_lsrc, own_rptr, own_lvl;                        // ... sparse-own plans (BandPlan::cd_sparse)
  DevBuf f_desc, f_col, f_val, f_lrow;  // L only: the streams with the level's F entries appended (host.hpp build_cd_streams_fused)
  bool f_fused = false;
  // tile form of the dense-own component bands' walked entries (host.hpp build_ct_tiles, kernel k_band_ct)
  DevBuf rowflag;  // sparse-own plans: per slot, what a level's FIRST solve may leave out (build_row_flags; kernels RowSkip)
  // U triangles of sparse-own plans: black rows in LDS, sinks streamed (host.hpp build_us_plan; kernel k_band_us)
  DevBuf us_desc, us_rowid, us_oslot, us_mptr, us_mcol, us_mval, us_own_val, us_own_src, us_own_rptr, us_own_lvl;
  std::vector<uint8_t> us_band_ok;
  std::vector<int32_t> us_band_nbk, us_band_own, us_band_c0;
  // L triangles of sparse-own plans: dependent rows in LDS, sources streamed through a chunk (host.hpp build_ls_plan; kernel k_band_ls)
  DevBuf ls_desc, ls_rowid, ls_oslot, ls_own_val, ls_own_src, ls_own_rptr, ls_own_lvl;
  DevBuf ls_ebase[2], ls_ewptr[2], ls_ecol[2], ls_eval[2], ls_etag[2];  // outside entries: [0] plain, [1] with the level's F entries
  bool ls_fused = false;
  std::vector<uint8_t> ls_band_ok;
  std::vector<int32_t> ls_band_nd, ls_band_own, ls_band_rptr, ls_band_c0, ls_band_cw, ls_band_nch;
  int64_t ls_sources = 0, ls_deps = 0, ls_chunk_rows = 0;
  DevBuf ct_desc, ct_sptr, ct_src, ct_coef;
  bool ct_on = false;
  int64_t ct_tiles = 0;
  std::vector<int32_t> band_wave_tiles;  // per band: most tiles one wave of one component walks
  bool cd_sparse = false;
  std::vector<int32_t> band_chunk_max;  // component bands: most entries of one wave chunk of the band (the serial walk of its slowest wave)
  int32_t own_cap = kCdOwnCap;  // sparse-own plans: most own nonzeros of one component, rounded up to 64 (sizes the kernels' LDS)
  std::vector<int32_t> band_wg_ptr, band_slot_ptr, host_wg_grp_ptr;
  std::vector<uint8_t> band_prefix, band_dense, band_fused, band_cd, band_old;
  std::vector<int32_t> band_blk_ptr, blk_slot0, blk_slot1;
  std::vector<int64_t> blk_inv_off;
  DevBuf tinv;  // explicit inverses of the diagonal blocks of block-dense thin bands
  // tiled form of a coupling block (E, F) for k_spmm_tile (host.hpp SpmmTiles); nblk == 0: not built
  DevBuf tl_gptr, tl_ucol, tl_coef;
  int64_t tl_nblk = 0;
  int tl_rb = 1;  // 16-row tiles per block (host.hpp SpmmTiles::rb)

  void alias(const DevCsr &o) {  // share the device arrays, copy the (small) host-side launch metadata
    nrows = o.nrows;
    ncols = o.ncols;
    nnz = o.nnz;
    ptr.alias(o.ptr);
    col.alias(o.col);
    val.alias(o.val);
    rowid.alias(o.rowid);
    srcslot.alias(o.srcslot);
    split.alias(o.split);
    wg_grp_ptr.alias(o.wg_grp_ptr);
    grp_slot_ptr.alias(o.grp_slot_ptr);
    wg_slot.alias(o.wg_slot);
    csplit.alias(o.csplit);
    own_cap = o.own_cap;
    band_chunk_max = o.band_chunk_max;
    grp_inv_off.alias(o.grp_inv_off);
    cd_desc.alias(o.cd_desc);
    mid_col.alias(o.mid_col);
    mid_val.alias(o.mid_val);
    mid_lrow.alias(o.mid_lrow);
    own_val.alias(o.own_val);
    own_lsrc.alias(o.own_lsrc);
    own_rptr.alias(o.own_rptr);
    own_lvl.alias(o.own_lvl);
    f_desc.alias(o.f_desc);
    f_col.alias(o.f_col);
    f_val.alias(o.f_val);
    f_lrow.alias(o.f_lrow);
    f_fused = o.f_fused;
    rowflag.alias(o.rowflag);
    us_desc.alias(o.us_desc), us_rowid.alias(o.us_rowid), us_oslot.alias(o.us_oslot), us_mptr.alias(o.us_mptr), us_mcol.alias(o.us_mcol);
    us_mval.alias(o.us_mval), us_own_val.alias(o.us_own_val), us_own_src.alias(o.us_own_src), us_own_rptr.alias(o.us_own_rptr);
    us_own_lvl.alias(o.us_own_lvl);
    us_band_ok = o.us_band_ok, us_band_nbk = o.us_band_nbk, us_band_own = o.us_band_own, us_band_c0 = o.us_band_c0;
    ls_desc.alias(o.ls_desc), ls_rowid.alias(o.ls_rowid), ls_oslot.alias(o.ls_oslot), ls_own_val.alias(o.ls_own_val);
    ls_own_src.alias(o.ls_own_src), ls_own_rptr.alias(o.ls_own_rptr), ls_own_lvl.alias(o.ls_own_lvl);
    for (int f = 0; f < 2; ++f)
      ls_ebase[f].alias(o.ls_ebase[f]), ls_ewptr[f].alias(o.ls_ewptr[f]), ls_ecol[f].alias(o.ls_ecol[f]), ls_eval[f].alias(o.ls_eval[f]),
          ls_etag[f].alias(o.ls_etag[f]);
    ls_fused = o.ls_fused;
    ls_band_ok = o.ls_band_ok, ls_band_nd = o.ls_band_nd, ls_band_own = o.ls_band_own, ls_band_rptr = o.ls_band_rptr;
    ls_band_c0 = o.ls_band_c0, ls_band_cw = o.ls_band_cw, ls_band_nch = o.ls_band_nch;
    ls_sources = o.ls_sources, ls_deps = o.ls_deps, ls_chunk_rows = o.ls_chunk_rows;
    ct_desc.alias(o.ct_desc);
    ct_sptr.alias(o.ct_sptr);
    ct_src.alias(o.ct_src);
    ct_coef.alias(o.ct_coef);
    ct_on = o.ct_on;
    ct_tiles = o.ct_tiles;
    band_wave_tiles = o.band_wave_tiles;
    cd_sparse = o.cd_sparse;
    band_cd = o.band_cd;
    band_old = o.band_old;
    host_wg_grp_ptr = o.host_wg_grp_ptr;
    tinv.alias(o.tinv);
    tl_gptr.alias(o.tl_gptr);
    tl_ucol.alias(o.tl_ucol);
    tl_coef.alias(o.tl_coef);
    tl_nblk = o.tl_nblk;
    tl_rb = o.tl_rb;
    band_wg_ptr = o.band_wg_ptr;
    band_slot_ptr = o.band_slot_ptr;
    band_prefix = o.band_prefix;
    band_fused = o.band_fused;
    band_dense = o.band_dense;
    band_blk_ptr = o.band_blk_ptr;
    blk_slot0 = o.blk_slot0;
    blk_slot1 = o.blk_slot1;
    blk_inv_off = o.blk_inv_off;
  }
  template <class T>
  void upload(const Csr<T> &A, const BandPlan *P) {
    nrows = A.nrows;
    ncols = A.ncols;
    nnz = (int64_t)A.col.size();
    ptr.upload(A.ptr);
    col.upload(A.col, 80);  // padded: a 64-wide item load may start at the last nonzero
    val.upload(A.val, 80);
    rowid.upload(A.rowid);
    if (P) {
      srcslot.upload(P->srcslot, 80);
      split.upload(P->split);
      wg_grp_ptr.upload(P->wg_grp_ptr);
      grp_slot_ptr.upload(P->grp_slot_ptr);
      {
        std::vector<int32_t> ws(P->wg_grp_ptr.size());
        for (size_t g = 0; g < ws.size(); ++g) ws[g] = P->grp_slot_ptr[(size_t)P->wg_grp_ptr[g]];
        wg_slot.upload(ws);
      }
      csplit.upload(P->csplit);
      grp_inv_off.upload(P->grp_inv_off);
      cd_desc.upload(P->cd_desc);
      {  // the packed gather streams of the component-dense bands: column and value of every entry, 80 padding entries
        std::vector<int32_t> mc(P->mid_k.size());
        std::vector<T> mv(P->mid_k.size());
        for (size_t e = 0; e < mc.size(); ++e) mc[e] = A.col[(size_t)P->mid_k[e]], mv[e] = A.val[(size_t)P->mid_k[e]];
        mid_col.upload(mc, 80);
        mid_val.upload(mv, 80);
        mid_lrow.upload(P->mid_lrow, 80);
        cd_sparse = P->cd_sparse;
        band_chunk_max.assign(P->band_wg_ptr.size() - 1, 0);
        for (size_t b = 0; b + 1 < P->band_wg_ptr.size(); ++b) {
          if (P->band_cd.empty() || !P->band_cd[b] || P->cd_desc.empty()) continue;
          for (int32_t c = P->wg_grp_ptr[(size_t)P->band_wg_ptr[b]]; c < P->wg_grp_ptr[(size_t)P->band_wg_ptr[b + 1]]; ++c) {
            const uint16_t *wm = reinterpret_cast<const uint16_t *>(&P->cd_desc[(size_t)c * kCdDescWords + 11]);
            for (int q = 0; q < 16; ++q) band_chunk_max[b] = std::max<int32_t>(band_chunk_max[b], (int32_t)wm[q + 1] - (int32_t)wm[q]);
          }
        }
        if (cd_sparse) {
          int32_t mx = 0;
          for (size_t c = 0; c * kCdDescWords < P->cd_desc.size(); ++c) mx = std::max(mx, P->cd_desc[c * kCdDescWords + 21]);
          own_cap = std::min<int32_t>(kCdOwnCap, std::max<int32_t>(64, (mx + 63) & ~63));
        }
        std::vector<T> ov(P->own_k.size());
        for (size_t e = 0; e < ov.size(); ++e) ov[e] = A.val[(size_t)P->own_k[e]];
        own_val.upload(ov, 8);
        own_lsrc.upload(P->own_lsrc, 8);
        own_rptr.upload(P->own_rptr, 8);
        own_lvl.upload(P->own_lvl, 8);
      }
      band_cd = P->band_cd;
      band_old = P->band_old;
      host_wg_grp_ptr = P->wg_grp_ptr;
      band_wg_ptr = P->band_wg_ptr;
      band_prefix = P->band_prefix;
      band_fused = P->band_fused;
      band_dense = P->band_dense;
      band_blk_ptr = P->band_blk_ptr;
      blk_slot0 = P->blk_slot0;
      blk_slot1 = P->blk_slot1;
      blk_inv_off = P->blk_inv_off;
      band_slot_ptr.clear();
      for (size_t b = 0; b < band_wg_ptr.size(); ++b)
        band_slot_ptr.push_back(P->grp_slot_ptr[(size_t)P->wg_grp_ptr[(size_t)band_wg_ptr[b]]]);
    }
  }
};

struct DevLevel {
  int64_t m = 0, n = 0, F_ncols = 0;
  bool E_void = false;  // adjoint of a level without F: the restriction F^H does not exist (not merely empty)
  DevCsr L, U, E, F;
  DevBuf d, s, t, p, qinv;
  DevBuf w, v;  // arena: n * Rmax each, v right behind w in ONE allocation (row n + i of w is row i of v: the fused
                // F streams address the child's solution through the L solve's vector)
  DevBuf arena;
  // S7 fused into the last band of the final U solve (kernels LastU): q on the device, and the output rows the band
  // does not write itself (the other bands' rows and the child's)
  DevBuf q_s7, s7_list;
  int64_t s7_n = -1;  // -1: not fused
  int64_t s7_child = 0;  // the list's first s7_child rows are the CHILD's (nothing of this level's second solve feeds them)
  int64_t skip_w = 0, skip_v = 0;  // rows the first solve does not store (L.rowflag bit 0 / U.rowflag bit 0)
  void alloc_arena(size_t bytes_each) {
    arena.alloc(2 * bytes_each);
    w.view(arena, 0, bytes_each);
    v.view(arena, bytes_each, bytes_each);
  }
  // combined top operator G = U_TT^{-1} D_T^{-1} L_TT^{-1} (host.hpp choose_top / build_top_operator), MFMA operand
  DevBuf topG;
  int64_t top_n = 0;
  int32_t top_bandL = -1, top_bandU = -1;
  DevBuf q, pinv;        // product only (prec_prod.hpp:76,132), uploaded with the product buffers
  DevBuf pg, pc, pr;     // product only: permuted input, child product / D(U+I)g, result rows
};

struct DevDense {
  int64_t n = 0, rank = 0;
  bool symm = false;  // SYEIG last level: QH = diag(1/w) V^H, Qm = V (truncation order), Rm = diag(w) V^H
  bool lup = false;   // LUP last level: QH = A^{-1} (adjoint engine: its transpose), Rm = A (adjoint: A^H)
  DevBuf QH, Rinv, jpvt0, tmp;
  DevBuf Qm, RinvH, tmp2;  // adjoint engine only: Q, (R^{-1})^H and the permuted input
  DevBuf Rm;               // product only: R (primary engine, upper) or R^H (adjoint engine, lower)
};

struct GraphKey {  // one graph per SHAPE: the caller's pointers are read from a device slot at replay time
  int64_t ldb, ldx, nrhs, rank;
  int kind;            // 0: apply (prec_solve), 1: product (prec_prod)
  int tfirst, tstride; // which 64-column tiles this graph covers (the twin engine takes every other one)
  bool operator<(const GraphKey &o) const {
    return std::tie(ldb, ldx, nrhs, rank, kind, tfirst, tstride) <
           std::tie(o.ldb, o.ldx, o.nrhs, o.rank, o.kind, o.tfirst, o.tstride);
  }
};

// Kernel families of the launch census (hifamd_kernel_census): one per kernel the dispatch can choose between.  THE order of
// the C call's output; kFamilyNames below and hifir_amd/hif.py KERNEL_FAMILIES follow it (tests/test_abi_and_host.py compares them)
enum KernelFamily {
  KF_BAND_CT1, KF_BAND_CT2, KF_BAND_CT4, KF_BAND_CD, KF_BAND_CD_SPARSE, KF_BAND_CS, KF_BAND_CS_SPARSE, KF_BAND_US, KF_BAND_LS,
  KF_BAND_CT_Z, KF_BAND_CS_Z, KF_BAND_CD_Z,
  KF_TRSV_BAND, KF_TRSV_BAND_P, KF_TRSV_WIDE, KF_THIN_UPDATE,
  KF_SPMM_TILE_RB1, KF_SPMM_TILE_RB2, KF_SPMM_TILE4_RB1, KF_SPMM_TILE4_RB2, KF_SPMM_TILE_Z, KF_SPMM_EPI, KF_SPMM_EPI_NARROW,
  KF_TOP_GEMM, KF_TOP_REDUCE, KF_STRIP_GEMM, KF_STRIP_GEMM4, KF_TRI_GEMM, KF_DENSE_GEMM, KF_ZCOMBINE,
  KF_GATHER_SCALE, KF_SCATTER_SCALE, KF_SCATTER_SCALE_LIST,
  KF_BAND_SPLIT_PREFIX,  // k_trsv_wide as the chip-wide prefix pass of a split component band (HIFIR_AMD_CD_SPLIT_MIN)
  KF_ROW_GATHER,         // the row permutation in front of the adjoint's dense block
  KF_PROD,               // every kernel of the product M b that the apply does not share (k_gather_div ... k_scatter_div)
  KF_TOP_GEMM_Z, KF_TOP_REDUCE_Z,  // top / tail operator products of a complex handle (hifamd_set_complex_operators)
  KF_COUNT
};
static const char *const kFamilyNames[KF_COUNT] = {
    "band_ct1", "band_ct2", "band_ct4", "band_cd", "band_cd_sparse", "band_cs", "band_cs_sparse", "band_us", "band_ls",
    "band_ct_z", "band_cs_z", "band_cd_z",
    "trsv_band", "trsv_band_p", "trsv_wide", "thin_update",
    "spmm_tile_rb1", "spmm_tile_rb2", "spmm_tile4_rb1", "spmm_tile4_rb2", "spmm_tile_z", "spmm_epi", "spmm_epi_narrow",
    "top_gemm", "top_reduce", "strip_gemm", "strip_gemm4", "tri_gemm", "dense_gemm", "zcombine",
    "gather_scale", "scatter_scale", "scatter_scale_list",
    "band_split_prefix", "row_gather", "prod", "top_gemm_z", "top_reduce_z"};
// launches per family: [0, KF_COUNT) on every level, [KF_COUNT, 2 KF_COUNT) those of them on a level >= 1
typedef std::array<int32_t, 2 * KF_COUNT> Census;
// Graph capture, instantiation and launch are serialized across the handles of a process: distinct handles may be used from
// distinct host threads (hifir_amd.h), and the runtime's graph calls have not proved safe to interleave between threads (a
// host-side crash inside two concurrent applies of tests/test_gpu_parity.py::test_two_handles_from_two_threads).  Only the
// enqueue is inside the lock -- the kernels of two handles still overlap on the device -- and an uncontended lock costs
// nanoseconds per apply.
static std::mutex &graph_mutex() {
  static std::mutex m;
  return m;
}
static std::atomic<uint64_t> &census_clock() {
  static std::atomic<uint64_t> c{0};
  return c;
}

struct GraphEntry {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  void **slots = nullptr;  // device: {B base, X base}, rewritten (stream-ordered) before every replay
  int64_t launches = 0;
  uint64_t stamp = 0;
  std::vector<int32_t> map;  // per launch: 16 * level + stage (Engine::launch_map)
  Census census{};           // launches by kernel family (Engine::kernel_census)
};

class EngineBase {
 public:
  virtual ~EngineBase() {}
  int vt = 0;
};

template <class T>
class Engine : public EngineBase {
 public:
  typedef T value_type;
  typedef typename DevT<T>::type D;
  // the C ABI's untyped blocks as this engine reads them: host arrays hold T, device arrays hold D
  static const T *val(const void *p) { return (const T *)p; }
  static T *val(void *p) { return (T *)p; }
  static const D *dev(const void *p) { return (const D *)p; }
  static D *dev(void *p) { return (D *)p; }
  int device = 0;
  hipStream_t stream = nullptr;
  bool owns_stream = true;  // the adjoint engine runs on its primary's stream
  bool finalized = false;
  int64_t Rmax = 0, max_nrhs = 0;
  HostHierarchy<T> host;
  // x = M^{-H} b (HIF::solve(b, x, true), prec_solve_tran, alg/prec_solve.hpp:542-612) is the SAME
  // machinery applied to the adjoint hierarchy: L' = U^H, U' = L^H, E' = F^H, F' = E^H, d' = conj(d),
  // (s', p') = (t, q), (t', q_inv') = (s, p_inv), dense block solved with A^H.  Built on first use.
  bool adjoint = false;
  std::unique_ptr<Engine<T>> adj;
  // Batches wider than 64 columns: the 64-column tiles are independent, and two of them in flight hide
  // each other's latency-bound phases (measured 1.37x at 128 columns).  The TWIN engine shares every
  // read-only device array of this one (matrices, inverses, permutations) and owns only a second work
  // arena and stream; odd tiles run there, even tiles here, joined by events.  Built on first use.
  bool is_twin = false;
  std::vector<std::unique_ptr<Engine<T>>> twins;
  hipEvent_t ev_fork = nullptr;
  std::vector<hipEvent_t> ev_join;
  // S7 of the child's rows beside the level's second solve (enqueue_level): a side stream and one fork / join event per level
  hipStream_t side_stream = nullptr;
  std::vector<hipEvent_t> ev_side_fork, ev_side_join;
  std::vector<std::unique_ptr<DevLevel>> lv;
  DevDense dn;
  DevCsr A;
  bool has_A = false;
  DevCsr Bm;  // the mass matrix of the generalized eigenproblem (set_mass_matrix)
  bool has_B = false;
  std::map<GraphKey, GraphEntry> graphs;
  static constexpr size_t kIoRing = 1024;  // pinned staging of the (B, X) pointers handed to the graphs
  void **io_ring = nullptr;
  uint64_t io_next = 0;
  uint64_t clock = 0;
  int64_t last_launches = 0;
  // which level and stage every launch of the apply being enqueued belongs to (16 * level + stage; stages: 1 S1 gather,
  // 2 first LDU solve incl. the fused S1, 3 S3 product with E, 4 dense block / tail operator, 5 S5 product with F,
  // 6 second LDU solve incl. the fused S5 / S7, 7 S7 scatter); last_map: of the apply launched last (hifamd_launch_map)
  std::vector<int32_t> cur_map, last_map;
  void mark(size_t level, int stage, int64_t c0, int64_t c1) {
    for (int64_t c = c0; c < c1; ++c) cur_map.push_back((int32_t)(16 * level + stage));
  }
  // launches by kernel family of the apply being enqueued, kept like the launch map (host-side bookkeeping at the launch
  // sites); last_census: of the apply launched last, summed over the twin lanes (hifamd_kernel_census).  census_seq orders
  // the applies of a handle's two engines: the call reports the one that ran last, forwards or adjoint.
  Census cur_census{}, last_census{};
  int cur_level = 0;
  uint64_t census_seq = 0;
  void tally(int family, int n = 1) {
    cur_census[(size_t)family] += n;
    if (cur_level >= 1) cur_census[(size_t)(KF_COUNT + family)] += n;
  }
  EngineOptions opt;  // the creation-time options (options.hpp)
  double spmm_tile_reuse = 2.0;  // opt.spmm_tiles ... when a 16-row block has at least this many nonzeros per distinct column
  int64_t tail_level = -1, tail_n = 0;  // the tail operator (opt.tail_rows)
  DevBuf tailG;
  double tail_probe_err = 0.0, tail_max_abs = 0.0;  // build_tail_operator: G c against the recursion on a probe, max |G|
  int tail_rejected = 0;                            // 1: not finite, 2: growth, 3: probe, 4: an error while building
  double finalize_seconds = 0.0, capture_ms = 0.0;  // set-up cost: hifamd_finalize, the last hipGraph capture + instantiate
  double bytes_inverses = 0.0, bytes_top = 0.0, bytes_tail = 0.0;  // resident explicit operators (HBM)
  DevBuf gemm_part;      // partial tiles of the K splits of k_top_gemm
  DevBuf gemm_cnt;       // ... and one arrival counter per 64-row tile (the last split to arrive adds them: no k_top_reduce launch)
  void set_complex_operators(int flags) {
    if (flags < 0 || flags > 3) throw Error(HIFAMD_MISMATCHED_SIZES, "complex operator flags must be 0 ... 3 (HIFAMD_ZOP_TAIL | HIFAMD_ZOP_TOP)");
    if (sizeof(T) == sizeof(double)) {
      if (flags != 0) throw Error(HIFAMD_BAD_PREC, "a real handle already has the tail and the top operators: the flags belong to complex handles");
      return;
    }
    if (finalized || !host.levels.empty())
      throw Error(HIFAMD_BAD_PREC, "complex operators are a planner option: set them before the first hifamd_add_level");
    opt.zop_flags = flags;
    opt.band.top_max = (flags & 2) ? opt.zop_top_max : 0;
  }
  // opt.cd_dbg: ... and bit 2048 (kDbgCtPlain), which switches nothing off: k_band_ct's phase 1 gathers a tile batch in front of its own
  // products, as it did before its requests ran ahead -- the same sums in the same order, the same bits; the tests' second opinion
  static constexpr int kDbgCtPlain = 2048;
  // ... and bit 4096 (kDbgSpmmPlain), which switches nothing off either: k_spmm_tile / k_spmm_tile4 run the group loop and the epilogue of
  // before their requests ran ahead (the second template instance) -- the same sums in the same order, the same bits
  static constexpr int kDbgSpmmPlain = 4096;
  int act_cols = 64;     // columns of the 64-column arena that the tile being enqueued actually uses (enqueue_apply)
  DevBuf errflag;        // sticky error word: a bounded spin of k_trsv_band expired
#ifdef HIFAMD_PROBE
  DevBuf probe;          // development probe (make PROBE=1): wave timestamps of k_trsv_band, dumped at destruction
#endif
#ifdef HIFAMD_CSPROBE
  DevBuf csprobe;        // development probe (make CSPROBE=1): phase stamps of the component band kernels
  void csprobe_reset() {
    if (!csprobe.p) return;
    const unsigned z = 0;
    HIP_OK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_csprobe_cnt), &z, sizeof(z), 0, hipMemcpyHostToDevice, xfer_stream()));
    HIP_OK(hipStreamSynchronize(xfer_stream()));
  }
  void csprobe_dump() {
    if (!csprobe.p || !getenv("HIFIR_AMD_CSPROBE_OUT")) return;
    (void)hipDeviceSynchronize();
    unsigned cnt = 0;
    (void)hipMemcpyFromSymbol(&cnt, HIP_SYMBOL(g_csprobe_cnt), sizeof(cnt));
    cnt = std::min(cnt, 400000u);
    std::vector<unsigned long long> h((size_t)cnt * 12);
    if (cnt) (void)hipMemcpy(h.data(), csprobe.p, h.size() * 8, hipMemcpyDeviceToHost);
    if (FILE *f = fopen(getenv("HIFIR_AMD_CSPROBE_OUT"), "wb")) {
      fwrite(h.data(), 8, h.size(), f);
      fclose(f);
    }
    unsigned long long *np = nullptr;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_csprobe), &np, sizeof(np));
  }
#endif
  DevBuf blk_tmp;        // right-hand side of one diagonal block of a block-dense thin band
  DevBuf zt1, zt2;       // complex handles: the two real partial products A_re X, A_im X (k_zcombine)
  // IR scratch
  DevBuf ir_r, ir_xk, ir_part, stage_b, stage_x;
  // constant-mode null-space filter of this engine's solve (HIF::nsp on the primary, HIF::nsp_tran on the adjoint)
  bool nsp_on = false;
  int64_t nsp_r0 = 0, nsp_r1 = -1;
  DevBuf nsp_part;
  // basis mode (hifamd_set_nsp_basis): Q [n][nsp_kp] orthonormal, nsp_k vectors padded with zero vectors to nsp_kp; the
  // block partials [nsp_kp][kCgBlocks][64] and the coefficients [nsp_kp][64] of one tile.  One filter per engine:
  // nsp_on and nsp_k > 0 exclude each other.  (Twin engines never filter: solve_dev filters after their join.)
  int nsp_k = 0, nsp_kp = 0;
  DevBuf nsp_Q, nsp_cpart, nsp_C;
  DevBuf gm_Q, gm_Z;  // GMRES: Krylov basis, flexible: the preconditioned vectors (its work vectors: kr_vec, its scalars: kr_state)
  int64_t ir_cols = 0;

  // Every read-back of the engine's own (counters, flags, norms, small matrices; not the callers' arrays, which the host
  // entries copy under StreamWait or staged): `count` values of V from `dev` on `stream` into the one pinned buffer, waited
  // for before the return.  The buffer grows on demand and is freed by ~Engine only, so no copy outlives its destination
  // whichever call throws.  The pointer holds until the next read_back.
  void *rb_pin = nullptr;
  size_t rb_cap = 0;
  template <class V>
  const V *read_back(const void *dev, size_t count) {
    const size_t bytes = count * sizeof(V);
    if (rb_cap < bytes) {
      if (rb_pin) HIP_OK(hipHostFree(rb_pin));
      rb_pin = nullptr, rb_cap = 0;
      const size_t cap = std::max<size_t>(bytes, 4096);
      HIP_OK(hipHostMalloc(&rb_pin, cap, hipHostMallocDefault));
      rb_cap = cap;
    }
    HIP_OK(hipMemcpyAsync(rb_pin, dev, bytes, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    return (const V *)rb_pin;
  }

  // Import and host-side analysis (CCS -> CSR, level schedules, dense QRCP) need no GPU; the
  // device is bound in finalize(), and every compute entry point requires a finalized handle.
  // The handle's engine gets what EngineOptions::from_env read when the handle was created; the adjoint engine and the
  // twin lanes, built on first use long after, get their handle's `opt` and never look at the environment.
  Engine(int dev, const EngineOptions &o) : device(dev), opt(o) {}

  void bind_device() {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0)
      throw Error(HIFAMD_HIFIR_ERROR, "no HIP device available: the hifir_amd apply path has no CPU fallback");
    if (device < 0) HIP_OK(hipGetDevice(&device));
    if (device >= cnt) throw Error(HIFAMD_HIFIR_ERROR, "device ordinal out of range");
    HIP_OK(hipSetDevice(device));
    if (!stream) HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (const auto &e : band_lds_table())  // (a launch of up to 64 KB needs no raised limit)
      if (e.second > 64 * 1024) HIP_OK(hipFuncSetAttribute(e.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)e.second));
    HIP_OK(hipFuncSetAttribute((const void *)k_top_gemm<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTopGemmLds));
    HIP_OK(hipFuncSetAttribute((const void *)k_top_gemm<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTopGemmLds));
    HIP_OK(hipFuncSetAttribute((const void *)k_top_gemm<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTopGemmLds));
    HIP_OK(hipFuncSetAttribute((const void *)k_top_gemm<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTopGemmLds));
    if (sizeof(T) != sizeof(double) && opt.zop_flags) {
      HIP_OK(hipFuncSetAttribute((const void *)k_top_gemm_z<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTopGemmLds));
      HIP_OK(hipFuncSetAttribute((const void *)k_top_gemm_z<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTopGemmLds));
    }
  }

  ~Engine() override {
    if (stream) (void)hipSetDevice(device);
    // nothing of this handle may still be in flight when its graphs, events, streams and pinned buffers go (the runtime
    // completes asynchronous work on threads of its own; see DESIGN 8 on the host copy that changed twice in four rounds)
    if (stream && !is_twin) (void)hipDeviceSynchronize();
    if (rb_pin) (void)hipHostFree(rb_pin);
#ifdef HIFAMD_CSPROBE
    csprobe_dump();
#endif
#ifdef HIFAMD_PROBE
    if (probe.p && getenv("HIFIR_AMD_PROBE_OUT")) {
      std::vector<unsigned long long> h(probe.bytes / 8);
      (void)hipDeviceSynchronize();
      (void)hipMemcpy(h.data(), probe.p, probe.bytes, hipMemcpyDeviceToHost);
      if (FILE *f = fopen(getenv("HIFIR_AMD_PROBE_OUT"), "wb")) {
        fwrite(h.data(), 8, h.size(), f);
        fclose(f);
      }
    }
#endif
    adj.reset();
    twins.clear();
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    for (auto e : ev_join) (void)hipEventDestroy(e);
    for (auto e : ev_side_fork) (void)hipEventDestroy(e);
    for (auto e : ev_side_join) (void)hipEventDestroy(e);
    clear_graphs();
    if (side_stream) (void)hipStreamDestroy(side_stream);
    if (stream && owns_stream) (void)hipStreamDestroy(stream);
  }

  void clear_graphs() {
    for (auto &kv : graphs) {
      if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
      if (kv.second.graph) (void)hipGraphDestroy(kv.second.graph);
      if (kv.second.slots) (void)hipFree(kv.second.slots);
    }
    graphs.clear();
    if (io_ring) (void)hipHostFree(io_ring);
    io_ring = nullptr;
  }

  // ---- import (validation, conversion and analysis live in import.hpp: host-only, sanitizer-tested) ----------
  void add_level(int64_t m, int64_t n, const int64_t *Lcp, const int32_t *Lri, const T *Lv,
                 const int64_t *Ucp, const int32_t *Uri, const T *Uv, const int64_t *Ecp,
                 const int32_t *Eri, const T *Ev, int64_t F_ncols, const int64_t *Fcp,
                 const int32_t *Fri, const T *Fv, const T *d, const double *s, const double *t,
                 const int32_t *p, const int32_t *p_inv, const int32_t *q, const int32_t *q_inv) {
    if (finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy already finalized");
    if (host.has_dense) throw Error(HIFAMD_BAD_PREC, "the dense block must come after the last level");
    const int64_t parent_nm = host.levels.empty() ? -1 : host.levels.back().n - host.levels.back().m;
    HostLevel<T> H = import_level<T>(parent_nm, m, n, Lcp, Lri, Lv, Ucp, Uri, Uv, Ecp, Eri, Ev, F_ncols, Fcp, Fri, Fv, d, s,
                                     t, p, p_inv, q, q_inv);
    // (hifamd_load of a file that carries the analysis of its levels -- import.hpp load_analysis: adopted, not redone)
    const size_t li = host.levels.size();
    const auto t_an0 = std::chrono::steady_clock::now();
    if (li < cached_analysis.size() && adopt_analysis(H, cached_analysis[li], opt.band))
      ++levels_from_cache;
    else
      analyze_level(H, opt.band, env_int("HIFIR_AMD_PLAN_DUMP", 0) != 0, li);
    analysis_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_an0).count();
    seal_level(H);  // (what finalize must find again: import.hpp verify_level)
    host.levels.push_back(std::move(H));
    herm_known = false;
  }
  // hifamd_hermitian: import.hpp check_hermitian over the host copy, computed once per imported hierarchy
  bool herm_known = false;
  HermCheck herm;
  const HermCheck &hermitian() {
    if (!herm_known) herm = check_hermitian(host), herm_known = true;
    return herm;
  }
  int64_t host_repairs = 0;  // arrays of the host copy that verify_level found changed and rebuilt (hifamd_stats_ext slot 21)
  std::vector<LevelAnalysis<T>> cached_analysis;  // (alive during hifamd_load only)
  int64_t levels_from_cache = 0;
  double analysis_seconds = 0.0;  // host seconds spent analyzing (or adopting the analysis of) the levels

  // the adjoint of one imported level (see `adj` above)
  void add_level_adjoint(const HostLevel<T> &P) {
    HostLevel<T> H = adjoint_level(P);
    analyze_level(H, opt.band, env_int("HIFIR_AMD_PLAN_DUMP", 0) != 0, host.levels.size());
    seal_level(H);
    host.levels.push_back(std::move(H));
  }

  // the residual mode of this engine and of every engine built from it so far (those built later inherit it)
  void set_resid_mode(int mode) {
    opt.resid_mode = mode;
    for (auto &tw : twins) tw->set_resid_mode(mode);
    if (adj) adj->set_resid_mode(mode);
  }

  Engine<T> &adjoint_engine() {
    if (adjoint) throw Error(HIFAMD_HIFIR_ERROR, "internal error: adjoint of the adjoint engine");
    if (!finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
    if (!adj) {
      std::unique_ptr<Engine<T>> E(new Engine<T>(device, opt));
      E->adjoint = true;
      E->stream = stream;
      E->owns_stream = false;
      for (const auto &P : host.levels) E->add_level_adjoint(P);
      if (host.has_dense && host.dense.kind == 2) {  // LUP: ?getrs 'T' / ?gemv 'C' (LUP.hpp:150,187)
        E->host.dense.kind = 2;
        E->host.dense.n = host.dense.n;
        E->host.dense.rank = host.dense.rank;
        E->host.dense.mat = host.dense.mat;
        E->host.dense.qr = host.dense.qr;
        E->host.dense.jpvt0 = host.dense.jpvt0;
        dense_lup_ops(E->host.dense, true);
        E->host.has_dense = true;
      } else if (host.has_dense && host.dense.kind == 1) {
        // Hermitian last level: the conjugate-transpose solve IS the solve (prec_solve.hpp:583-584)
        E->host.dense.kind = 1;
        E->host.dense.spd = host.dense.spd;
        E->host.dense.n = host.dense.n;
        E->host.dense.rank = host.dense.rank;
        E->host.dense.w = host.dense.w;
        E->host.dense.trunc = host.dense.trunc;
        E->host.dense.evec = host.dense.evec;
        dense_symm_ops(E->host.dense);
        E->host.has_dense = true;
      } else if (host.has_dense) {
        E->host.dense.n = host.dense.n;
        E->host.dense.rank = host.dense.rank;
        E->host.dense.qr = host.dense.qr;
        E->host.dense.tau = host.dense.tau;
        E->host.dense.jpvt0 = host.dense.jpvt0;
        dense_adjoint_ops(E->host.dense);
        E->host.has_dense = true;
      }
      E->finalize(max_nrhs);
      if (has_A) E->upload_matrix(adjoint_of_csr(host.A));
      adj = std::move(E);
    }
    return *adj;
  }

  Engine<T> &twin_engine(int k) {
    while ((int)twins.size() <= k) {
      std::unique_ptr<Engine<T>> E(new Engine<T>(device, opt));
      E->is_twin = true;
      E->adjoint = adjoint;
      E->max_nrhs = max_nrhs;
      E->Rmax = Rmax;
      E->host.has_dense = host.has_dense;
      E->bind_device();  // its own stream
      for (const auto &Pl : lv) {
        std::unique_ptr<DevLevel> Lp(new DevLevel());
        DevLevel &L = *Lp;
        L.m = Pl->m;
        L.n = Pl->n;
        L.F_ncols = Pl->F_ncols;
        L.E_void = Pl->E_void;
        L.L.alias(Pl->L);
        L.U.alias(Pl->U);
        L.E.alias(Pl->E);
        L.F.alias(Pl->F);
        L.topG.alias(Pl->topG);
        L.top_n = Pl->top_n;
        L.top_bandL = Pl->top_bandL;
        L.top_bandU = Pl->top_bandU;
        L.d.alias(Pl->d);
        L.s.alias(Pl->s);
        L.t.alias(Pl->t);
        L.p.alias(Pl->p);
        L.qinv.alias(Pl->qinv);
        L.q_s7.alias(Pl->q_s7);
        L.s7_list.alias(Pl->s7_list);
        L.s7_n = Pl->s7_n;
        L.s7_child = Pl->s7_child;
        L.alloc_arena(Pl->w.bytes);
        if (L.w.bytes) zero_dev(L.w.p, L.w.bytes);
        if (L.v.bytes) zero_dev(L.v.p, L.v.bytes);
        E->lv.push_back(std::move(Lp));
      }
      E->tailG.alias(tailG);
      E->tail_level = tail_level;
      E->tail_n = tail_n;
      E->dn.n = dn.n;
      E->dn.rank = dn.rank;
      E->dn.symm = dn.symm;
      E->dn.lup = dn.lup;
      E->dn.QH.alias(dn.QH);
      E->dn.Rinv.alias(dn.Rinv);
      E->dn.jpvt0.alias(dn.jpvt0);
      E->dn.Qm.alias(dn.Qm);
      E->dn.RinvH.alias(dn.RinvH);
      if (dn.tmp.bytes) E->dn.tmp.alloc(dn.tmp.bytes);
      if (dn.tmp2.bytes) E->dn.tmp2.alloc(dn.tmp2.bytes);
      E->errflag.alloc(sizeof(unsigned));
      zero_dev(E->errflag.p, E->errflag.bytes);
      if (blk_tmp.bytes) {
        E->blk_tmp.alloc(blk_tmp.bytes);
        zero_dev(E->blk_tmp.p, E->blk_tmp.bytes);
      }
      if (gemm_part.bytes) E->gemm_part.alloc(gemm_part.bytes);
      if (gemm_cnt.bytes) {
        E->gemm_cnt.alloc(gemm_cnt.bytes);
        zero_dev(E->gemm_cnt.p, E->gemm_cnt.bytes);
      }
      if (zt1.bytes) {
        E->zt1.alloc(zt1.bytes);
        E->zt2.alloc(zt2.bytes);
      }
      hipEvent_t ej = nullptr;
      HIP_OK(hipEventCreateWithFlags(&ej, hipEventDisableTiming));
      ev_join.push_back(ej);
      HIP_OK(hipStreamSynchronize(stream));  // (transfers were synchronous on the transfer stream)
      E->finalized = true;
      twins.push_back(std::move(E));
    }
    return *twins[(size_t)k];
  }

  // the twin's share of the product set-up: views of the operators, its own three row buffers
  void ensure_prod_buffers_as_twin(const Engine<T> &P) {
    if (prod_ready) return;
    for (size_t l = 0; l < lv.size(); ++l) {
      DevLevel &L = *lv[l];
      const DevLevel &Q = *P.lv[l];
      L.q.alias(Q.q);
      L.pinv.alias(Q.pinv);
      L.pg.alloc(Q.pg.bytes);
      L.pc.alloc(Q.pc.bytes);
      L.pr.alloc(Q.pr.bytes);
    }
    dn.QH.alias(P.dn.QH);
    dn.Qm.alias(P.dn.Qm);
    dn.Rm.alias(P.dn.Rm);
    if (P.dn.tmp2.bytes && !dn.tmp2.bytes) dn.tmp2.alloc(P.dn.tmp2.bytes);
    HIP_OK(hipStreamSynchronize(stream));  // (transfers were synchronous on the transfer stream)
    prod_ready = true;
  }

  void set_dense(int64_t nd, const T *mat, double rrqr_cond) {
    if (finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy already finalized");
    if (host.levels.empty()) throw Error(HIFAMD_BAD_PREC, "add the sparse levels before the dense block");
    const auto &last = host.levels.back();
    if (nd != last.n - last.m) throw Error(HIFAMD_MISMATCHED_SIZES, "dense block size must be n-m of the last level");
    if (!mat) throw Error(HIFAMD_NULL_OBJ, "NULL dense block");
    dense_factorize(host.dense, mat, nd, rrqr_cond);
    host.has_dense = true;
    herm_known = false;
  }

  // LU last level of a reference built with HIF_DENSE_MODE=0 (small_scale/LUP.hpp)
  void set_dense_lup(int64_t nd, const T *mat) {
    if (finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy already finalized");
    if (host.levels.empty()) throw Error(HIFAMD_BAD_PREC, "add the sparse levels before the dense block");
    const auto &last = host.levels.back();
    if (nd != last.n - last.m) throw Error(HIFAMD_MISMATCHED_SIZES, "dense block size must be n-m of the last level");
    if (!mat) throw Error(HIFAMD_NULL_OBJ, "NULL dense block");
    dense_factorize_lup(host.dense, mat, nd);
    host.has_dense = true;
    herm_known = false;
  }

  // symmetric / Hermitian last level (the reference's symm_dense_solver, filled by symm_factor.hpp:654-657)
  void set_dense_symm(int64_t nd, const T *mat, int spd) {
    if (finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy already finalized");
    if (host.levels.empty()) throw Error(HIFAMD_BAD_PREC, "add the sparse levels before the dense block");
    const auto &last = host.levels.back();
    if (nd != last.n - last.m) throw Error(HIFAMD_MISMATCHED_SIZES, "dense block size must be n-m of the last level");
    if (!mat) throw Error(HIFAMD_NULL_OBJ, "NULL dense block");
    dense_factorize_symm(host.dense, mat, nd, spd);
    host.has_dense = true;
    herm_known = false;
  }

  // What the FIRST solve of a level (S2, prec_solve.hpp:364) need not move (round 4).  Its result y_1 only feeds the Schur
  // right-hand side b_2 - E y_1 (:366-368) -- the second solve starts again from b_1 -- and level 0 of a PDE hierarchy is
  // two thirds rows WITHOUT any L entry (their L solve is the copy s[p] b[p]).  For the rows of a level (without a top
  // operator) that sit in sparse-own component bands which touch them first, in BOTH triangles:
  //   L slot, bit 0: the row has no entry and no row outside its own component reads it: the L band keeps it in LDS for its
  //                  component and does not store it;
  //   U slot, bit 1: that row: the U band takes its right-hand side from the level's input (same product, same bits);
  //   U slot, bit 0: no column of E and no row outside the component refers to the row: its result is not stored.
  // Rows of other kinds of bands (prefix passes, dense blocks) are never marked and count as outside readers.
  // Used by enqueue_level for S2 only, and only with S1 fused (the flags' rows are never written otherwise).
  // per slot: the component (group) it belongs to when its band is a sparse-own component band that touches its rows
  // first (no prefix pass, no carried prefix, no dense blocks); -1 otherwise
  static std::vector<int32_t> first_touch_component(const BandPlan &P, int64_t m) {
    std::vector<int32_t> comp((size_t)m, -1);
    if (!P.cd_sparse) return comp;
    for (int64_t b = 0; b < P.nbands(); ++b) {
      if (P.band_cd.empty() || !P.band_cd[(size_t)b]) continue;
      if (!P.band_dense.empty() && P.band_dense[(size_t)b]) continue;
      if (!P.band_prefix.empty() && P.band_prefix[(size_t)b]) continue;
      if (!P.band_fused.empty() && P.band_fused[(size_t)b]) continue;
      for (int32_t g = P.wg_grp_ptr[(size_t)P.band_wg_ptr[(size_t)b]]; g < P.wg_grp_ptr[(size_t)P.band_wg_ptr[(size_t)b + 1]]; ++g)
        for (int32_t sl = P.grp_slot_ptr[(size_t)g]; sl < P.grp_slot_ptr[(size_t)g + 1]; ++sl) comp[(size_t)sl] = g;
    }
    return comp;
  }
  void build_row_flags(const HostLevel<T> &H, DevLevel &L) {
    const int64_t m = H.m;
    if (m <= 0 || H.n <= m || L.top_n > 0 || !L.L.cd_sparse || !L.U.cd_sparse) return;
    if ((int64_t)H.Lr.rowid.size() != m || (int64_t)H.Ur.rowid.size() != m || H.Lp.srcslot.size() != H.Lr.col.size() ||
        H.Up.srcslot.size() != H.Ur.col.size())
      return;
    const std::vector<int32_t> compL = first_touch_component(H.Lp, m), compU = first_touch_component(H.Up, m);
    // slots whose value a row OUTSIDE their own component reads from memory (rows of other kinds of bands: every entry)
    auto outside_sources = [&](const Csr<T> &A, const BandPlan &P, const std::vector<int32_t> &comp) {
      std::vector<uint8_t> used((size_t)m, 0);
      for (int64_t t = 0; t < m; ++t)
        for (int32_t k = A.ptr[(size_t)t]; k < A.ptr[(size_t)t + 1]; ++k) {
          const int32_t src = P.srcslot[(size_t)k];
          if (comp[(size_t)t] < 0 || comp[(size_t)src] != comp[(size_t)t]) used[(size_t)src] = 1;
        }
      return used;
    };
    const std::vector<uint8_t> usedL = outside_sources(H.Lr, H.Lp, compL), usedU = outside_sources(H.Ur, H.Up, compU);
    std::vector<uint8_t> ecol((size_t)m, 0);
    for (int32_t c : H.Er.col) ecol[(size_t)c] = 1;
    std::vector<int32_t> uslot((size_t)m, -1);  // row -> U slot
    for (int64_t sl = 0; sl < m; ++sl) uslot[(size_t)H.Ur.rowid[(size_t)sl]] = (int32_t)sl;
    std::vector<uint8_t> fL((size_t)m, 0), fU((size_t)m, 0);
    int64_t nred = 0, nskip = 0;
    for (int64_t sl = 0; sl < m && (opt.skip_rows & 1); ++sl) {
      if (compL[(size_t)sl] < 0 || usedL[(size_t)sl] || H.Lr.ptr[(size_t)sl + 1] != H.Lr.ptr[(size_t)sl]) continue;
      const int32_t us = uslot[(size_t)H.Lr.rowid[(size_t)sl]];
      if (us < 0 || compU[(size_t)us] < 0) continue;  // (the U kernel that touches the row first must know where to look)
      fL[(size_t)sl] = 1;
      fU[(size_t)us] |= 2;
      ++nred;
    }
    for (int64_t sl = 0; sl < m && (opt.skip_rows & 2); ++sl)
      if (compU[(size_t)sl] >= 0 && !usedU[(size_t)sl] && !ecol[(size_t)H.Ur.rowid[(size_t)sl]]) {
        fU[(size_t)sl] |= 1;
        ++nskip;
      }
    if (nred + nskip == 0) return;
    L.L.rowflag.upload(fL, 8);
    L.U.rowflag.upload(fU, 8);
    L.skip_w = nred;
    L.skip_v = nskip;
  }
  // Block inverses of a triangle -- the 2,048-row blocks of its dense chains and the components of its
  // component-dense bands: built into two pinned staging buffers (reused, so the host never holds more than two
  // buffers full) and streamed to HBM while the next batch is being inverted.  Consecutive small blocks share a
  // batch (built in parallel, one thread per block, ONE copy); a big block is a batch of its own (parallel inside).
  // A band whose inverses grow beyond dense_max_growth reverts to the sequential (flag) scheme.
  // NOTE (analysis trailer): a band whose inverses grow beyond dense_max_growth loses its dense / component flag HERE, on the
  // host plan, and save_analysis (which runs after finalize) writes those value-dependent verdicts into the trailer; a
  // load with OTHER values of the same pattern keeps such a band on the flag scheme (still correct, never checked against
  // growth again in the other direction: a band that is flagged and grows under the new values is demoted as usual).
  void ship_block_inverses(BandPlan &P, const Csr<T> &A, int64_t total_elems, DevCsr &M) {
    M.upload(A, &P);
    if (opt.ct_mode && (sizeof(T) == sizeof(double) ? opt.ct_mode_real : opt.ct_mode_z) && opt.band.dense_block > 0 && !P.cd_sparse && !P.band_cd.empty()) {
      // dense-own component bands: the entries a component reads from older rows as 16 x 4 coefficient tiles (k_band_ct)
      CtTiles Tl;
      build_ct_tiles(P, A, Tl);
      if (Tl.ntiles > 0 || !Tl.desc.empty()) {
        M.ct_desc.upload(Tl.desc);
        M.ct_sptr.upload(Tl.sptr, 8);
        M.ct_src.upload(Tl.src, 64);
        M.ct_coef.upload(Tl.coef, 512);
        M.ct_on = true;
        M.ct_tiles = Tl.ntiles;
        M.band_wave_tiles = Tl.band_wave_tiles;
      }
    }
    if (!total_elems) return;
    M.tinv.alloc((size_t)total_elems * sizeof(double));
    const bool cplx = sizeof(T) != sizeof(double);
    auto elems_of = [&](size_t q) { return dense_block_elems(P.blk_slot1[q] - P.blk_slot0[q], cplx); };
    int64_t biggest = dense_block_elems(std::max<int64_t>(opt.band.dense_block, 32), cplx);
    for (size_t q = 0; q < P.blk_slot0.size(); ++q) biggest = std::max(biggest, elems_of(q));
    const size_t cap = (size_t)biggest * sizeof(double);
    if (!opt.device_inverses && (!pin[0] || pin_cap < cap)) {
      for (int k = 0; k < 2; ++k) {
        if (pin[k]) (void)hipHostFree(pin[k]);
        HIP_OK(hipHostMalloc((void **)&pin[k], cap, hipHostMallocDefault));
        if (!pin_done[k]) HIP_OK(hipEventCreateWithFlags(&pin_done[k], hipEventDisableTiming));
      }
      pin_cap = cap;
    }
    std::vector<uint8_t> bad(P.blk_slot0.size(), 0);
    const size_t nblk = P.blk_slot0.size();
    if (opt.device_inverses && nblk) {
      // on the device (kernels.hip.hpp k_block_inverse): the factors are there already, the operators never cross PCIe
      DevBuf d0, d1, doff, dg;
      std::vector<int64_t> off64(P.blk_inv_off.begin(), P.blk_inv_off.end());
      d0.upload(P.blk_slot0), d1.upload(P.blk_slot1), doff.upload(off64);
      dg.alloc(nblk * sizeof(unsigned long long));
      HIP_OK(hipMemsetAsync(dg.p, 0, dg.bytes, stream));
      HIP_OK(hipMemsetAsync(M.tinv.p, 0, M.tinv.bytes, stream));
      int32_t rows_max = 1;
      for (size_t q = 0; q < nblk; ++q) rows_max = std::max(rows_max, P.blk_slot1[q] - P.blk_slot0[q]);
      const unsigned gy = (unsigned)((rows_max + 255) / 256);
      for (size_t q0 = 0; q0 < nblk; q0 += 1u << 20) {  // (grid.x in slices of 2^20 blocks)
        const unsigned gx = (unsigned)std::min<size_t>(nblk - q0, 1u << 20);
        hipLaunchKernelGGL((k_block_inverse<D>), dim3(gx, gy), dim3(256), 0, stream, d0.as<int32_t>() + q0, d1.as<int32_t>() + q0,
                           doff.as<int64_t>() + q0, M.ptr.as<int32_t>(), M.srcslot.as<int32_t>(), M.val.as<D>(), M.tinv.as<double>(),
                           dg.as<unsigned long long>() + q0);
      }
      HIP_OK(hipGetLastError());
      const unsigned long long *gbits = read_back<unsigned long long>(dg.p, nblk);
      for (size_t q = 0; q < nblk; ++q) {
        double g;
        std::memcpy(&g, &gbits[q], 8);
        if (!(g <= opt.band.dense_max_growth)) bad[q] = 1;
      }
    }
    for (size_t q0 = opt.device_inverses ? nblk : 0; q0 < nblk;) {
      size_t q1 = q0 + 1;
      int64_t batch = elems_of(q0);
      while (q1 < nblk && batch + elems_of(q1) <= biggest && P.blk_inv_off[q1] == P.blk_inv_off[q0] + batch) batch += elems_of(q1++);
      const int which = (int)(pin_next++ & 1);
      HIP_OK(hipEventSynchronize(pin_done[which]));  // the copy that last used this buffer has finished
      double *buf = pin[which];
      if (q1 - q0 == 1) {
        if (!(build_dense_block(P, A, q0, buf) <= opt.band.dense_max_growth)) bad[q0] = 1;
      } else {
        parallel_for((int64_t)(q1 - q0), 1, [&](int64_t i0, int64_t i1) {
          for (int64_t i = i0; i < i1; ++i) {
            const size_t q = q0 + (size_t)i;
            if (!(build_dense_block(P, A, q, buf + (P.blk_inv_off[q] - P.blk_inv_off[q0]), true) <= opt.band.dense_max_growth)) bad[q] = 1;
          }
        });
      }
      HIP_OK(hipMemcpyAsync(M.tinv.as<double>() + P.blk_inv_off[q0], buf, (size_t)batch * sizeof(double), hipMemcpyHostToDevice,
                            stream));
      HIP_OK(hipEventRecord(pin_done[which], stream));
      q0 = q1;
    }
    bool any_bad = false;
    for (int64_t b = 0; b < P.nbands(); ++b)
      for (int32_t q = P.band_blk_ptr[(size_t)b]; q < P.band_blk_ptr[(size_t)b + 1]; ++q)
        if (bad[(size_t)q]) P.band_dense[(size_t)b] = 0, P.band_cd[(size_t)b] = 0, any_bad = true;
    if (any_bad) {  // (launch_trsv walks the band table of the device copy)
      M.band_dense = P.band_dense;
      M.band_cd = P.band_cd;
    }
  }
  size_t pin_cap = 0;
  int64_t top_rows_max = 0;  // rows of the largest combined top operator (sizes blk_tmp)
  double *pin[2] = {nullptr, nullptr};
  hipEvent_t pin_done[2] = {nullptr, nullptr};
  uint64_t pin_next = 0;

  void finalize(int64_t max_nrhs_) {
    if (finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy already finalized");
    if (host.levels.empty()) throw Error(HIFAMD_BAD_PREC, "empty hierarchy");
    const auto &last = host.levels.back();
    if (last.n != last.m && !host.has_dense)
      throw Error(HIFAMD_BAD_PREC, "last level has a Schur complement but no dense block was set");
    const auto t_fin0 = std::chrono::steady_clock::now();
    if (max_nrhs_ < 1) max_nrhs_ = 1;
    max_nrhs = max_nrhs_;
    Rmax = 1;
    while (Rmax < max_nrhs && Rmax < 64) Rmax <<= 1;
    Rmax = std::max<int64_t>(Rmax, 1LL << opt.min_logR);
    // every array the kernels index with is re-validated right before it is shipped (import.hpp): a host copy that
    // is not what the conversion must have produced is refused here instead of hanging or mis-solving on the device
    // (development aid, HIFIR_AMD_FINALIZE_DUMP=1: seconds per piece of the set-up on stderr)
    const bool fdump = env_int("HIFIR_AMD_FINALIZE_DUMP", 0) != 0;
    auto fnow = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double ft = fnow();
    auto tick = [&](const char *what, size_t level) {
      if (!fdump) return;
      (void)hipDeviceSynchronize();
      const double t = fnow();
      std::fprintf(stderr, "FINALIZE level=%zu %-28s %.3f s\n", level, what, t - ft);
      ft = t;
    };
    for (size_t l = 0; l < host.levels.size(); ++l) host_repairs += verify_level(host.levels[l], l, adjoint);
    for (size_t l = 0; l < host.levels.size(); ++l) check_level_invariants(host.levels[l], l, adjoint, &opt.band);
    tick("invariants (all levels)", 0);
    bind_device();
    tick("bind device", 0);
    for (auto &H : host.levels) {
      const size_t fl_ = lv.size();
      std::unique_ptr<DevLevel> Lp(new DevLevel());
      DevLevel &L = *Lp;
      L.m = H.m;
      L.n = H.n;
      L.F_ncols = H.F_ncols;
      L.E_void = H.E_void;
      // sparse-own L bands: the one per-row order of the own entries that k_band_ls, k_band_cd and k_band_cs share (host.hpp
      // ls_reorder_own) -- before the lists are shipped, whatever HIFIR_AMD_LS says and whatever analyzed the level
      if constexpr (std::is_same<T, double>::value) {
        if (opt.band.dense_block > 0 && H.Lp.cd_sparse) ls_reorder_own(H.Lp);
      }
      ship_block_inverses(H.Lp, H.Lr, H.Ltinv_elems, L.L);
      ship_block_inverses(H.Up, H.Ur, H.Utinv_elems, L.U);
      tick("triangles + block inverses", fl_);
      if (H.top_n > 0 && H.Lp.band_dense[(size_t)H.top_bandL] && H.Up.band_dense[(size_t)H.top_bandU]) {
        // (a top band whose block inverses grew too much has lost its dense flag: then the bands run one by one)
        const int32_t r0L = H.Lp.grp_slot_ptr[(size_t)H.Lp.wg_grp_ptr[(size_t)H.Lp.band_wg_ptr[(size_t)H.top_bandL]]];
        const int32_t r0U = H.Up.grp_slot_ptr[(size_t)H.Up.wg_grp_ptr[(size_t)H.Up.band_wg_ptr[(size_t)H.top_bandU]]];
        std::vector<T> G;
        const double growth = build_top_operator(H.Lr, H.Lp, r0L, H.Ur, H.Up, r0U, H.top_n, H.d, G);
        if (growth <= opt.band.dense_max_growth) {
          L.topG.upload(mfma_operand(G.data(), H.top_n, H.top_n, round_up32(H.top_n)), 4096);  // (k zero-padded to 32; k_top_gemm reads past the end)
          L.top_n = H.top_n;
          L.top_bandL = H.top_bandL;
          L.top_bandU = H.top_bandU;
          top_rows_max = std::max(top_rows_max, H.top_n);
        }
      }
      tick("combined top operator", fl_);
      L.E.upload(H.Er, nullptr);
      L.F.upload(H.Fr, nullptr);
      if (opt.spmm_tiles && opt.band.dense_block > 0 && (sizeof(T) == sizeof(double) || opt.spmm_tiles_z))  // fast mode
        for (int which = 0; which < 2; ++which) {
          const Csr<T> &Ah = which ? H.Fr : H.Er;
          DevCsr &Md = which ? L.F : L.E;
          if (Ah.nrows < 64 || Ah.col.size() < 8 * (size_t)Ah.nrows) continue;  // (sparse rows share too little)
          SpmmTiles Tl = build_spmm_tiles(Ah, opt.spmm_rb);
          if (Tl.reuse < spmm_tile_reuse) continue;
          Md.tl_rb = Tl.rb;
          Md.tl_gptr.upload(Tl.blk_gptr);
          Md.tl_ucol.upload(Tl.ucol);
          Md.tl_coef.upload(Tl.coef);
          Md.tl_nblk = Tl.nblk;
        }
      tick("E / F + product tiles", fl_);
      // S5 fused into the second L solve (host.hpp build_cd_streams_fused): thin F rows only -- rows that share columns
      // are better served by the tiled product
      if constexpr (std::is_same<T, double>::value) {
        if (opt.fuse_f && opt.fuse_gather && opt.band_pipe && Rmax == 64 && opt.band.dense_block > 0 && H.F_ncols > 0 && H.m > 0 &&
            L.top_n == 0 && L.F.tl_nblk == 0 && cd_f_fusable(H.Lp)) {
          CdFusedStreams<T> S;
          if (build_cd_streams_fused(H.Lp, H.Lr, H.Fr, H.n + H.m, S)) {
            L.L.f_desc.upload(S.desc);
            L.L.f_col.upload(S.col, 80);
            L.L.f_val.upload(S.val, 80);
            L.L.f_lrow.upload(S.lrow, 80);
            L.L.f_fused = true;
          }
        }
      }
      {
        // S7 fused into the last U band (LastU): that band must be a component band (its kernel knows how) and the level
        // must have come with q (hifamd_add_level: optional).  Complex handles (round 4): the slice kernel k_band_cs_z
        // knows how -- enqueue_level asks s7_kernel_ok() whether this launch's last U band runs through it
        const BandPlan &Up = H.Up;
        const int64_t nbU = Up.nbands();
        if (opt.fuse_out && Rmax == 64 && H.m > 0 && nbU > 0 && !Up.band_cd.empty() && Up.band_cd[(size_t)nbU - 1] &&
            !(L.top_n > 0 && L.top_bandU == nbU - 1) && (int64_t)H.q.size() == H.n) {
          std::vector<uint8_t> covered((size_t)H.n, 0);
          const int32_t s0 = Up.grp_slot_ptr[(size_t)Up.wg_grp_ptr[(size_t)Up.band_wg_ptr[(size_t)nbU - 1]]];
          const int32_t s1 = Up.grp_slot_ptr[(size_t)Up.wg_grp_ptr[(size_t)Up.band_wg_ptr[(size_t)nbU]]];
          for (int32_t sl = s0; sl < s1; ++sl) covered[(size_t)H.Ur.rowid[(size_t)sl]] = 1;
          std::vector<int32_t> list;  // (the child's rows first: they can go out while this level's second solve runs)
          for (int64_t i = 0; i < H.n; ++i)
            if (H.q_inv[(size_t)i] >= H.m) list.push_back((int32_t)i);
          L.s7_child = (int64_t)list.size();
          for (int64_t i = 0; i < H.n; ++i)
            if (H.q_inv[(size_t)i] < H.m && !covered[(size_t)H.q_inv[(size_t)i]]) list.push_back((int32_t)i);
          L.q_s7.upload(H.q);
          L.s7_list.upload(list, 8);
          L.s7_n = (int64_t)list.size();
        }
      }
      if constexpr (std::is_same<T, double>::value) {
        if (opt.skip_rows && opt.band.dense_block > 0) build_row_flags(H, L);
        if (opt.us_mode && opt.band.dense_block > 0 && L.U.cd_sparse && Rmax == 64) {
          UsPlan<T> Up2;
          build_us_plan(H.Up, H.Ur, Up2);
          if (Up2.any) check_us_plan(H.Up, H.Ur, Up2);
          if (Up2.any) {
            DevCsr &M = L.U;
            M.us_desc.upload(Up2.desc, 8), M.us_rowid.upload(Up2.rowid, 8), M.us_oslot.upload(Up2.oslot, 8), M.us_mptr.upload(Up2.mptr, 8);
            M.us_mcol.upload(Up2.mcol, 8), M.us_mval.upload(Up2.mval, 8), M.us_own_val.upload(Up2.own_val, 8);
            M.us_own_src.upload(Up2.own_src, 8), M.us_own_rptr.upload(Up2.own_rptr, 8), M.us_own_lvl.upload(Up2.own_lvl, 8);
            M.us_band_ok = Up2.band_ok, M.us_band_nbk = Up2.band_nbk, M.us_band_own = Up2.band_own, M.us_band_c0 = Up2.band_c0;
          }
        }
      }
      if constexpr (std::is_same<T, double>::value) {
        if (opt.ls_mode && opt.band.dense_block > 0 && L.L.cd_sparse && Rmax == 64) {
          LsPlan<T> Lp2;
          build_ls_plan(H.Lp, H.Lr, L.L.f_fused ? &H.Fr : nullptr, H.n + H.m, opt.ls_chunk, Lp2);
          if (Lp2.any) check_ls_plan(H.Lp, H.Lr, Lp2, 2 * H.n);  // (the arena: w, v behind it)
          if (Lp2.any) {
            DevCsr &M = L.L;
            M.ls_desc.upload(Lp2.desc, 8), M.ls_rowid.upload(Lp2.rowid, 8), M.ls_oslot.upload(Lp2.oslot, 8);
            M.ls_own_val.upload(Lp2.own_val, 8), M.ls_own_src.upload(Lp2.own_src, 8), M.ls_own_rptr.upload(Lp2.own_rptr, 8);
            M.ls_own_lvl.upload(Lp2.own_lvl, 8);
            for (int f = 0; f < 2; ++f) {
              const LsStream<T> &E = f ? Lp2.fused : Lp2.plain;
              if (!E.on) continue;
              M.ls_ebase[f].upload(E.base, 8), M.ls_ewptr[f].upload(E.wptr, 8);
              M.ls_ecol[f].upload(E.col, 80), M.ls_eval[f].upload(E.val, 80), M.ls_etag[f].upload(E.tag, 80);
            }
            M.ls_fused = Lp2.fused.on;
            M.ls_band_ok = Lp2.band_ok, M.ls_band_nd = Lp2.band_nd, M.ls_band_own = Lp2.band_own, M.ls_band_rptr = Lp2.band_rptr;
            M.ls_band_c0 = Lp2.band_c0, M.ls_band_cw = Lp2.band_cw, M.ls_band_nch = Lp2.band_nch;
            M.ls_sources = Lp2.sources, M.ls_deps = Lp2.deps, M.ls_chunk_rows = Lp2.chunk_rows;
          }
        }
      }
      L.d.upload(H.d);
      L.s.upload(H.s);
      L.t.upload(H.t);
      L.p.upload(H.p);
      L.qinv.upload(H.q_inv);
      L.alloc_arena((size_t)H.n * Rmax * sizeof(T));
      zero_dev(L.w.p, L.w.bytes);
      zero_dev(L.v.p, L.v.bytes);
      tick("fused streams, vectors, arena", fl_);

      lv.push_back(std::move(Lp));
    }
    if (host.has_dense && host.dense.kind == 2) {
      dn.n = host.dense.n;
      dn.rank = host.dense.rank;
      dn.lup = true;
      dn.QH.upload(mfma_operand(host.dense.QH.data(), dn.n, dn.n));
      std::vector<T>().swap(host.dense.QH);
      std::vector<T>().swap(host.dense.SymMul);
    } else if (host.has_dense && host.dense.kind == 1) {
      dn.n = host.dense.n;
      dn.rank = host.dense.rank;
      dn.symm = true;
      dn.QH.upload(mfma_operand(host.dense.QH.data(), dn.n, dn.n));
      dn.Qm.upload(mfma_operand(host.dense.Q.data(), dn.n, dn.n));
      dn.tmp.alloc((size_t)dn.n * Rmax * sizeof(T));
      std::vector<T>().swap(host.dense.QH);
      std::vector<T>().swap(host.dense.Q);
      std::vector<T>().swap(host.dense.SymMul);
    } else if (host.has_dense) {
      dn.n = host.dense.n;
      dn.rank = host.dense.rank;
      if (!adjoint) {  // MFMA operands (complex: two real planes each)
        dn.QH.upload(mfma_operand(host.dense.QH.data(), dn.n, dn.n));
        dn.Rinv.upload(mfma_operand(host.dense.Rinv.data(), dn.n, dn.n));
      }
      dn.jpvt0.upload(host.dense.jpvt0);
      dn.tmp.alloc((size_t)dn.n * Rmax * sizeof(T));
      if (adjoint) {
        dn.Qm.upload(mfma_operand(host.dense.Q.data(), dn.n, dn.n));
        dn.RinvH.upload(mfma_operand(host.dense.RinvH.data(), dn.n, dn.n));
        dn.tmp2.alloc((size_t)dn.n * Rmax * sizeof(T));
        std::vector<T>().swap(host.dense.Q);
        std::vector<T>().swap(host.dense.RinvH);
      }
      // the explicit operators are only needed on the device from here on
      std::vector<T>().swap(host.dense.QH);
      std::vector<T>().swap(host.dense.Rinv);
    }
    errflag.alloc(sizeof(unsigned));
    zero_dev(errflag.p, errflag.bytes);
#ifdef HIFAMD_CSPROBE
    if (getenv("HIFIR_AMD_CSPROBE_OUT") && !adjoint && !is_twin) {  // 12 words per workgroup
      const unsigned cap = 400000;
      csprobe.alloc((size_t)cap * 12 * 8);
      zero_dev(csprobe.p, csprobe.bytes);
      unsigned long long *pp = csprobe.as<unsigned long long>();
      HIP_OK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_csprobe), &pp, sizeof(pp), 0, hipMemcpyHostToDevice, xfer_stream()));
      HIP_OK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_csprobe_cap), &cap, sizeof(cap), 0, hipMemcpyHostToDevice, xfer_stream()));
      HIP_OK(hipStreamSynchronize(xfer_stream()));
    }
#endif
#ifdef HIFAMD_PROBE
    if (getenv("HIFIR_AMD_PROBE_OUT")) {  // 600 launches x 256 workgroups x 16 waves x 16 words
      probe.alloc((size_t)600 * 256 * 16 * 16 * 8);
      zero_dev(probe.p, probe.bytes);
    }
#endif
    if (sizeof(T) != sizeof(double)) {
      const size_t rows = (size_t)std::max<int64_t>(opt.band.dense_block + 32, host.has_dense ? host.dense.n + 32 : 0);
      zt1.alloc(rows * (size_t)Rmax * 2 * sizeof(double));
      zt2.alloc(rows * (size_t)Rmax * 2 * sizeof(double));
    }
    {
      const int remap = opt.xcd_remap;
      HIP_OK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_xcd_remap), &remap, sizeof(int), 0, hipMemcpyHostToDevice, xfer_stream()));
      HIP_OK(hipStreamSynchronize(xfer_stream()));
    }
    if (top_rows_max > 0) gemm_part.alloc((size_t)kTopGemmSplits * (size_t)((top_rows_max + 63) / 64 * 64) * 64 * sizeof(T));  // (complex: partial tiles of 128 doubles a row)
    gemm_cnt.alloc(kTopGemmTilesMax * sizeof(unsigned));  // (tops and tails have at most top_max / tail_rows <= 64 x this many rows)
    zero_dev(gemm_cnt.p, gemm_cnt.bytes);
    if (opt.band.dense_block > 0) {  // +32 rows: the MFMA kernel reads whole 32-k operand sets (masked)
      blk_tmp.alloc((size_t)(std::max<int64_t>(opt.band.dense_block, top_rows_max) + 32) * Rmax * sizeof(T));
      zero_dev(blk_tmp.p, blk_tmp.bytes);
    }
    HIP_OK(hipStreamSynchronize(stream));  // (transfers were synchronous on the transfer stream)
    for (int k = 0; k < 2; ++k) {  // the staging buffers of the block inverses are not needed any more
      if (pin[k]) (void)hipHostFree(pin[k]);
      if (pin_done[k]) (void)hipEventDestroy(pin_done[k]);
      pin[k] = nullptr;
      pin_done[k] = nullptr;
    }
    pin_cap = 0;
    for (const auto &Lp : lv) {
      bytes_inverses += (double)Lp->L.tinv.bytes + (double)Lp->U.tinv.bytes;
      bytes_top += (double)Lp->topG.bytes;
    }
    // The tail operator is an optimisation: whatever goes wrong while it is formed (allocation, a device error of
    // its own applies) leaves the handle with the recursion -- and the handle is marked finalized only afterwards.
    tick("dense block, buffers", lv.size());
    try {
      build_tail_operator();
      tick("tail operator", lv.size());
    } catch (const std::exception &) {
      (void)hipGetLastError();
      tailG.release();
      tail_level = -1;
      tail_n = 0;
      tail_rejected = 4;
    }
    bytes_tail = (double)tailG.bytes;
    finalized = true;
    finalize_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_fin0).count();
  }

  void build_tail_operator() {
    // (complex handles: on request only -- hifamd_set_complex_operators, HIFAMD_ZOP_TAIL)
    if (!std::is_same<T, double>::value && !(opt.zop_flags & 1)) return;
    if (opt.tail_rows <= 0 || opt.band.dense_block <= 0 || Rmax != 64 || lv.size() < 2) return;
    size_t l0 = 0;
    for (size_t l = 1; l < lv.size(); ++l)
      if (lv[l]->n <= opt.tail_rows) {
        l0 = l;
        break;
      }
    if (!l0) return;
    const int64_t n = lv[l0]->n, ld = round_up32(n);
    DevBuf I, O;
    I.alloc((size_t)(n + 32) * 64 * sizeof(T));
    O.alloc((size_t)(n + 32) * 64 * sizeof(T));
    std::vector<T> hI((size_t)n * 64), hO((size_t)n * 64), G((size_t)(n * n), T(0));
    for (int64_t j0 = 0; j0 < n; j0 += 64) {
      const int64_t jw = std::min<int64_t>(64, n - j0);
      std::fill(hI.begin(), hI.end(), T(0));
      for (int64_t c = 0; c < jw; ++c) hI[(size_t)((j0 + c) * 64 + c)] = T(1);
      copy_h2d(I.p, hI.data(), hI.size() * sizeof(T));
      int64_t cnt = 0;
      enqueue_level(stream, l0, in_direct(I.as<D>()), 64, out_direct(O.as<D>()), 64, 64, 6, 0, cnt);
      HIP_OK(hipStreamSynchronize(stream));
      copy_d2h(hO.data(), O.p, hO.size() * sizeof(T));
      for (int64_t c = 0; c < jw; ++c)
        for (int64_t i = 0; i < n; ++i) G[(size_t)(i + (j0 + c) * n)] = hO[(size_t)(i * 64 + c)];
    }
    check_device_error();
    // Guards (every other explicit operator has one: block inverses and top operators fall back to substitution when
    // their entries grow beyond dense_max_growth).  G = M_tail^{-1} bakes the sparse levels below l0 AND the (possibly
    // rank-truncated) dense block into one matrix:
    //  (1) every entry finite (a singular tail: keep the recursion, which reports what it finds);
    //  (2) max |G| <= tail_max_growth: the product G c then loses at most that factor against the data;
    //  (3) a probe: G c against the recursion on a fixed pseudo-random block c (complex handles: real and imaginary
    //      parts drawn in turn), relative difference (max norm, all 64 columns) <= tail_probe_tol -- an ill-conditioned
    //      tail, where the two roads differ by kappa eps, keeps the recursion, i.e. the road the oracle comparison is
    //      stated for.
    const double *Gd = reinterpret_cast<const double *>(G.data());  // (complex: both parts must be finite)
    for (size_t i = 0; i < G.size() * (sizeof(T) / sizeof(double)); ++i)
      if (!std::isfinite(Gd[i])) {
        tail_rejected = 1;
        return;
      }
    double gmax = 0.0;
    for (const T &g : G) gmax = std::max(gmax, (double)std::abs(g));
    tail_max_abs = gmax;
    if (gmax > opt.tail_max_growth) {
      tail_rejected = 2;
      return;
    }
    tailG.upload(mfma_operand(G.data(), n, n, ld), 4096);
    if (gemm_part.bytes < (size_t)kTopGemmSplits * (size_t)((n + 63) / 64 * 64) * 64 * sizeof(T)) {
      HIP_OK(hipStreamSynchronize(stream));
      gemm_part.alloc((size_t)kTopGemmSplits * (size_t)((n + 63) / 64 * 64) * 64 * sizeof(T));
    }
    {
      uint64_t rs = 0x9E3779B97F4A7C15ull;
      double *hId = reinterpret_cast<double *>(hI.data());
      for (size_t i = 0; i < hI.size() * (sizeof(T) / sizeof(double)); ++i) {
        rs = rs * 6364136223846793005ull + 1442695040888963407ull;
        hId[i] = (double)(int64_t)(rs >> 11) / 9007199254740992.0 * 2.0 - 1.0;
      }
      copy_h2d(I.p, hI.data(), hI.size() * sizeof(T));
      int64_t cnt = 0;
      enqueue_level(stream, l0, in_direct(I.as<D>()), 64, out_direct(O.as<D>()), 64, 64, 6, 0, cnt);  // the recursion
      HIP_OK(hipStreamSynchronize(stream));
      copy_d2h(hO.data(), O.p, hO.size() * sizeof(T));
      std::vector<T> hP((size_t)n * 64);
      tail_n = n;  // (launch_tail reads it)
      launch_tail(stream, I.as<D>(), O.as<D>(), cnt);  // the product
      HIP_OK(hipStreamSynchronize(stream));
      copy_d2h(hP.data(), O.p, hP.size() * sizeof(T));
      tail_n = 0;
      check_device_error();
      double num = 0.0, den = 0.0;
      for (size_t i = 0; i < hP.size(); ++i) {
        num = std::max(num, (double)std::abs(hP[i] - hO[i]));
        den = std::max(den, (double)std::abs(hO[i]));
      }
      tail_probe_err = den > 0.0 ? num / den : num;
      if (!(tail_probe_err <= opt.tail_probe_tol)) {
        tailG.release();
        tail_rejected = 3;
        return;
      }
    }
    tail_level = (int64_t)l0;
    tail_n = n;
  }

  // the sticky error word of the band kernels (a bounded spin expired); checked at sync points
  void check_device_error() {
    if (adj) adj->check_device_error();
    for (auto &tw : twins) tw->check_device_error();
    unsigned e = 0;
    copy_d2h(&e, errflag.p, sizeof(e));
    if (e) {
      zero_dev(errflag.p, sizeof(e));
      throw Error(HIFAMD_HIFIR_ERROR, "a triangular-solve workgroup timed out waiting for a dependency (device fault)");
    }
  }

  // the checks of hifamd_set_matrix / hifamd_set_mass_matrix on a user's CRS arrays (0- or 1-based), and its 0-based copy
  Csr<T> crs_from_user(int64_t n, const int64_t *indptr, const int32_t *indices, const T *vals) const {
    if (!indptr || !indices || !vals) throw Error(HIFAMD_NULL_OBJ, "NULL CRS array");
    if (!host.levels.empty() && n != host.levels[0].n)
      throw Error(HIFAMD_MISMATCHED_SIZES, "matrix size differs from the preconditioner size");
    const int64_t base = indptr[0];
    if (base != 0 && base != 1) throw Error(HIFAMD_MISMATCHED_SIZES, "indptr must be 0- or 1-based");
    const int64_t nz = indptr[n] - base;
    if (nz > (int64_t)std::numeric_limits<int32_t>::max()) throw Error(HIFAMD_HIFIR_ERROR, "nnz(A) >= 2^31");
    Csr<T> C;
    C.nrows = C.ncols = n;
    C.ptr.resize((size_t)n + 1);
    for (int64_t i = 0; i <= n; ++i) C.ptr[(size_t)i] = (int32_t)(indptr[i] - base);
    C.col.resize((size_t)nz);
    for (int64_t k = 0; k < nz; ++k) {
      const int64_t j = (int64_t)indices[k] - base;
      if (j < 0 || j >= n) throw Error(HIFAMD_MISMATCHED_SIZES, "column index out of range");
      C.col[(size_t)k] = (int32_t)j;
    }
    C.val.assign(vals, vals + nz);
    if (!finalized) throw Error(HIFAMD_BAD_PREC, "attach the matrix after hifamd_finalize");
    return C;
  }
  void set_matrix(int64_t n, const int64_t *indptr, const int32_t *indices, const T *vals) {
    const Csr<T> C = crs_from_user(n, indptr, indices, vals);
    if (adj) adj->upload_matrix(adjoint_of_csr(C));
    host.A = C;  // kept for the adjoint engine (built on first use)
    host.has_A = true;
    upload_matrix(C);
  }
  // B of the generalized eigenproblem A x = lambda B x (lobpcg_tile<true>): a second CRS matrix of THIS engine only -- the adjoint
  // engine does not get it, hifamd_save does not write it, and like A it is not checked for being Hermitian or definite
  void set_mass_matrix(int64_t n, const int64_t *indptr, const int32_t *indices, const T *vals) {
    const Csr<T> C = crs_from_user(n, indptr, indices, vals);
    HIP_OK(hipSetDevice(device));
    Bm.upload(C, nullptr);
    HIP_OK(hipStreamSynchronize(stream));
    B_norm_inf = crs_norm_inf(C);
    has_B = true;
  }

  static double crs_norm_inf(const Csr<T> &C) {  // largest row sum of |c_ij|; a NaN row sum wins
    double nrm = 0.0;
    for (int64_t i = 0; i < C.nrows; ++i) {
      double s = 0.0;
      for (int32_t k = C.ptr[(size_t)i]; k < C.ptr[(size_t)i + 1]; ++k) s += abs_(C.val[(size_t)k]);
      if (s > nrm || s != s) nrm = s;
    }
    return nrm;
  }
  double A_norm_inf = 0.0;  // largest row sum of |a_ij| of THIS engine's matrix (the adjoint engine: of A^H), for nsp_find
  double B_norm_inf = 0.0;  // the same of the mass matrix
  void upload_matrix(const Csr<T> &C) {
    HIP_OK(hipSetDevice(device));
    A.upload(C, nullptr);
    HIP_OK(hipStreamSynchronize(stream));  // (transfers were synchronous on the transfer stream)
    A_norm_inf = crs_norm_inf(C);
    has_A = true;
  }

  // ---- launch helpers ------------------------------------------------------------------------
  static int log2i(int64_t R) {
    int l = 0;
    while ((1LL << l) < R) ++l;
    return l;
  }
  // Batch width of the arena for nrhs columns.  The R = 64 kernels (one wave per row, software
  // pipeline) are latency-optimised and measured FASTER than the narrow lane mappings even for a
  // single right-hand side on the reference's 1M-row hierarchies (27 vs 96 ms default, 5.8 vs 7.5 ms
  // tuned), so narrow batches are padded up to min_logR (default 6 = always 64 wide).
  int pick_logR(int64_t nrhs) const {
    int64_t R = 1;
    while (R < nrhs && R < 64) R <<= 1;
    return std::max(log2i(R), opt.min_logR);
  }
  static unsigned grid_for(int64_t rows, int logR, int threads = 256) {
    const int64_t G = 64 >> logR, rows_per_block = (threads / 64) * G;
    int64_t g = (rows + rows_per_block - 1) / rows_per_block;
    if (g < 1) g = 1;
    if (g > 256 * 16) g = 256 * 16;  // grid-stride beyond that
    return (unsigned)g;
  }

  // One triangle = its bands in order (host.hpp BandPlan): an optional PREFIX pass on the whole
  // chip, then ONE launch whose workgroups each own whole dependency components of the band.
  typedef FirstL<D> FL;
  static FL no_fl() { return FL{IoPtr<const D>{nullptr, nullptr, 0}, 0, 0, nullptr, nullptr}; }
  typedef LastU<D> LU;
  static LU no_lu() { return LU{IoPtr<D>{nullptr, nullptr, 0}, 0, 0, nullptr, nullptr}; }
  // the band's rows start at split[]: [ptr, split) is folded in by a prefix pass first (its own, or carried by the launch before)
  static bool band_has_prefix(const DevCsr &M, size_t b) { return M.band_prefix[b] || (!M.band_fused.empty() && M.band_fused[b]); }
  // flp != NULL: S1 is fused into this L solve -- whichever kernel touches a row first reads s[p] * b[p] (kernels FirstL)
  template <bool LOWER>
  void launch_trsv(hipStream_t st, const DevLevel &L, int logR, int64_t &count, const FL *flp = nullptr, bool with_f = false,
                   const LU *lup = nullptr, const FL *skip_fl = nullptr) {
    const DevCsr &M = LOWER ? L.L : L.U;
    if (M.nrows == 0) return;
    const FL fl = (LOWER && flp) ? *flp : no_fl();
    D *w = L.w.as<D>(), *v = L.v.as<D>();
    const size_t nb = M.band_wg_ptr.size() - 1;
    const bool top = L.top_n > 0 && logR == 6;  // the level's narrow top is ONE dense product (launch_top)
    bool carried = false;  // the previous band's launch ran this band's carried prefix (host.hpp finish_band_plan)
    for (size_t b = 0; b < nb; ++b) {
      if (top && (int32_t)b == (LOWER ? L.top_bandL : L.top_bandU)) {
        if (LOWER) launch_top(st, L, logR, count, fl);  // (U's top band: already solved by that product)
        carried = false;
        continue;
      }
      const int32_t g0 = M.band_wg_ptr[b], g1 = M.band_wg_ptr[b + 1];
      const bool fused = !M.band_fused.empty() && M.band_fused[b];
      const bool have_carried = carried;
      carried = false;
      // the kernel that touches a U row first starts it from w[i] / d[i] (the L kernels no longer write v).
      // pre: the band's rows start at split[] and [ptr, split) is folded in by a prefix pass first -- its own launch,
      // unless the previous band's launch carried it
      int pre = band_has_prefix(M, b) ? 1 : 0;
      // a component band split into a chip-wide prefix pass over ALL outside sources + the band kernel without its walk
      const bool cd_two = opt.cd_split_min > 0 && logR == 6 && act_cols > 48 && !M.band_cd.empty() && M.band_cd[b] && !M.band_dense[b] &&
                          !M.cd_sparse && !(LOWER && with_f) && b < M.band_chunk_max.size() && M.band_chunk_max[b] >= opt.cd_split_min &&
                          g1 - g0 <= opt.cd_split_wgs && sizeof(T) == sizeof(double);
      if (cd_two) {
        const int64_t s0 = M.band_slot_ptr[b], s1 = M.band_slot_ptr[b + 1];
        const bool touched = fused && have_carried;  // [ptr, split) was folded in (first touch included) by the previous launch
        tally(KF_BAND_SPLIT_PREFIX);
        hipLaunchKernelGGL((k_trsv_wide<D, LOWER, true>), dim3(grid_for(s1 - s0, logR)), dim3(256), 0, st, s0, s1,
                           (touched ? M.split : M.ptr).template as<int32_t>(), M.csplit.as<int32_t>(), M.col.as<int32_t>(), M.val.as<D>(),
                           M.rowid.as<int32_t>(), L.d.as<D>(), w, v, logR, touched ? 0 : 1, (D *)nullptr, 0, touched ? no_fl() : fl);
        ++count;
        pre = 1;  // (the band kernel finds its rows touched)
      }
      // block-dense band at R = 64: the prefix pass delivers the rows of the band's first block straight into the
      // block product's right-hand side (nothing else contributes to them), so that block needs no k_thin_update
      const int32_t qb0 = M.band_dense[b] ? M.band_blk_ptr[b] : -1;
      const bool direct = pre && M.band_dense[b] && logR == 6 && qb0 < M.band_blk_ptr[b + 1] &&
                          M.blk_slot0[(size_t)qb0] == M.band_slot_ptr[b];
      if (pre && !cd_two && !(fused && have_carried)) {  // (a fused band whose predecessor could not carry it: its own launch)
        const int64_t s0 = M.band_slot_ptr[b], s1 = M.band_slot_ptr[b + 1];
        tally(KF_TRSV_WIDE);
        hipLaunchKernelGGL((k_trsv_wide<D, LOWER, true>), dim3(grid_for(s1 - s0, logR)), dim3(256), 0, st, s0, s1,
                           M.ptr.as<int32_t>(), M.split.as<int32_t>(), M.col.as<int32_t>(), M.val.as<D>(),
                           M.rowid.as<int32_t>(), L.d.as<D>(), w, v, logR, 1, direct ? blk_tmp.as<D>() : (D *)nullptr,
                           direct ? M.blk_slot1[(size_t)qb0] : 0, fl);
        ++count;
      }
      if (M.band_dense[b]) {  // block by block: sparse update, then ONE dense product per block
        for (int32_t q = M.band_blk_ptr[b]; q < M.band_blk_ptr[b + 1]; ++q)
          launch_dense_block<LOWER>(st, L, M, q, logR, count, direct && q == qb0);
        continue;
      }
      const bool cdb = !M.band_cd.empty() && M.band_cd[b] && logR == 6;
      if ((logR == 6 && opt.band_pipe) || cdb) {  // the overlapped pipeline (trsv_band_r64); HIFIR_AMD_BAND_PIPE=0: the first version
        // extra workgroups for the carried prefix of the NEXT band (they run on the units this band leaves idle)
        int32_t ps0 = 0, ps1 = 0;
        unsigned extra = 0;
        if (b + 1 < nb && !M.band_fused.empty() && M.band_fused[b + 1]) {
          ps0 = M.band_slot_ptr[b + 1];
          ps1 = M.band_slot_ptr[b + 2];
          extra = (unsigned)std::min<int64_t>(opt.carry_wgs, std::max<int64_t>(1, ((int64_t)ps1 - ps0 + 15) / 16));
          carried = true;
        }
        if (cdb) {
          // (the fused S7 -- LastU -- belongs to the LAST band of the final U solve only)
          // (skip_fl: the level's first solve; the U bands get the level's input for the rows the L bands did not store)
          launch_band_cd<LOWER>(st, L, M, g0, g1, pre, ps0, ps1, extra, (!LOWER && skip_fl) ? *skip_fl : fl, LOWER && with_f,
                                (!LOWER && lup && b + 1 == nb) ? *lup : no_lu(), b, cd_two,
                                RowSkip{skip_fl ? M.rowflag.template as<uint8_t>() : (const uint8_t *)nullptr});
          ++count;
          continue;
        }
        tally(KF_TRSV_BAND_P);
        hipLaunchKernelGGL((k_trsv_band_p<D, LOWER>), dim3((unsigned)(g1 - g0) + extra), dim3(1024), 0, st, g0,
                           M.wg_slot.as<int32_t>(), M.ptr.as<int32_t>(),
                           M.split.as<int32_t>(), M.col.as<int32_t>(), M.val.as<D>(), M.srcslot.as<int32_t>(),
                           M.rowid.as<int32_t>(), L.d.as<D>(), w, v, errflag.as<unsigned>(), pre ? 0 : 1,
                           (int32_t)(g1 - g0), ps0, ps1, fl
#ifdef HIFAMD_PROBE
                           ,
                           probe.as<unsigned long long>(), (int)count
#endif
        );
        ++count;
        continue;
      }
      tally(KF_TRSV_BAND);
      hipLaunchKernelGGL((k_trsv_band<D, LOWER>), dim3((unsigned)(g1 - g0)), dim3(1024), 0, st, g0,
                         M.wg_grp_ptr.as<int32_t>(), M.grp_slot_ptr.as<int32_t>(), M.ptr.as<int32_t>(),
                         M.split.as<int32_t>(), M.col.as<int32_t>(), M.val.as<D>(), M.srcslot.as<int32_t>(),
                         M.rowid.as<int32_t>(), L.d.as<D>(), w, v, logR, errflag.as<unsigned>(), pre ? 0 : 1
#ifdef HIFAMD_PROBE
                         ,
                         probe.as<unsigned long long>(), (int)count
#endif
      );
      ++count;
    }
  }
  // one diagonal block of a block-dense thin band: t = rhs - (everything before the block); then
  // x[rows] = Tinv * t on the matrix cores (LOWER: also v = x / d)
  template <bool LOWER>
  void launch_dense_block(hipStream_t st, const DevLevel &L, const DevCsr &M, int32_t q, int logR, int64_t &count,
                          bool rhs_ready = false) {
    const int32_t r0 = M.blk_slot0[(size_t)q], r1 = M.blk_slot1[(size_t)q], nb = r1 - r0;
    D *x = LOWER ? L.w.as<D>() : L.v.as<D>();
    D *tb = blk_tmp.as<D>();
    if (!rhs_ready) {  // (the first block of a band gets its right-hand side from the prefix pass)
      tally(KF_THIN_UPDATE);
      hipLaunchKernelGGL((k_thin_update<D>), dim3(grid_for(nb, logR)), dim3(256), 0, st, r0, r1, M.ptr.as<int32_t>(),
                         M.split.as<int32_t>(), M.col.as<int32_t>(), M.val.as<D>(), M.srcslot.as<int32_t>(),
                         M.rowid.as<int32_t>(), (const D *)x, tb, logR);
      ++count;
    }
    zgemm_tri(st, nb, M.tinv.as<double>() + M.blk_inv_off[(size_t)q], (const D *)tb, logR, M.rowid.as<int32_t>() + r0, x,
              (const D *)nullptr, (D *)nullptr, count);
  }
  // Out[rowmap] = G X on the matrix cores (kernels.hip.hpp k_top_gemm): 64-row tiles x K splits chosen so that one wave
  // of workgroups fills the chip; the splits' partial tiles are added in order by k_top_reduce
  static constexpr int kTopGemmSplits = 8;
  static constexpr int kTopGemmTilesMax = 4096;  // arrival counters of the last-arriver reduction (rows / 64)
  void launch_top_gemm(hipStream_t st, int nt, const double *G, const double *X, const int32_t *rowmap, double *Out,
                       int64_t &count) {
    const int lda = (int)round_up32(nt);
    const int tiles = (nt + 63) / 64;
    int nks = std::max(1, std::min(kTopGemmSplits, 256 / std::max(1, tiles)));
    int kper = (int)(((int64_t)(lda + nks - 1) / nks + 63) / 64 * 64);
    nks = (lda + kper - 1) / kper;
    const int nct = std::min(4, (act_cols + 15) / 16);
    const int pad = (nt + 63) / 64 * 64;
    if (nks > 1 && gemm_part.bytes < (size_t)nks * pad * 64 * sizeof(double)) {  // (sized at finalize; cannot happen)
      nks = 1;
      kper = (int)((lda + 63) / 64 * 64);
    }
    auto kern = nct == 1 ? k_top_gemm<1> : (nct == 2 ? k_top_gemm<2> : (nct == 3 ? k_top_gemm<3> : k_top_gemm<4>));
    const bool fused_sum = opt.top_last_arriver && nks > 1 && tiles <= kTopGemmTilesMax && gemm_cnt.p;
    tally(KF_TOP_GEMM);
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles, (unsigned)nks), dim3(1024), kTopGemmLds, st, nt, nt, kper, G, lda, X, rowmap,
                       Out, gemm_part.as<double>(), pad, fused_sum ? gemm_cnt.as<unsigned>() : (unsigned *)nullptr);
    ++count;
    if (nks > 1 && !fused_sum) {
      tally(KF_TOP_REDUCE);
      hipLaunchKernelGGL(k_top_reduce, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, st, nt, nks,
                         (const double *)gemm_part.as<double>(), pad, rowmap, Out, nct);
      ++count;
    }
  }
  // the same product of a complex handle (kernels.hip.hpp k_top_gemm_z): X, Out the real views [rows][128] of the complex
  // arrays, G two real planes; tiles and K splits as above -- from nt alone, so that a column's sum order does not depend on
  // the batch -- and a third grid axis of column groups (32 real = 16 complex columns each; the last one may use one tile).
  // The K splits are always added by k_top_reduce_z: there is no last-arriver variant of this kernel
  void launch_top_gemm_z(hipStream_t st, int nt, const double *G, const double *X, const int32_t *rowmap, double *Out,
                         int64_t &count) {
    const int lda = (int)round_up32(nt);
    const int tiles = (nt + 63) / 64;
    int nks = std::max(1, std::min(kTopGemmSplits, 256 / std::max(1, tiles)));
    int kper = (int)(((int64_t)(lda + nks - 1) / nks + 63) / 64 * 64);
    nks = (lda + kper - 1) / kper;
    const int ntiles = std::min(8, (act_cols + 7) / 8);  // 16-real-column tiles (8 complex columns) in use
    const int groups = (ntiles + 1) / 2, nct = ntiles - 2 * (groups - 1);
    const int pad = (nt + 63) / 64 * 64;
    if (nks > 1 && gemm_part.bytes < (size_t)nks * pad * 128 * sizeof(double)) {  // (sized at finalize; cannot happen)
      nks = 1;
      kper = (int)((lda + 63) / 64 * 64);
    }
    tally(KF_TOP_GEMM_Z);
    hipLaunchKernelGGL(nct == 1 ? k_top_gemm_z<1> : k_top_gemm_z<2>, dim3((unsigned)tiles, (unsigned)nks, (unsigned)groups), dim3(1024),
                       kTopGemmLds, st, nt, nt, kper, G, lda, X, rowmap, Out, gemm_part.as<double>(), pad);
    ++count;
    if (nks > 1) {
      tally(KF_TOP_REDUCE_Z);
      hipLaunchKernelGGL(k_top_reduce_z, dim3((unsigned)((nt + 1) / 2)), dim3(256), 0, st, nt, nks,
                         (const double *)gemm_part.as<double>(), pad, rowmap, Out, 16 * ntiles);
      ++count;
    }
  }
  // the level's top rows: t_T = w_T - (sources outside T) by the chip-wide prefix pass, straight into the product's
  // right-hand side; then v_T = G t_T on the matrix cores (G = U_TT^{-1} D_T^{-1} L_TT^{-1}, rows scattered by L's row ids)
  void launch_top(hipStream_t st, const DevLevel &L, int logR, int64_t &count, const FL &fl) {
    if constexpr (!std::is_same<T, double>::value)
      if (!(opt.zop_flags & 2)) throw Error(HIFAMD_HIFIR_ERROR, "internal error: combined top operator on a complex handle that did not ask for it");
    const DevCsr &M = L.L;
    const size_t b = (size_t)L.top_bandL;
    const int64_t s0 = M.band_slot_ptr[b], s1 = M.band_slot_ptr[b + 1];
    tally(KF_TRSV_WIDE);
    hipLaunchKernelGGL((k_trsv_wide<D, true, true>), dim3(grid_for(s1 - s0, logR)), dim3(256), 0, st, s0, s1,
                       M.ptr.as<int32_t>(), M.split.as<int32_t>(), M.col.as<int32_t>(), M.val.as<D>(),
                       M.rowid.as<int32_t>(), L.d.as<D>(), L.w.as<D>(), L.v.as<D>(), logR, 1, blk_tmp.as<D>(), (int32_t)s1,
                       fl);
    ++count;  // (the prefix pass)
    if constexpr (std::is_same<T, double>::value) {
      const int nt = (int)L.top_n;
      const int ktop = (int)round_up32(nt);
      if (opt.top_gemm >= 4) {
        launch_top_gemm(st, nt, L.topG.as<double>(), (const double *)blk_tmp.as<double>(), M.rowid.as<int32_t>() + s0,
                        L.v.as<double>(), count);
        return;
      }
      ++count;
      tally(opt.top_gemm == 1 ? KF_STRIP_GEMM : KF_STRIP_GEMM4);
      if (opt.top_gemm == 1)
        hipLaunchKernelGGL(k_strip_gemm_d<4>, dim3((unsigned)((nt + 15) / 16)), dim3(1024), 0, st, nt, ktop, L.topG.as<double>(), ktop,
                           (const double *)blk_tmp.as<double>(), M.rowid.as<int32_t>() + s0, L.v.as<double>());
      else if (opt.top_gemm == 2)
        hipLaunchKernelGGL(k_strip_gemm4_d<2>, dim3((unsigned)((nt + 15) / 16)), dim3(1024), 0, st, nt, ktop, L.topG.as<double>(), ktop,
                           (const double *)blk_tmp.as<double>(), M.rowid.as<int32_t>() + s0, L.v.as<double>());
      else
        hipLaunchKernelGGL(k_strip_gemm4_d<4>, dim3((unsigned)((nt + 15) / 16)), dim3(1024), 0, st, nt, ktop, L.topG.as<double>(), ktop,
                           (const double *)blk_tmp.as<double>(), M.rowid.as<int32_t>() + s0, L.v.as<double>());
    } else {
      launch_top_gemm_z(st, (int)L.top_n, L.topG.as<double>(), (const double *)blk_tmp.as<double>(), M.rowid.as<int32_t>() + s0,
                        L.v.as<double>(), count);
    }
  }
  // rows the LDS layout of a component band kernel is built for (band_lds.hpp); dense-own plans: rounded up to a multiple
  // of 32 -- the inverse product reads whole operand sets
  int32_t cd_lds_rows(bool sparse) const {
    return (int32_t)(sparse ? opt.band.cd_sparse_rows : ((opt.band.cd_rows + 31) & ~(int64_t)31));
  }
  // v_tail = G c_tail (build_tail_operator); the product reads up to 31 rows behind c_tail: they lie inside the level's
  // arena (v follows w) and meet zero columns of the operand
  bool launch_tail(hipStream_t st, const D *cin, D *zout, int64_t &count) {
    if constexpr (std::is_same<T, double>::value) {
      const int nt = (int)tail_n, kt = (int)round_up32(tail_n);
      if (opt.top_gemm >= 4) {  // (reads exactly the tail_n rows of c_tail: nothing behind them)
        launch_top_gemm(st, nt, tailG.as<double>(), (const double *)cin, nullptr, (double *)zout, count);
        return true;
      }
      ++count;
      tally(KF_STRIP_GEMM4);
      hipLaunchKernelGGL(k_strip_gemm4_d<2>, dim3((unsigned)((nt + 15) / 16)), dim3(1024), 0, st, nt, kt, tailG.as<double>(), kt,
                         (const double *)cin, (const int32_t *)nullptr, (double *)zout);
      return true;
    } else {  // (only a handle that asked for the operator has one: build_tail_operator)
      launch_top_gemm_z(st, (int)tail_n, tailG.as<double>(), (const double *)cin, nullptr, (double *)zout, count);
      return true;
    }
  }
  // the instances of k_band_ls: CW = chunk rows / 16, NCH = chunks whose rows a wave holds in registers (CW * NCH <= kLsMaxSlots)
  static const void *ls_kernel(int cw, int nch) {
    typedef void (*K)(int32_t, const int32_t *, const int32_t *, const int32_t *, const int32_t *, const uint16_t *, const int32_t *,
                      const double *, const uint8_t *, const double *, const uint8_t *, const uint16_t *, const uint8_t *, double *, int32_t,
                      int32_t, int32_t, FirstL<double>, RowSkip);
    static const K tab[3][3] = {{k_band_ls<2, 2>, k_band_ls<2, 3>, k_band_ls<2, 4>},
                                {k_band_ls<3, 2>, k_band_ls<3, 3>, nullptr},
                                {k_band_ls<4, 2>, nullptr, nullptr}};
    return (cw < 2 || cw > 4 || nch < 2 || nch > 4) ? nullptr : (const void *)tab[cw - 2][nch - 2];
  }
  // ---- component bands: ONE choice of kernel (choose_band), one launch site per kernel (launch_band_cd) ----------------
  static constexpr size_t kBandLdsMax = 160 * 1024;  // a compute unit's LDS
  struct BandChoice {
    int family;        // census family (KF_BAND_*): names the kernel
    unsigned grid, block;
    size_t lds;        // bytes of dynamic LDS: the kernel's layout (band_lds.hpp) at the sizes below
    int32_t lds_rows;  // rows the layout holds (k_band_us: black rows, k_band_ls: dependent rows)
    int nsl = 1;       // column slices per component workgroup (the slice and tile kernels)
    int nct = 1;       // k_band_ct: column tiles per workgroup
    int32_t own_cap = 0, rptr_cap = 0;  // k_band_us / k_band_ls: own entries, row offsets of the layout
    int cw = 0, nch = 0;                // k_band_ls: the instance
  };
  // does the family's kernel take LastU, i.e. can it write the level's output itself (the fused S7)?
  static bool family_takes_last_u(int family) { return family != KF_BAND_CD_Z && family != KF_BAND_LS; }
  // Which kernel runs component band `band` of M (workgroups [g0, g1)) in a launch with these facts, and its launch shape.
  // Decides only; every condition of the choice is here and nowhere else.
  template <bool LOWER>
  BandChoice choose_band(const DevCsr &M, int32_t g0, int32_t g1, int pre, unsigned extra, bool with_f, size_t band,
                         bool no_walk) const {
    const unsigned n = (unsigned)(g1 - g0);
    if constexpr (std::is_same<T, double>::value) {
      const int32_t lds_rows = cd_lds_rows(M.cd_sparse);
      const size_t lds = BandCdLds(lds_rows, M.cd_sparse, M.own_cap).bytes();
      if (lds > kBandLdsMax)  // (only with HIFIR_AMD_CD_SPARSE_ROWS / HIFIR_AMD_CD_ROWS raised beyond their defaults)
        throw Error(HIFAMD_HIFIR_ERROR, "component band needs more than 160 KB of LDS: lower HIFIR_AMD_CD_SPARSE_ROWS / HIFIR_AMD_CD_ROWS");
      // column slices (k_band_cs): narrow batches always, full batches where the band is narrow
      const int nsl = std::min(4, (act_cols + 15) / 16);
      const bool fits = (int64_t)(g1 - g0) * nsl + 4 * (int64_t)extra < (1LL << 30);
      if (opt.ct_mode && M.ct_on && !M.cd_sparse && !with_f && fits) {  // coefficient tiles on the matrix cores, every batch width
        // a wide band takes two column tiles per workgroup (a coefficient tile is fetched for 32 columns at once); a narrow
        // one a workgroup per 16-column slice: its heaviest component then runs on four compute units
        const int ncols = (act_cols + 15) / 16;  // column tiles in use
        const int nct = (ncols == 4 && g1 - g0 > opt.ct_wide4_wgs) ? 4 : ((ncols >= 2 && g1 - g0 > opt.ct_wide_wgs) ? 2 : 1);
        const int nslc = (ncols + nct - 1) / nct;
        return {nct == 4 ? KF_BAND_CT4 : (nct == 2 ? KF_BAND_CT2 : KF_BAND_CT1), (unsigned)(((g1 - g0 + 7) / 8) * 8 * nslc) + 4 * extra, 256,
                BandCtLds(lds_rows, nct).bytes(), lds_rows, nslc, nct};
      }
      if (!LOWER && opt.us_mode && M.cd_sparse && nsl == 4 && !pre && !extra && !with_f && band < M.us_band_ok.size() && M.us_band_ok[band] &&
          !(opt.cs_mode && (g1 - g0 <= opt.cs_max_wgs || opt.cs_sparse))) {  // black rows in LDS, sinks streamed: two workgroups per unit
        const int32_t own_cap2 = (M.us_band_own[band] + 63) & ~63;
        const int32_t lds_black = std::max(1, M.us_band_nbk[band]);
        const size_t lds2 = BandUsLds(lds_black, own_cap2).bytes();
        if (lds2 <= kBandLdsMax) return {KF_BAND_US, n, 1024, lds2, lds_black, 1, 1, own_cap2};
      }
      if (LOWER && opt.ls_mode && M.cd_sparse && nsl == 4 && !pre && !extra && band < M.ls_band_ok.size() && M.ls_band_ok[band] &&
          (!with_f || M.ls_fused) && !(opt.cd_dbg & ~(kDbgCtPlain | kDbgSpmmPlain)) && !no_walk && !(opt.cs_mode && (g1 - g0 <= opt.cs_max_wgs || opt.cs_sparse))) {
        // dependent rows in LDS, sources through a chunk: two workgroups per unit
        const int cw = M.ls_band_cw[band], nch = std::max(2, M.ls_band_nch[band]);
        const int32_t own_cap2 = std::max(64, (M.ls_band_own[band] + 63) & ~63), rptr_cap = (M.ls_band_rptr[band] + 3) & ~3;
        const int32_t lds_dep = std::max(1, M.ls_band_nd[band]);
        const size_t lds2 = ls_lds_bytes(lds_dep, 16 * cw, own_cap2, rptr_cap);
        if (ls_kernel(cw, nch) && lds2 <= kLsLdsMax) return {KF_BAND_LS, n, 1024, lds2, lds_dep, 1, 1, own_cap2, rptr_cap, cw, nch};
      }
      if (opt.cs_mode && (nsl < 4 || g1 - g0 <= opt.cs_max_wgs || (opt.cs_sparse && M.cd_sparse)) && fits)
        return {M.cd_sparse ? KF_BAND_CS_SPARSE : KF_BAND_CS, n * (unsigned)nsl + 4 * extra, 256,
                BandCsLds(lds_rows, M.cd_sparse, M.own_cap).bytes(), lds_rows, nsl};
      return {M.cd_sparse ? KF_BAND_CD_SPARSE : KF_BAND_CD, n + extra, 1024, lds, lds_rows};
    } else {
      (void)pre, (void)with_f, (void)band, (void)no_walk;
      if (extra) throw Error(HIFAMD_HIFIR_ERROR, "internal error: carried prefix on a complex handle");
      const int nslz = std::min(4, (act_cols + 15) / 16);
      const int32_t lds_rows = cd_lds_rows(M.cd_sparse);
      if (opt.ct_mode && M.ct_on && !M.cd_sparse)  // coefficient tiles (round 4): 16-column slices at every batch width
        return {KF_BAND_CT_Z, n * (unsigned)nslz, 256, BandCtzLds(lds_rows).bytes(), lds_rows, nslz};
      if (M.cd_sparse) {  // sparse-own components (round 4): 16-column slices at every batch width
        const BandCszLds lay(lds_rows, true, M.own_cap);  // (lay.rows: even)
        return {KF_BAND_CS_Z, n * (unsigned)nslz, 256, lay.bytes(), lay.rows, nslz, 1, M.own_cap};
      }
      if (opt.cs_mode && nslz < 4 && (int64_t)(g1 - g0) * nslz < (1LL << 30))  // a narrow batch: only the slices it has
        return {KF_BAND_CS_Z, n * (unsigned)nslz, 256, BandCszLds(lds_rows, false, 0).bytes(), lds_rows, nslz};
      const int32_t rows = (int32_t)opt.band.cd_rows;  // (two planes of 64 columns: not rounded)
      return {KF_BAND_CD_Z, n, 1024, BandCdzLds(rows).bytes(), rows};
    }
  }
  // does the last U band of this level run through a kernel that can write the level's output itself (LastU)?  The band
  // as launch_trsv<false> launches it: nothing carried behind the last band, no F product.  (launch_trsv may split a
  // dense-own band of a real handle in two -- cd_two -- and then passes pre = 1 and no_walk: those two facts move the
  // choice only between k_band_us / k_band_ls and the kernels behind them, never to or from a family without LastU)
  bool s7_kernel_ok(const DevLevel &L) const {
    const DevCsr &M = L.U;
    const size_t b = M.band_wg_ptr.size() - 2;
    return family_takes_last_u(
        choose_band<false>(M, M.band_wg_ptr[b], M.band_wg_ptr[b + 1], band_has_prefix(M, b) ? 1 : 0, 0, false, b, false).family);
  }
  // every instance of the component band kernels with the most LDS the engine can ask of it: the layouts at the option
  // caps, never more than a compute unit has (choose_band refuses such a band) -- bind_device raises the limit from this
  std::vector<std::pair<const void *, size_t>> band_lds_table() const {
    std::vector<std::pair<const void *, size_t>> t;
    auto add = [&t](auto kernel, size_t bytes) { t.emplace_back((const void *)kernel, std::min(bytes, kBandLdsMax)); };
    if (opt.band.cd_rows <= 0) return t;
    const int32_t rd = cd_lds_rows(false), rs = cd_lds_rows(true);
    if constexpr (std::is_same<T, double>::value) {
      const size_t ct1 = BandCtLds(rd, 1).bytes(), ct2 = BandCtLds(rd, 2).bytes(), ct4 = BandCtLds(rd, 4).bytes();
      add(k_band_ct<true, 1, true>, ct1), add(k_band_ct<false, 1, true>, ct1), add(k_band_ct<true, 1, false>, ct1), add(k_band_ct<false, 1, false>, ct1);
      add(k_band_ct<true, 2, true>, ct2), add(k_band_ct<false, 2, true>, ct2), add(k_band_ct<true, 2, false>, ct2), add(k_band_ct<false, 2, false>, ct2);
      add(k_band_ct<true, 4, true>, ct4), add(k_band_ct<false, 4, true>, ct4), add(k_band_ct<true, 4, false>, ct4), add(k_band_ct<false, 4, false>, ct4);
      const size_t cdd = BandCdLds(rd, false, 0).bytes(), cds = BandCdLds(rs, true, kCdOwnCap).bytes();
      add(k_band_cd<true, false>, cdd), add(k_band_cd<false, false>, cdd), add(k_band_cd<true, true>, cds), add(k_band_cd<false, true>, cds);
      const size_t csd = BandCsLds(rd, false, 0).bytes(), css = BandCsLds(rs, true, kCdOwnCap).bytes();
      add(k_band_cs<true, false>, csd), add(k_band_cs<false, false>, csd), add(k_band_cs<true, true>, css), add(k_band_cs<false, true>, css);
      add(k_band_us, BandUsLds(rs, kCdOwnCap).bytes());
      for (int cw = 2; cw <= 4; ++cw)
        for (int nch = 2; nch <= ls_max_chunks(cw); ++nch)  // (choose_band takes the kernel up to kLsLdsMax)
          t.emplace_back(ls_kernel(cw, nch), std::min(ls_lds_bytes(rs, 16 * cw, kCdOwnCap, (nch + 1) * rs + 4), kLsLdsMax));
    } else {
      add(k_band_ct_z<true>, BandCtzLds(rd).bytes()), add(k_band_ct_z<false>, BandCtzLds(rd).bytes());
      const size_t csd = BandCszLds(rd, false, 0).bytes(), css = BandCszLds(rs, true, kCdOwnCap).bytes();
      add(k_band_cs_z<true, false>, csd), add(k_band_cs_z<false, false>, csd), add(k_band_cs_z<true, true>, css), add(k_band_cs_z<false, true>, css);
      const size_t cdz = BandCdzLds((int32_t)opt.band.cd_rows).bytes();
      add(k_band_cd_z<true>, cdz), add(k_band_cd_z<false>, cdz);
    }
    return t;
  }
  template <bool LOWER>
  void launch_band_cd(hipStream_t st, const DevLevel &L, const DevCsr &M, int32_t g0, int32_t g1, int pre, int32_t ps0,
                      int32_t ps1, unsigned extra, const FL &fl, bool with_f = false, const LU &lu = no_lu(), size_t band = 0,
                      bool no_walk = false, RowSkip rs = RowSkip{nullptr}) {
    const BandChoice c = choose_band<LOWER>(M, g0, g1, pre, extra, with_f, band, no_walk);
    const dim3 grid(c.grid), block(c.block);
    const int first_u = pre ? 0 : 1;  // (the packed streams already start at split[] for a carried band, at ptr[] otherwise)
    const int dbg = opt.cd_dbg | (no_walk ? 1 : 0);
    const int32_t n_band = g1 - g0;
    tally(c.family);
    if constexpr (std::is_same<T, double>::value) {
      // one component per workgroup (the usual case): the kernel derives the component from blockIdx
      const int32_t c0 = M.host_wg_grp_ptr[(size_t)g0], c1 = M.host_wg_grp_ptr[(size_t)g1];
      const int32_t single_c0 = (c1 - c0 == g1 - g0) ? c0 : -1;
      const RowSkip rsk = M.cd_sparse ? rs : RowSkip{nullptr};
      switch (c.family) {
      case KF_BAND_CT1:
      case KF_BAND_CT2:
      case KF_BAND_CT4: {
        const bool ct_ahead = !(opt.cd_dbg & kDbgCtPlain);
        auto kct = ct_ahead ? (c.nct == 4 ? k_band_ct<LOWER, 4, true> : (c.nct == 2 ? k_band_ct<LOWER, 2, true> : k_band_ct<LOWER, 1, true>))
                            : (c.nct == 4 ? k_band_ct<LOWER, 4, false> : (c.nct == 2 ? k_band_ct<LOWER, 2, false> : k_band_ct<LOWER, 1, false>));
        hipLaunchKernelGGL(kct, grid, block, c.lds, st, g0,
                           M.wg_grp_ptr.as<int32_t>(), M.ct_desc.as<int32_t>(), M.ptr.as<int32_t>(), M.split.as<int32_t>(),
                           M.col.as<int32_t>(), M.val.as<double>(), M.rowid.as<int32_t>(), L.d.as<double>(), L.w.as<double>(),
                           L.v.as<double>(), M.tinv.as<double>(), M.ct_sptr.as<int32_t>(), M.ct_src.as<int32_t>(),
                           M.ct_coef.as<double>(), first_u, n_band, (int32_t)c.nsl, ps0, ps1, single_c0, c.lds_rows, dbg, fl, lu);
        break;
      }
      case KF_BAND_US:
        hipLaunchKernelGGL(k_band_us, grid, block, c.lds, st, M.us_band_c0[band], M.us_desc.as<int32_t>(),
                           M.us_rowid.as<int32_t>(), M.us_oslot.as<int32_t>(), M.us_mptr.as<int32_t>(), M.us_mcol.as<int32_t>(),
                           M.us_mval.as<double>(), M.us_own_val.as<double>(), M.us_own_src.as<uint8_t>(), M.us_own_rptr.as<uint16_t>(),
                           M.us_own_lvl.as<uint8_t>(), L.d.as<double>(), (const double *)L.w.as<double>(), L.v.as<double>(), c.lds_rows,
                           c.own_cap, fl, lu, rsk);
        break;
      case KF_BAND_LS: {
        const int f = with_f ? 1 : 0;
        int32_t a_c0 = M.ls_band_c0[band], a_dep = c.lds_rows, a_own = c.own_cap, a_rp = c.rptr_cap;
        const int32_t *a_desc = M.ls_desc.as<int32_t>(), *a_rowid = M.ls_rowid.as<int32_t>(), *a_oslot = M.ls_oslot.as<int32_t>();
        const int32_t *a_eb = M.ls_ebase[f].template as<int32_t>(), *a_ec = M.ls_ecol[f].template as<int32_t>();
        const uint16_t *a_ew = M.ls_ewptr[f].template as<uint16_t>(), *a_or = M.ls_own_rptr.as<uint16_t>();
        const double *a_ev = M.ls_eval[f].template as<double>(), *a_ov = M.ls_own_val.as<double>();
        const uint8_t *a_et = M.ls_etag[f].template as<uint8_t>(), *a_os = M.ls_own_src.as<uint8_t>(), *a_ol = M.ls_own_lvl.as<uint8_t>();
        double *a_w = L.w.as<double>();
        FL a_fl = fl;
        RowSkip a_rs = rs;
        void *args[] = {&a_c0, &a_desc, &a_rowid, &a_oslot, &a_eb, &a_ew, &a_ec, &a_ev, &a_et, &a_ov, &a_os, &a_or, &a_ol, &a_w,
                        &a_dep, &a_own, &a_rp, &a_fl, &a_rs};
        HIP_OK(hipLaunchKernel(ls_kernel(c.cw, c.nch), grid, block, args, c.lds, st));
        break;
      }
      case KF_BAND_CS:
      case KF_BAND_CS_SPARSE:
        hipLaunchKernelGGL((M.cd_sparse ? k_band_cs<LOWER, true> : k_band_cs<LOWER, false>), grid, block, c.lds, st, g0,
                           M.wg_grp_ptr.as<int32_t>(), (with_f ? M.f_desc : M.cd_desc).template as<int32_t>(), M.ptr.as<int32_t>(),
                           M.split.as<int32_t>(), M.col.as<int32_t>(), M.val.as<double>(), M.rowid.as<int32_t>(), L.d.as<double>(),
                           L.w.as<double>(), L.v.as<double>(), M.tinv.as<double>(), (with_f ? M.f_col : M.mid_col).template as<int32_t>(),
                           (with_f ? M.f_val : M.mid_val).template as<double>(), (with_f ? M.f_lrow : M.mid_lrow).template as<uint8_t>(),
                           first_u, n_band, (int32_t)c.nsl, ps0, ps1, single_c0, c.lds_rows, M.own_cap, dbg, fl, M.own_val.as<double>(),
                           M.own_lsrc.as<uint8_t>(), M.own_rptr.as<uint16_t>(), M.own_lvl.as<uint8_t>(), lu, rsk);
        break;
      default:  // KF_BAND_CD, KF_BAND_CD_SPARSE
        hipLaunchKernelGGL((M.cd_sparse ? k_band_cd<LOWER, true> : k_band_cd<LOWER, false>), grid, block, c.lds, st, g0,
                           M.wg_grp_ptr.as<int32_t>(), (with_f ? M.f_desc : M.cd_desc).template as<int32_t>(), M.ptr.as<int32_t>(),
                           M.split.as<int32_t>(), M.col.as<int32_t>(), M.val.as<double>(), M.rowid.as<int32_t>(), L.d.as<double>(),
                           L.w.as<double>(), L.v.as<double>(), M.tinv.as<double>(), (with_f ? M.f_col : M.mid_col).template as<int32_t>(),
                           (with_f ? M.f_val : M.mid_val).template as<double>(), (with_f ? M.f_lrow : M.mid_lrow).template as<uint8_t>(),
                           first_u, n_band, ps0, ps1, single_c0, c.lds_rows, M.own_cap, dbg, fl, M.own_val.as<double>(),
                           M.own_lsrc.as<uint8_t>(), M.own_rptr.as<uint16_t>(), M.own_lvl.as<uint8_t>(), lu, rsk);
      }
    } else {
      (void)ps0, (void)ps1, (void)n_band, (void)rs;
      switch (c.family) {
      case KF_BAND_CT_Z:
        hipLaunchKernelGGL(k_band_ct_z<LOWER>, grid, block, c.lds, st, g0, M.wg_grp_ptr.as<int32_t>(),
                           M.ct_desc.as<int32_t>(), M.rowid.as<int32_t>(), L.d.as<cplx>(), L.w.as<cplx>(), L.v.as<cplx>(),
                           M.tinv.as<double>(), M.ct_sptr.as<int32_t>(), M.ct_src.as<int32_t>(), M.ct_coef.as<double>(), first_u,
                           (int32_t)c.nsl, c.lds_rows, dbg, fl, lu);
        break;
      case KF_BAND_CS_Z:
        if (M.cd_sparse)
          hipLaunchKernelGGL((k_band_cs_z<LOWER, true>), grid, block, c.lds, st, g0,
                             M.wg_grp_ptr.as<int32_t>(), M.cd_desc.as<int32_t>(), M.rowid.as<int32_t>(), L.d.as<cplx>(), L.w.as<cplx>(),
                             L.v.as<cplx>(), M.tinv.as<double>(), M.mid_col.as<int32_t>(), M.mid_val.as<cplx>(), M.mid_lrow.as<uint8_t>(),
                             first_u, (int32_t)c.nsl, c.lds_rows, fl, c.own_cap, M.own_val.as<cplx>(), M.own_lsrc.as<uint8_t>(),
                             M.own_rptr.as<uint16_t>(), M.own_lvl.as<uint8_t>(), lu);
        else
          hipLaunchKernelGGL((k_band_cs_z<LOWER, false>), grid, block, c.lds, st, g0,
                             M.wg_grp_ptr.as<int32_t>(), M.cd_desc.as<int32_t>(), M.rowid.as<int32_t>(), L.d.as<cplx>(), L.w.as<cplx>(),
                             L.v.as<cplx>(), M.tinv.as<double>(), M.mid_col.as<int32_t>(), M.mid_val.as<cplx>(), M.mid_lrow.as<uint8_t>(),
                             first_u, (int32_t)c.nsl, c.lds_rows, fl, 0, (const cplx *)nullptr, (const uint8_t *)nullptr,
                             (const uint16_t *)nullptr, (const uint8_t *)nullptr, lu);
        break;
      default:  // KF_BAND_CD_Z
        hipLaunchKernelGGL(k_band_cd_z<LOWER>, grid, block, c.lds, st, g0, M.wg_grp_ptr.as<int32_t>(),
                           M.cd_desc.as<int32_t>(), M.rowid.as<int32_t>(), L.d.as<cplx>(), L.w.as<cplx>(), L.v.as<cplx>(),
                           M.tinv.as<double>(), M.mid_col.as<int32_t>(), M.mid_val.as<cplx>(), M.mid_lrow.as<uint8_t>(), first_u,
                           c.lds_rows, fl);
      }
    }
    // a refused launch is an error, not a band that did not run (launches happen at capture, not at replay).  The call
    // also returns and clears an earlier error of this thread that nobody looked at: that one is then reported here
    HIP_OK(hipGetLastError());
  }

  // first: this is the level's FIRST solve with S1 fused -- the bands may leave out what build_row_flags marked
  void launch_ldu(hipStream_t st, DevLevel &L, int logR, int64_t &count, const FL *fl = nullptr, bool with_f = false,
                  const LU *lu = nullptr, bool first = false) {
    if (!L.m) return;
    const bool skip = first && fl && !with_f && !lu && logR == 6 && L.L.rowflag.p && L.U.rowflag.p;
    launch_trsv<true>(st, L, logR, count, fl, with_f, nullptr, skip ? fl : nullptr);
    launch_trsv<false>(st, L, logR, count, nullptr, false, lu, skip ? fl : nullptr);
  }

  // complex products on the real matrix cores (operands: two real planes, see host.hpp mfma_operand)
  void zgemm(hipStream_t st, int rows_total, int rows_valid, int kend, int tri, const DevBuf &A, int lda, const cplx *X,
             int logR, const int32_t *rowmap, cplx *Out, const cplx *dscale, cplx *Out2, int64_t &count) {
    const double *Are = A.as<double>(), *Aim = Are + plane_elems(rows_total, lda);
    const dim3 grid((unsigned)((rows_total + 15) / 16), ((2u << logR) + 15) / 16);
    double *t1 = zt1.as<double>(), *t2 = zt2.as<double>();
    tally(KF_DENSE_GEMM, 2), tally(KF_ZCOMBINE);
    hipLaunchKernelGGL(k_dense_gemm_d<4>, grid, dim3(256), 0, st, rows_total, rows_valid, kend, tri, Are, lda,
                       (const double *)X, logR + 1, (const int32_t *)nullptr, t1, (const double *)nullptr, (double *)nullptr);
    hipLaunchKernelGGL(k_dense_gemm_d<4>, grid, dim3(256), 0, st, rows_total, rows_valid, kend, tri, Aim, lda,
                       (const double *)X, logR + 1, (const int32_t *)nullptr, t2, (const double *)nullptr, (double *)nullptr);
    hipLaunchKernelGGL(k_zcombine, dim3(grid_for(rows_total, logR)), dim3(256), 0, st, (int64_t)rows_total,
                       (const double *)t1, (const double *)t2, logR, rowmap, Out, dscale, Out2);
    count += 3;
  }
  // the same step of a real handle: one product, one workgroup per 16-row strip (4 waves split K)
  void zgemm(hipStream_t st, int rows_total, int rows_valid, int kend, int tri, const DevBuf &A, int lda, const double *X,
             int logR, const int32_t *rowmap, double *Out, const double *dscale, double *Out2, int64_t &count) {
    const dim3 grid((unsigned)((rows_total + 15) / 16), ((1u << logR) + 15) / 16);
    hipLaunchKernelGGL(k_dense_gemm_d<4>, grid, dim3(256), 0, st, rows_total, rows_valid, kend, tri, A.as<double>(), lda, X,
                       logR, rowmap, Out, dscale, Out2);
    tally(KF_DENSE_GEMM);
    ++count;
  }
  void row_gather(hipStream_t st, const D *in, const int32_t *map, int rows, D *out, int logR, int64_t &count) {
    hipLaunchKernelGGL((k_row_gather<D>), dim3(grid_for(rows, logR)), dim3(256), 0, st, in, map, (int64_t)rows, out, logR);
    tally(KF_ROW_GATHER);
    ++count;
  }
  void zgemm_tri(hipStream_t st, int nb, const double *Aops, const cplx *X, int logR, const int32_t *rowmap, cplx *Out,
                 const cplx *dscale, cplx *Out2, int64_t &count) {
    const int lda = (int)round_up32(nb);
    const double *Are = Aops, *Aim = Aops + plane_elems(nb, lda);
    const unsigned pairs = (unsigned)(((nb + 15) / 16 + 1) / 2);
    const dim3 grid(pairs, ((2u << logR) + 15) / 16);
    double *t1 = zt1.as<double>(), *t2 = zt2.as<double>();
    tally(KF_TRI_GEMM, 2), tally(KF_ZCOMBINE);
    hipLaunchKernelGGL(k_tri_gemm_d<16>, grid, dim3(1024), 0, st, nb, Are, lda, (const double *)X, logR + 1,
                       (const int32_t *)nullptr, t1, (const double *)nullptr, (double *)nullptr);
    hipLaunchKernelGGL(k_tri_gemm_d<16>, grid, dim3(1024), 0, st, nb, Aim, lda, (const double *)X, logR + 1,
                       (const int32_t *)nullptr, t2, (const double *)nullptr, (double *)nullptr);
    hipLaunchKernelGGL(k_zcombine, dim3(grid_for(nb, logR)), dim3(256), 0, st, (int64_t)nb, (const double *)t1,
                       (const double *)t2, logR, rowmap, Out, dscale, Out2);
    count += 3;
  }
  // the same step of a real handle: one product, with as many waves as gemm_waves asks for
  void zgemm_tri(hipStream_t st, int nb, const double *Aops, const double *X, int logR, const int32_t *rowmap, double *Out,
                 const double *dscale, double *Out2, int64_t &count) {
    const int lda = (int)round_up32(nb);
    const unsigned pairs = (unsigned)(((nb + 15) / 16 + 1) / 2);
    const dim3 grid(pairs, ((1u << logR) + 15) / 16);
    tally(KF_TRI_GEMM);
    if (opt.gemm_waves >= 16)
      hipLaunchKernelGGL(k_tri_gemm_d<16>, grid, dim3(1024), 0, st, nb, Aops, lda, X, logR, rowmap, Out, dscale, Out2);
    else if (opt.gemm_waves >= 8)
      hipLaunchKernelGGL(k_tri_gemm_d<8>, grid, dim3(512), 0, st, nb, Aops, lda, X, logR, rowmap, Out, dscale, Out2);
    else
      hipLaunchKernelGGL(k_tri_gemm_d<4>, grid, dim3(256), 0, st, nb, Aops, lda, X, logR, rowmap, Out, dscale, Out2);
    ++count;
  }

  // dense last level: z = P * [ Rinv(1:rk,1:rk) * (Q^H c)(1:rk) ; 0 ]   (QRCP::_solve_nt, QRCP.hpp:371-411)
  void launch_dense(hipStream_t st, const D *cin, D *zout, int logR, int64_t rank, int64_t &count) {
    const int nd = (int)dn.n, rk = (int)eff_rank(rank);
    D *tmp = dn.tmp.as<D>();
    if (dn.lup) {  // LUP::solve (LUP.hpp:141-152): ?getrs, here one product with the explicit inverse; rank is ignored
      zgemm(st, nd, nd, nd, 0, dn.QH, nd, cin, logR, nullptr, zout, nullptr, nullptr, count);
      return;
    }
    if (dn.symm) {  // SYEIG::solve (SYEIG.hpp:181-200): z = V(:,to(1:rk)) diag(1/w) V(:,to(1:rk))^H c
      zgemm(st, nd, rk, nd, 0, dn.QH, nd, cin, logR, nullptr, tmp, nullptr, nullptr, count);
      zgemm(st, nd, nd, rk, 0, dn.Qm, nd, tmp, logR, nullptr, zout, nullptr, nullptr, count);
      return;
    }
    if (adjoint) {  // QRCP::_solve_t (QRCP.hpp:413-452): z = Q(:,1:rk) R(1:rk,1:rk)^{-H} (P^T c)(1:rk)
      D *tmp2 = dn.tmp2.as<D>();
      row_gather(st, cin, dn.jpvt0.as<int32_t>(), nd, tmp2, logR, count);
      // T1[i] = sum_{k<=i} conj(Rinv(k,i)) c[jpvt[k]], i < rk (rows >= rk come out as zeros)
      zgemm(st, nd, rk, rk, 2, dn.RinvH, nd, tmp2, logR, nullptr, tmp, nullptr, nullptr, count);
      zgemm(st, nd, nd, rk, 0, dn.Qm, nd, tmp, logR, nullptr, zout, nullptr, nullptr, count);
      return;
    }
    // T1 = Q^H(1:rk, :) c   (rows >= rk come out as zeros and are never read)
    zgemm(st, nd, rk, nd, 0, dn.QH, nd, cin, logR, nullptr, tmp, nullptr, nullptr, count);
    // z[jpvt[i]] = sum_{k>=i} Rinv(i,k) T1[k], i < rk; zero rows beyond rk
    zgemm(st, nd, rk, rk, 1, dn.Rinv, nd, tmp, logR, dn.jpvt0.as<int32_t>(), zout, nullptr, nullptr, count);
  }

  int64_t eff_rank(int64_t rank) const {
    if (rank == 0) return dn.rank;
    if (rank < 0 || rank > dn.n) return dn.n;
    return rank;
  }

  // one level of prec_solve (prec_solve.hpp:332-412); bin/yout may be user or arena pointers
  typedef IoPtr<const D> InP;
  typedef IoPtr<D> OutP;
  static InP in_direct(const D *p) { return InP{p, nullptr, 0}; }
  static OutP out_direct(D *p) { return OutP{p, nullptr, 0}; }

  // S3 / S5: out = s[p] b[p] - A x.  R = 64, fast mode, real data, rows that share columns: on the matrix cores
  // (k_spmm_tile); otherwise the row-gather kernel in the reference's summation order (k_spmm_epi)
  // the instance of the tiled products: row tiles per block, column tiles of the batch, requests running ahead or the former loop
  typedef void (*SpmmTileKernel)(int64_t, int64_t, const int32_t *, const int32_t *, const double *, const double *, IoPtr<const double>,
                                 int64_t, int, const int32_t *, const double *, int64_t, double *);
  template <bool AHEAD>
  static SpmmTileKernel spmm_tile_kernel_of(int rb, int nct) {
    return rb == 2 ? (nct == 1 ? k_spmm_tile<2, 1, AHEAD> : nct == 2 ? k_spmm_tile<2, 2, AHEAD> : nct == 3 ? k_spmm_tile<2, 3, AHEAD> : k_spmm_tile<2, 4, AHEAD>)
                   : (nct == 1 ? k_spmm_tile<1, 1, AHEAD> : nct == 2 ? k_spmm_tile<1, 2, AHEAD> : nct == 3 ? k_spmm_tile<1, 3, AHEAD> : k_spmm_tile<1, 4, AHEAD>);
  }
  template <bool AHEAD>
  static SpmmTileKernel spmm_tile4_kernel_of(int rb, int nct) {
    return rb == 2 ? (nct == 1 ? k_spmm_tile4<2, 1, AHEAD> : nct == 2 ? k_spmm_tile4<2, 2, AHEAD> : nct == 3 ? k_spmm_tile4<2, 3, AHEAD> : k_spmm_tile4<2, 4, AHEAD>)
                   : (nct == 1 ? k_spmm_tile4<1, 1, AHEAD> : nct == 2 ? k_spmm_tile4<1, 2, AHEAD> : nct == 3 ? k_spmm_tile4<1, 3, AHEAD> : k_spmm_tile4<1, 4, AHEAD>);
  }
  static SpmmTileKernel spmm_tile_kernel(int rb, int nct, bool ahead) { return ahead ? spmm_tile_kernel_of<true>(rb, nct) : spmm_tile_kernel_of<false>(rb, nct); }
  static SpmmTileKernel spmm_tile4_kernel(int rb, int nct, bool ahead) { return ahead ? spmm_tile4_kernel_of<true>(rb, nct) : spmm_tile4_kernel_of<false>(rb, nct); }

  void launch_spmm(hipStream_t st, const DevCsr &A, int64_t nrows, const D *x, InP bin, int64_t ldb, int nrhs,
                   const DevLevel &L, int64_t roff, D *out, int logR) {
    if constexpr (std::is_same<T, double>::value) {
      // one block per workgroup, its groups dealt to the four waves: where the per-wave kernel would leave the chip short
      // of waves (with more blocks the product runs at the fabric's gather bandwidth either way: 95 vs 100 us, 101 vs 123 us)
      const int nct = opt.narrow_tiles ? std::min(4, (act_cols + 15) / 16) : 4;  // column tiles of the batch
      const bool ahead = !(opt.cd_dbg & kDbgSpmmPlain);
      if (A.tl_nblk > 0 && A.tl_nblk < opt.spmm_split_blocks && logR == 6 && opt.spmm_split) {
        auto k4 = spmm_tile4_kernel(A.tl_rb, nct, ahead);
        tally(A.tl_rb == 2 ? KF_SPMM_TILE4_RB2 : KF_SPMM_TILE4_RB1);
        hipLaunchKernelGGL(k4, dim3((unsigned)A.tl_nblk), dim3(256), 0, st, nrows, A.tl_nblk, A.tl_gptr.as<int32_t>(),
                           A.tl_ucol.as<int32_t>(), A.tl_coef.as<double>(), (const double *)x, bin, ldb, nrhs, L.p.as<int32_t>(),
                           L.s.as<double>(), roff, out);
        return;
      }
      if (A.tl_nblk > 0 && logR == 6) {
        const unsigned grid = (unsigned)std::min<int64_t>((A.tl_nblk + 3) / 4, 256 * 16);
        auto k1 = spmm_tile_kernel(A.tl_rb, nct, ahead);
        tally(A.tl_rb == 2 ? KF_SPMM_TILE_RB2 : KF_SPMM_TILE_RB1);
        hipLaunchKernelGGL(k1, dim3(grid), dim3(256), 0, st, nrows, A.tl_nblk, A.tl_gptr.as<int32_t>(),
                           A.tl_ucol.as<int32_t>(), A.tl_coef.as<double>(), (const double *)x, bin, ldb, nrhs, L.p.as<int32_t>(),
                           L.s.as<double>(), roff, out);
        return;
      }
    }
    if constexpr (!std::is_same<T, double>::value) {
      if (A.tl_nblk > 0 && logR == 6) {  // complex coupling block on coefficient tiles: one 16-column slice per grid row
        const unsigned gx = (unsigned)std::min<int64_t>((A.tl_nblk + 3) / 4, 256 * 16);
        const unsigned gy = (unsigned)std::min(4, (act_cols + 15) / 16);
        tally(KF_SPMM_TILE_Z);
        hipLaunchKernelGGL(k_spmm_tile_z, dim3(gx, gy), dim3(256), 0, st, nrows, A.tl_nblk, A.tl_gptr.as<int32_t>(),
                           A.tl_ucol.as<int32_t>(), A.tl_coef.as<double>(), (const cplx *)x, bin, ldb, nrhs, L.p.as<int32_t>(),
                           L.s.as<double>(), roff, (cplx *)out);
        return;
      }
    }
    // a narrow batch in the 64-column arena: 64 / R rows per wave (R = 16 or 32 lanes per row)
    if (logR == 6 && opt.narrow_spmm && act_cols <= 32) {
      const int lr = act_cols <= 16 ? 4 : 5;
      tally(KF_SPMM_EPI_NARROW);
      hipLaunchKernelGGL((k_spmm_epi_narrow<D>), dim3(grid_for(nrows, lr)), dim3(256), 0, st, nrows, A.ptr.as<int32_t>(),
                         A.col.as<int32_t>(), A.val.as<D>(), x, bin, ldb, nrhs, L.p.as<int32_t>(), L.s.as<double>(), roff, out, lr);
      return;
    }
    tally(KF_SPMM_EPI);
    hipLaunchKernelGGL((k_spmm_epi<D>), dim3(grid_for(nrows, logR)), dim3(256), 0, st, nrows, A.ptr.as<int32_t>(),
                       A.col.as<int32_t>(), A.val.as<D>(), x, bin, ldb, nrhs, L.p.as<int32_t>(), L.s.as<double>(), roff, out,
                       logR);
  }

  void launch_s7_list(hipStream_t st, const DevLevel &L, const D *v, int64_t first, int64_t cnt, OutP yout, int64_t ldy, int nrhs) {
    tally(KF_SCATTER_SCALE_LIST);
    hipLaunchKernelGGL((k_scatter_scale_list<D>), dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(8192, (cnt + 15) / 16))), dim3(256), 0,
                       st, v, L.qinv.as<int32_t>(), L.t.as<double>(), L.s7_list.as<int32_t>() + first, cnt, yout, ldy, nrhs);
  }
  // fork / join of the side stream around one level's early S7 list (inside a stream capture these become graph edges)
  void side_fork(hipStream_t st, size_t l) {
    if (!side_stream) HIP_OK(hipStreamCreateWithFlags(&side_stream, hipStreamNonBlocking));
    while (ev_side_fork.size() <= l) {
      hipEvent_t a = nullptr, b = nullptr;
      HIP_OK(hipEventCreateWithFlags(&a, hipEventDisableTiming));
      HIP_OK(hipEventCreateWithFlags(&b, hipEventDisableTiming));
      ev_side_fork.push_back(a);
      ev_side_join.push_back(b);
    }
    HIP_OK(hipEventRecord(ev_side_fork[l], st));
    HIP_OK(hipStreamWaitEvent(side_stream, ev_side_fork[l], 0));
  }
  void side_join(hipStream_t st, size_t l) {
    HIP_OK(hipEventRecord(ev_side_join[l], side_stream));
    HIP_OK(hipStreamWaitEvent(st, ev_side_join[l], 0));
  }
  void enqueue_level(hipStream_t st, size_t l, InP bin, int64_t ldb, OutP yout, int64_t ldy, int nrhs,
                     int logR, int64_t rank, int64_t &count) {
    DevLevel &L = *lv[l];
    const int64_t m = L.m, n = L.n, nm = n - m;
    const int64_t R = 1LL << logR;
    D *w = L.w.as<D>(), *v = L.v.as<D>();
    const bool last = (l + 1 == lv.size());
    // S1 (:359, :402) fused into the L solve that follows it (kernels FirstL): the R = 64 band pipeline only
    const bool fuse_s1 = opt.fuse_gather && logR == 6 && opt.band_pipe && m > 0;
    cur_level = (int)l;
    const FL fl{bin, ldb, nrhs, L.p.as<int32_t>(), L.s.as<double>()};
    const bool fuse_f_lv = fuse_s1 && L.L.f_fused;  // S5 fused as well (level with thin F rows, all-component L plan)
    const bool fuse_s7_lv = opt.fuse_out && logR == 6 && m > 0 && L.s7_n >= 0 && s7_kernel_ok(L);
    int64_t early_rows = 0;  // rows of the S7 list already sent out on the side stream
    int64_t c0 = count;
    if (m && !fuse_s1) {  // S1  :359
      tally(KF_GATHER_SCALE);
      hipLaunchKernelGGL((k_gather_scale<D>), dim3(grid_for(m, logR)), dim3(256), 0, st, bin, ldb, nrhs,
                         L.p.as<int32_t>(), L.s.as<double>(), m, w, logR);
      ++count;
    }
    mark(l, 1, c0, count);
    if (nm) {
      c0 = count;
      launch_ldu(st, L, logR, count, fuse_s1 ? &fl : nullptr, false, nullptr, /*first=*/fuse_s1);  // S2  :364
      mark(l, 2, c0, count);
      // S3  :366-368  -> w[m:n] (becomes the child's rhs, :386)
      c0 = count;
      launch_spmm(st, L.E, nm, v, bin, ldb, nrhs, L, m, w + m * R, logR);
      ++count;
      mark(l, 3, c0, count);
      c0 = count;
      if (last) {
        launch_dense(st, w + m * R, v + m * R, logR, rank, count);  // :371-381
        mark(l, 4, c0, count);
      } else if ((int64_t)l + 1 == tail_level && logR == 6 && (!host.has_dense || eff_rank(rank) == dn.rank) &&  // (the rank it was built with)
                 (cur_level = (int)l + 1, launch_tail(st, w + m * R, v + m * R, count))) {
        mark(l + 1, 4, c0, count);  // (levels l+1 ... and the dense block as one product)
      } else
        enqueue_level(st, l + 1, in_direct(w + m * R), R, out_direct(v + m * R), R, (int)R, logR, rank, count);  // :383-388
      cur_level = (int)l;
      // S7 of the child's rows (:411) needs nothing of this level's second solve: it leaves now, on the side stream, beside
      // S5 / S6 (whose component bands are latency-bound and leave the memory system room); joined at the end of the level
      if (fuse_s7_lv && opt.list_early && L.s7_child > 0) {
        c0 = count;
        side_fork(st, l);
        launch_s7_list(side_stream, L, v, 0, L.s7_child, yout, ldy, nrhs);
        ++count;
        mark(l, 7, c0, count);
        early_rows = L.s7_child;
      }
      // S5  :392-403   (v[m:n] already is "work[m:n] = y[m:n]")
      c0 = count;
      if (m) {
        if (L.F_ncols && fuse_f_lv) {
          // fused into the first touch of the L solve below: rhs = s b[p] - sum F v[m + k] (FirstL + the F streams)
        } else if (L.F_ncols) {
          launch_spmm(st, L.F, m, v + m * R, bin, ldb, nrhs, L, (int64_t)0, w, logR);
          ++count;
        } else if (!fuse_s1) {
          tally(KF_GATHER_SCALE);
          hipLaunchKernelGGL((k_gather_scale<D>), dim3(grid_for(m, logR)), dim3(256), 0, st, bin, ldb, nrhs,
                             L.p.as<int32_t>(), L.s.as<double>(), m, w, logR);
          ++count;
        }
      }
      mark(l, 5, c0, count);
    }
    // S6  :406  (its right-hand side is w = s b[p] - F y from S5, or -- no F, or no Schur complement at all -- S1 again)
    // S7 (:411) fused into the last band of this U solve where the plan allows (kernels LastU; finalize built the list of
    // output rows that band does not write)
    const bool fuse_s7 = fuse_s7_lv;
    const LU lu{yout, ldy, nrhs, L.q_s7.as<int32_t>(), L.t.as<double>()};
    c0 = count;
    launch_ldu(st, L, logR, count, (fuse_s1 && (!(nm && L.F_ncols) || fuse_f_lv)) ? &fl : nullptr, fuse_f_lv && nm && L.F_ncols,
               fuse_s7 ? &lu : nullptr);
    mark(l, 6, c0, count);
    c0 = count;
    if (fuse_s7) {
      if (L.s7_n > early_rows) {
        launch_s7_list(st, L, v, early_rows, L.s7_n - early_rows, yout, ldy, nrhs);
        ++count;
      }
      if (early_rows) side_join(st, l);
    } else {
      tally(KF_SCATTER_SCALE);
      hipLaunchKernelGGL((k_scatter_scale<D>), dim3(grid_for(n, logR)), dim3(256), 0, st, v, L.qinv.as<int32_t>(),
                         L.t.as<double>(), n, yout, ldy, nrhs, logR);
      ++count;
    }
    mark(l, 7, c0, count);
  }

  // ---- y = M b: prec_prod (alg/prec_prod.hpp:55-147), the inverse direction of the apply ------------
  // On the adjoint engine the same code is prec_prod_tran (:148-235): the adjoint hierarchy swaps the
  // roles exactly as that function does.
  bool prod_ready = false;
  void ensure_prod_buffers() {
    if (prod_ready) return;
    for (size_t l = 0; l < lv.size(); ++l) {
      DevLevel &L = *lv[l];
      const HostLevel<T> &H = host.levels[l];
      if (H.q.empty() || H.p_inv.empty())
        throw Error(HIFAMD_BAD_PREC, "the product operators need the q and p_inv permutations (hifamd_add_level)");
      L.q.upload(H.q);
      L.pinv.upload(H.p_inv);
      const size_t bytes = (size_t)H.n * Rmax * sizeof(T);
      L.pg.alloc(bytes);
      L.pc.alloc(bytes);
      L.pr.alloc(bytes);
    }
    if (host.has_dense && host.dense.kind == 2) {  // LUP::multiply: the unfactored block itself (LUP.hpp:181-188)
      HostDense<T> &Dn = host.dense;
      dense_lup_ops(Dn, adjoint);
      dn.Rm.upload(mfma_operand(Dn.SymMul.data(), Dn.n, Dn.n));
      std::vector<T>().swap(Dn.QH);
      std::vector<T>().swap(Dn.SymMul);
    } else if (host.has_dense && host.dense.kind == 1) {  // SYEIG::multiply: V diag(w) V^H (SYEIG.hpp:256-273), either engine
      HostDense<T> &Dn = host.dense;
      dense_symm_ops(Dn);
      dn.Rm.upload(mfma_operand(Dn.SymMul.data(), Dn.n, Dn.n));
      std::vector<T>().swap(Dn.QH);
      std::vector<T>().swap(Dn.Q);
      std::vector<T>().swap(Dn.SymMul);
    } else if (host.has_dense) {
      HostDense<T> &Dn = host.dense;
      const int64_t n = Dn.n;
      std::vector<T> Rm((size_t)(n * n), T(0));  // R (upper incl. diagonal) or, on the adjoint engine, R^H
      for (int64_t j = 0; j < n; ++j)
        for (int64_t i = 0; i <= j; ++i) {
          if (adjoint)
            Rm[(size_t)(j + i * n)] = conj_(Dn.qr[(size_t)(i + j * n)]);
          else
            Rm[(size_t)(i + j * n)] = Dn.qr[(size_t)(i + j * n)];
        }
      dense_explicit_ops(Dn);  // Q^H (and R^{-1}, unused here)
      if (adjoint) {  // _multiply_t needs Q^H and R^H
        dn.QH.upload(mfma_operand(Dn.QH.data(), n, n));
        dn.Rm.upload(mfma_operand(Rm.data(), n, n));
      } else {  // _multiply_nt needs R and Q
        dense_adjoint_ops(Dn);
        dn.Qm.upload(mfma_operand(Dn.Q.data(), n, n));
        dn.Rm.upload(mfma_operand(Rm.data(), n, n));
        if (!dn.tmp2.p) dn.tmp2.alloc((size_t)n * Rmax * sizeof(T));
      }
      std::vector<T>().swap(Dn.QH);
      std::vector<T>().swap(Dn.Rinv);
      std::vector<T>().swap(Dn.Q);
      std::vector<T>().swap(Dn.RinvH);
    }
    HIP_OK(hipStreamSynchronize(stream));  // (transfers were synchronous on the transfer stream)
    prod_ready = true;
  }

  // dense last level of the product: QRCP::_multiply_nt (QRCP.hpp:460-495) z = Q(:,1:rk) R(1:rk,1:rk) (P^T c)(1:rk);
  // on the adjoint engine QRCP::_multiply_t (:502-541) z[jpvt] = R^H (Q^H c)(1:rk)
  void launch_dense_mul(hipStream_t st, const D *cin, D *zout, int logR, int64_t rank, int64_t &count) {
    const int nd = (int)dn.n, rk = (int)eff_rank(rank);
    D *tmp = dn.tmp.as<D>();
    if (dn.lup) {  // LUP::multiply (LUP.hpp:181-188): z = A c (adjoint engine: A^H c)
      zgemm(st, nd, nd, nd, 0, dn.Rm, nd, cin, logR, nullptr, zout, nullptr, nullptr, count);
      return;
    }
    if (dn.symm) {  // SYEIG::multiply (SYEIG.hpp:256-273): z = V(:,to(1:rk)) diag(w) V(:,to(1:rk))^H c
      zgemm(st, nd, rk, nd, 0, dn.Rm, nd, cin, logR, nullptr, tmp, nullptr, nullptr, count);
      zgemm(st, nd, nd, rk, 0, dn.Qm, nd, tmp, logR, nullptr, zout, nullptr, nullptr, count);
      return;
    }
    if (adjoint) {
      zgemm(st, nd, rk, nd, 0, dn.QH, nd, cin, logR, nullptr, tmp, nullptr, nullptr, count);
      zgemm(st, nd, rk, rk, 2, dn.Rm, nd, tmp, logR, dn.jpvt0.as<int32_t>(), zout, nullptr, nullptr, count);
      return;
    }
    D *tmp2 = dn.tmp2.as<D>();
    row_gather(st, cin, dn.jpvt0.as<int32_t>(), nd, tmp2, logR, count);
    zgemm(st, nd, rk, rk, 1, dn.Rm, nd, tmp2, logR, nullptr, tmp, nullptr, nullptr, count);
    zgemm(st, nd, nd, rk, 0, dn.Qm, nd, tmp, logR, nullptr, zout, nullptr, nullptr, count);
  }

  void enqueue_prod_level(hipStream_t st, size_t l, InP bin, int64_t ldb, OutP yout, int64_t ldy, int nrhs,
                          int logR, int64_t rank, int64_t &count) {
    DevLevel &L = *lv[l];
    const int64_t m = L.m, n = L.n, nm = n - m;
    const int64_t R = 1LL << logR;
    D *w = L.w.as<D>(), *v = L.v.as<D>(), *g = L.pg.as<D>(), *cy = L.pc.as<D>(), *r = L.pr.as<D>();
    const bool last = (l + 1 == lv.size());
    cur_level = (int)l;
    // g = b[q] / t[q], all n rows  (:76, :97)
    tally(KF_PROD);
    hipLaunchKernelGGL((k_gather_div<D>), dim3(grid_for(n, logR)), dim3(256), 0, st, bin, ldb, nrhs, L.q.as<int32_t>(),
                       L.t.as<double>(), n, g, logR);
    ++count;
    if (nm) {  // the Schur complement's product -> cy[m:n]  (:80-93)
      if (last)
        launch_dense_mul(st, g + m * R, cy + m * R, logR, rank, count);
      else
        enqueue_prod_level(st, l + 1, in_direct(g + m * R), R, out_direct(cy + m * R), R, (int)R, logR, rank, count);
      cur_level = (int)l;
    }
    if (m) {
      // cy[0:m] = D (U + I) g   (:101-103);  r[0:m] = (L + I) cy   (:106-108)
      tally(KF_PROD, 2);
      hipLaunchKernelGGL((k_prod_rows<D, true>), dim3(grid_for(m, logR)), dim3(256), 0, st, m, L.U.ptr.as<int32_t>(),
                         L.U.col.as<int32_t>(), L.U.val.as<D>(), L.U.rowid.as<int32_t>(), (const D *)g, L.d.as<D>(), cy,
                         logR);
      hipLaunchKernelGGL((k_prod_rows<D, false>), dim3(grid_for(m, logR)), dim3(256), 0, st, m, L.L.ptr.as<int32_t>(),
                         L.L.col.as<int32_t>(), L.L.val.as<D>(), L.L.rowid.as<int32_t>(), (const D *)cy,
                         (const D *)nullptr, r, logR);
      count += 2;
      if (L.F_ncols) {  // w = F g[m:n]; r += w   (:112-115)
        tally(KF_PROD);
        hipLaunchKernelGGL((k_spmm_prod<D, 0>), dim3(grid_for(m, logR)), dim3(256), 0, st, m, L.F.ptr.as<int32_t>(),
                           L.F.col.as<int32_t>(), L.F.val.as<D>(), (const D *)(g + m * R), w, r, (const D *)nullptr, logR);
        ++count;
      } else if (nm) {  // no F: the reference's y(1:m) still holds D(U+I)g when the solve below reads it (:121)
        tally(KF_PROD);
        hipLaunchKernelGGL((k_vec_op<D>), dim3(vec_grid(m * R)), dim3(256), 0, st, 1, m, (int)R, w, R, (const D *)cy, R,
                           (const D *)nullptr, (int64_t)0);
        ++count;
      }
    }
    if (nm) {
      if (m) {
        launch_ldu(st, L, logR, count);  // v = (LDU)^{-1} w   (:121)
        tally(KF_PROD);
        hipLaunchKernelGGL((k_vec_op<D>), dim3(vec_grid(m * R)), dim3(256), 0, st, 2, m, (int)R, v, R, (const D *)g, R,
                           (const D *)nullptr, (int64_t)0);  // v += g   (:123)
        ++count;
      }
      if (L.E_void) {
        // transposed product of a level WITHOUT F: the reference's F.multiply_t_low writes F.ncols() = 0
        // entries (prec_prod.hpp:223), so work[m:n] still holds the permuted input when y[m:n] is added
        // (:225) -- reproduced literally (no factorization yields such a level; synthetic tests do)
        tally(KF_PROD);
        hipLaunchKernelGGL((k_vec_op<D>), dim3(vec_grid(nm * R)), dim3(256), 0, st, 3, nm, (int)R, r + m * R, R,
                           (const D *)(g + m * R), R, (const D *)(cy + m * R), R);
      } else {
        // r[m:n] = E v + cy[m:n]   (:125-127)
        tally(KF_PROD);
        hipLaunchKernelGGL((k_spmm_prod<D, 1>), dim3(grid_for(nm, logR)), dim3(256), 0, st, nm, L.E.ptr.as<int32_t>(),
                           L.E.col.as<int32_t>(), L.E.val.as<D>(), (const D *)v, r + m * R, (D *)nullptr,
                           (const D *)(cy + m * R), logR);
      }
      ++count;
    }
    // y = r[p_inv] / s   (:132)
    tally(KF_PROD);
    hipLaunchKernelGGL((k_scatter_div<D>), dim3(grid_for(n, logR)), dim3(256), 0, st, (const D *)r, L.pinv.as<int32_t>(),
                       L.s.as<double>(), n, yout, ldy, nrhs, logR);
    ++count;
  }
  static unsigned vec_grid(int64_t elems) {
    int64_t g = (elems + 255) / 256;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    return (unsigned)g;
  }

  // all kernels of one batched apply, nrhs tiled by 64 columns
  // `slots` (device: {B base, X base}) != NULL: the level-0 kernels read the caller's pointers from there
  int64_t enqueue_apply(hipStream_t st, const D *dB, int64_t ldb, D *dX, int64_t ldx, int64_t nrhs, int64_t rank,
                        int kind = 0, D *const *slots = nullptr, int tfirst = 0, int tstride = 1) {
    int64_t count = 0;
    cur_map.clear();
    cur_census.fill(0);
    for (int64_t c0 = 64 * (int64_t)tfirst; c0 < nrhs; c0 += 64 * (int64_t)tstride) {
      const int64_t nc = std::min<int64_t>(64, nrhs - c0);
      const int logR = pick_logR(nc);
      act_cols = (int)nc;
      const InP bin = slots ? InP{nullptr, (const D *const *)slots, c0} : in_direct(dB + c0);
      const OutP yout = slots ? OutP{nullptr, slots + 1, c0} : out_direct(dX + c0);
      if (kind == 0)
        enqueue_level(st, 0, bin, ldb, yout, ldx, (int)nc, logR, rank, count);
      else
        enqueue_prod_level(st, 0, bin, ldb, yout, ldx, (int)nc, logR, rank, count);
    }
    HIP_OK(hipGetLastError());
    return count;
  }

  void check_batch(const void *B, int64_t ldb, const void *X, int64_t ldx, int64_t nrhs) const {
    if (!finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
    if (!B || !X) throw Error(HIFAMD_NULL_OBJ, "NULL vector");
    if (nrhs < 1) throw Error(HIFAMD_MISMATCHED_SIZES, "nrhs must be >= 1");
    if (ldb < nrhs || ldx < nrhs) throw Error(HIFAMD_MISMATCHED_SIZES, "row stride smaller than nrhs");
    if (std::min<int64_t>(nrhs, 64) > std::max<int64_t>(Rmax, max_nrhs))
      throw Error(HIFAMD_MISMATCHED_SIZES, "batch wider than the max_nrhs given to hifamd_finalize");
    if (B == X) throw Error(HIFAMD_BAD_PREC, "b and x must not alias");
  }

  // graph-cached batched apply on device pointers
  void solve_dev(const D *dB, int64_t ldb, D *dX, int64_t ldx, int64_t nrhs, int64_t rank, hipStream_t user,
                 int kind = 0) {
    check_batch(dB, ldb, dX, ldx, nrhs);
    HIP_OK(hipSetDevice(device));
#ifdef HIFAMD_CSPROBE
    if (csprobe.p) {  // (development build: the dump holds the LAST apply only)
      HIP_OK(hipStreamSynchronize(user ? user : stream));
      csprobe_reset();
    }
#endif
    if (kind == 1) ensure_prod_buffers();
    hipStream_t st = user ? user : stream;
    const int ntiles = (int)((nrhs + 63) / 64);
    const int nl = std::min(ntiles, 1 + std::max(0, opt.use_twin));  // lanes: this engine + its twins
    if (nl > 1 && !is_twin) {  // tile t runs on lane t % nl, all lanes in flight
      if (!ev_fork) HIP_OK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
      HIP_OK(hipEventRecord(ev_fork, st));
      launch_part(dB, ldb, dX, ldx, nrhs, rank, st, kind, 0, nl);
      int64_t total = last_launches;
      for (int k = 1; k < nl; ++k) {
        Engine<T> &Tw = twin_engine(k - 1);
        if (kind == 1) Tw.ensure_prod_buffers_as_twin(*this);
        HIP_OK(hipStreamWaitEvent(Tw.stream, ev_fork, 0));
        Tw.launch_part(dB, ldb, dX, ldx, nrhs, rank, Tw.stream, kind, k, nl);
        HIP_OK(hipEventRecord(ev_join[(size_t)(k - 1)], Tw.stream));
        HIP_OK(hipStreamWaitEvent(st, ev_join[(size_t)(k - 1)], 0));
        total += Tw.last_launches;
        for (size_t f = 0; f < last_census.size(); ++f) last_census[f] += Tw.last_census[f];
      }
      last_launches = total;
      census_seq = ++census_clock();
      if (kind == 0) apply_nsp(dX, ldx, nrhs, st);
      return;
    }
    launch_part(dB, ldb, dX, ldx, nrhs, rank, st, kind, 0, 1);
    census_seq = ++census_clock();
    if (kind == 0) apply_nsp(dX, ldx, nrhs, st);
  }

  // builder.hpp:419-422: after the solve, x loses its component along the (constant) null space
  void apply_nsp(D *dX, int64_t ldx, int64_t nrhs, hipStream_t st) {
    if (nsp_k > 0) return apply_nsp_basis(dX, ldx, nrhs, st);
    if (!nsp_on) return;
    const int64_t n = lv[0]->n;
    const int64_t r0 = nsp_r0, r1 = (nsp_r1 < 0 || nsp_r1 < nsp_r0) ? n : nsp_r1;  // NspFilter.hpp:163-167
    if (r1 > n) throw Error(HIFAMD_MISMATCHED_SIZES, "null-space filter range exceeds the system size");
    if (r0 == r1) return;
    const int nblk = 256;
    if (nsp_part.bytes < (size_t)nblk * 64 * sizeof(T)) nsp_part.alloc((size_t)nblk * 64 * sizeof(T));
    for (int64_t c0 = 0; c0 < nrhs; c0 += 64) {
      const int nc = (int)std::min<int64_t>(64, nrhs - c0);
      hipLaunchKernelGGL((k_colsum_partial<D>), dim3(nblk), dim3(256), 0, st, r0, r1, nc, (const D *)(dX + c0), ldx,
                         nsp_part.as<D>());
      hipLaunchKernelGGL((k_sub_colmean<D>), dim3(vec_grid((r1 - r0) * nc)), dim3(256), 0, st, r0, r1, nc, dX + c0, ldx,
                         (const D *)nsp_part.as<D>(), nblk);
    }
  }

  // basis mode: x -= Q (Q^H x) per 64-column tile -- block partials of Q^H X, one workgroup per basis vector adds them,
  // then the update (kernels.hip.hpp k_nsp_*; reduction order fixed by n alone)
  template <int K>
  void launch_nsp_basis(D *x, int64_t ldx, int nc, hipStream_t st) {
    const int64_t n = lv[0]->n;
    const D *Q = nsp_Q.as<D>();
    D *part = nsp_cpart.as<D>(), *C = nsp_C.as<D>();
    hipLaunchKernelGGL((k_nsp_coef<D, K>), dim3(kCgBlocks), dim3(256), 0, st, n, nc, (const D *)x, ldx, Q, part);
    hipLaunchKernelGGL((k_nsp_finish<D>), dim3(K), dim3(1024), 0, st, (const D *)part, C);
    hipLaunchKernelGGL((k_nsp_sub<D, K>), dim3(kCgBlocks), dim3(256), 0, st, n, nc, x, ldx, Q, (const D *)C);
  }
  void apply_nsp_basis(D *dX, int64_t ldx, int64_t nrhs, hipStream_t st) {
    for (int64_t c0 = 0; c0 < nrhs; c0 += 64) {
      const int nc = (int)std::min<int64_t>(64, nrhs - c0);
      switch (nsp_kp) {
        case 1: launch_nsp_basis<1>(dX + c0, ldx, nc, st); break;
        case 2: launch_nsp_basis<2>(dX + c0, ldx, nc, st); break;
        case 4: launch_nsp_basis<4>(dX + c0, ldx, nc, st); break;
        case 8: launch_nsp_basis<8>(dX + c0, ldx, nc, st); break;
        case 16: launch_nsp_basis<16>(dX + c0, ldx, nc, st); break;
        default: throw Error(HIFAMD_HIFIR_ERROR, "internal error: null-space basis of an unsupported padded size");
      }
    }
    HIP_OK(hipGetLastError());
  }

  // hifamd_set_nsp_basis on this engine: orthonormalize on the host (import.hpp), ship Q, size the reduction buffers
  void set_nsp_basis(int64_t k, const T *V, int64_t ldv) {
    if (!finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
    HIP_OK(hipSetDevice(device));
    if (k == 0) {
      nsp_k = nsp_kp = 0;
      for (DevBuf *b : {&nsp_Q, &nsp_cpart, &nsp_C}) b->release();
      return;
    }
    const int64_t kp = nsp_padded(k);
    const std::vector<T> Q = nsp_orthonormalize<T>(lv[0]->n, k, V, ldv, kp);
    nsp_k = nsp_kp = 0;
    nsp_Q.upload(Q);
    nsp_cpart.alloc((size_t)kp * kCgBlocks * 64 * sizeof(T));
    nsp_C.alloc((size_t)kp * 64 * sizeof(T));
    nsp_k = (int)k, nsp_kp = (int)kp;
    nsp_on = false;  // one filter per op
  }

  // the filter alone, in place (hifamd_nsp_filter_batch / _dev)
  void nsp_filter_dev(D *dX, int64_t ldx, int64_t nrhs, hipStream_t user) {
    if (!finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
    if (!dX) throw Error(HIFAMD_NULL_OBJ, "NULL vector");
    if (nrhs < 1) throw Error(HIFAMD_MISMATCHED_SIZES, "nrhs must be >= 1");
    if (ldx < nrhs) throw Error(HIFAMD_MISMATCHED_SIZES, "row stride smaller than nrhs");
    HIP_OK(hipSetDevice(device));
    apply_nsp(dX, ldx, nrhs, user ? user : stream);
  }
  void nsp_filter_host(T *X, int64_t ldx, int64_t nrhs) {
    if (!finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
    if (!X) throw Error(HIFAMD_NULL_OBJ, "NULL vector");
    if (nrhs < 1) throw Error(HIFAMD_MISMATCHED_SIZES, "nrhs must be >= 1");
    if (ldx < nrhs) throw Error(HIFAMD_MISMATCHED_SIZES, "row stride smaller than nrhs");
    if (!nsp_on && nsp_k == 0) return;
    HIP_OK(hipSetDevice(device));
    const int64_t n = lv[0]->n;
    const size_t need = (size_t)n * nrhs * sizeof(T);
    if (stage_x.bytes < need) stage_x.alloc(need);
    HIP_OK(hipMemcpy2DAsync(stage_x.p, nrhs * sizeof(T), X, ldx * sizeof(T), nrhs * sizeof(T), n, hipMemcpyHostToDevice, stream));
    apply_nsp(stage_x.as<D>(), nrhs, nrhs, stream);
    HIP_OK(hipMemcpy2DAsync(X, ldx * sizeof(T), stage_x.p, nrhs * sizeof(T), nrhs * sizeof(T), n, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    check_device_error();
  }

  // ---- null-space search (hifamd_nsp_find) on this engine: null(A) on the primary, null(A^H) on the adjoint --------
  // B = -A X0 lies in range(A), so A D = B is consistent; D = gmres_dev(B) to rtol; V = X0 + D has ||A v|| <= rtol
  // ||A x0|| per column and numerical rank = nullity.  Then, on 16 x 16 matrices (import.hpp): G = V^H V, rotation +
  // scaling by its eigendecomposition (columns ordered by weight), and TWICE the order-preserving Cholesky step (a
  // second eigendecomposition of G ~ I would rotate the null vectors into the other columns).  Accepted by the
  // definition: res_j = ||A q_j||_2 <= tol ||A||_inf, the leading prefix, at most kmax.  Three [n][16] blocks live
  // for the duration of the call only.  The filter in force is suspended (GMRES's applies would project the sought
  // component away) and put back on every exit.
  struct NspSuspend {
    Engine<T> &E;
    bool on;
    int k, kp;
    explicit NspSuspend(Engine<T> &e) : E(e), on(e.nsp_on), k(e.nsp_k), kp(e.nsp_kp) { e.nsp_on = false, e.nsp_k = e.nsp_kp = 0; }
    ~NspSuspend() { E.nsp_on = on, E.nsp_k = k, E.nsp_kp = kp; }
  };
  // G[j * 64 + c] = v_j^H v_c of V [n][16]: the filter's reduction with Q = X = V (fixed order), read back
  void nsp_gram(const D *V, D *part, D *C, std::vector<T> &G) {
    const int64_t n = lv[0]->n;
    hipLaunchKernelGGL((k_nsp_coef<D, kNspMax>), dim3(kCgBlocks), dim3(256), 0, stream, n, kNspMax, V, (int64_t)kNspMax, V, part);
    hipLaunchKernelGGL((k_nsp_finish<D>), dim3(kNspMax), dim3(1024), 0, stream, (const D *)part, C);
    HIP_OK(hipGetLastError());
    const T *g = read_back<T>(C, (size_t)kNspMax * 64);
    G.assign(g, g + (size_t)kNspMax * 64);
  }
  // V <- V M for a host 16 x 16 row-major M (the stream is idle when M's device copy is overwritten: nsp_gram synchronized)
  void nsp_rmul(D *V, const std::vector<T> &M, D *dM) {
    const int64_t n = lv[0]->n;
    HIP_OK(hipMemcpyAsync(dM, M.data(), (size_t)kNspMax * kNspMax * sizeof(T), hipMemcpyHostToDevice, stream));
    HIP_OK(hipStreamSynchronize(stream));
    const int64_t g = std::min<int64_t>((n + 15) / 16, 4096);
    hipLaunchKernelGGL((k_blk_rmul<D>), dim3((unsigned)std::max<int64_t>(g, 1)), dim3(256), 0, stream, n, V, (const D *)dM);
    HIP_OK(hipGetLastError());
  }
  void nsp_find(int64_t kmax, double tol, double rtol, int restart, int maxit, int64_t rank, const T *X0, int64_t ldx0,
                uint64_t seed, bool install, int64_t *found, T *Qout, int64_t ldq, double *resid16, int *info4) {
    if (!finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
    if (!has_A) throw Error(HIFAMD_BAD_PREC, "the null-space search needs the matrix (hifamd_set_matrix)");
    HIP_OK(hipSetDevice(device));
    const int64_t n = lv[0]->n;
    const int K = kNspMax;
    *found = 0;
    NspSuspend guard(*this);
    DevBuf bV, bB, bD, bPart, bC, bM;
    const size_t blk = (size_t)n * K * sizeof(T);
    bV.alloc(blk), bB.alloc(blk), bD.alloc(blk);
    bPart.alloc((size_t)K * kCgBlocks * 64 * sizeof(T)), bC.alloc((size_t)K * 64 * sizeof(T)), bM.alloc((size_t)K * K * sizeof(T));
    D *V = bV.as<D>(), *B = bB.as<D>(), *Dx = bD.as<D>();
    if (X0) {
      HIP_OK(hipMemcpy2DAsync(V, K * sizeof(T), X0, ldx0 * sizeof(T), K * sizeof(T), n, hipMemcpyHostToDevice, stream));
    } else {
      hipLaunchKernelGGL((k_probe_fill<D>), dim3(vec_grid(n * K)), dim3(256), 0, stream, n, seed, V);
    }
    vec_op(0, n, K, Dx, K, nullptr, 0, nullptr, 0);
    resid_dev((const D *)Dx, K, (const D *)V, K, B, K, K, 0);  // B = 0 - A X0, in working precision whatever the mode
    std::vector<int> flags((size_t)K, 0), iters((size_t)K, 0);
    gmres_dev((const D *)B, K, Dx, K, K, restart, rtol, maxit, rank, flags.data(), iters.data());
    vec_op(2, n, K, V, K, (const D *)Dx, K, nullptr, 0);  // V = X0 + D
    bool finite = true;
    std::vector<T> G, M((size_t)K * K);
    std::vector<double> w((size_t)K);
    nsp_gram(V, bPart.as<D>(), bC.as<D>(), G);
    finite = finite && nsp_gram_finite(G.data(), 64);
    int cand = nsp_find_rotation<T>(G.data(), 64, M.data(), w.data());
    nsp_rmul(V, M, bM.as<D>());
    for (int pass = 0; pass < 2; ++pass) {
      nsp_gram(V, bPart.as<D>(), bC.as<D>(), G);
      finite = finite && nsp_gram_finite(G.data(), 64);
      cand = std::min(cand, nsp_chol_inverse<T>(G.data(), 64, M.data()));
      nsp_rmul(V, M, bM.as<D>());
    }
    spmv_dev((const D *)V, K, B, K, K, nullptr);  // B = A Q
    std::vector<double> res;
    col_norms(B, K, n, K, res);
    check_device_error();
    std::vector<double> rel((size_t)K);
    for (int j = 0; j < K; ++j) {
      rel[(size_t)j] = A_norm_inf > 0.0 ? res[(size_t)j] / A_norm_inf : res[(size_t)j];
      if (j < cand && !std::isfinite(rel[(size_t)j])) finite = false;
      if (j >= cand) rel[(size_t)j] = std::numeric_limits<double>::infinity();  // a dropped candidate (a zero column) is no null vector
    }
    int64_t nacc = 0;
    while (nacc < cand && rel[(size_t)nacc] <= tol) ++nacc;
    if (!finite) nacc = 0;
    const int64_t k = std::min<int64_t>(nacc, kmax);
    if (resid16) std::copy(rel.begin(), rel.end(), resid16);
    if (info4) {
      info4[0] = info4[1] = 0;
      for (int j = 0; j < K; ++j) info4[0] += flags[(size_t)j] != 0, info4[1] = std::max(info4[1], iters[(size_t)j]);
      info4[2] = (nacc > kmax || k == K) ? 1 : 0;
      info4[3] = finite ? 0 : 1;
    }
    if (k > 0 && Qout) {
      HIP_OK(hipMemcpy2DAsync(Qout, ldq * sizeof(T), V, K * sizeof(T), (size_t)k * sizeof(T), n, hipMemcpyDeviceToHost, stream));
      HIP_OK(hipStreamSynchronize(stream));
    }
    if (k > 0 && install) {
      // the columns are orthonormal already: no host round trip.  Everything that can fail happens on local buffers;
      // the engine's are exchanged last
      const int64_t kp = nsp_padded(k);
      DevBuf nQ, nPart, nC;
      nQ.alloc((size_t)n * kp * sizeof(T)), nPart.alloc((size_t)kp * kCgBlocks * 64 * sizeof(T)), nC.alloc((size_t)kp * 64 * sizeof(T));
      HIP_OK(hipMemsetAsync(nQ.p, 0, nQ.bytes, stream));
      HIP_OK(hipMemcpy2DAsync(nQ.p, kp * sizeof(T), V, K * sizeof(T), (size_t)k * sizeof(T), n, hipMemcpyDeviceToDevice, stream));
      HIP_OK(hipStreamSynchronize(stream));
      auto exchange = [](DevBuf &a, DevBuf &b) { std::swap(a.p, b.p), std::swap(a.bytes, b.bytes), std::swap(a.owner, b.owner); };
      exchange(nsp_Q, nQ), exchange(nsp_cpart, nPart), exchange(nsp_C, nC);
      guard.on = false, guard.k = (int)k, guard.kp = (int)kp;  // one filter per op
    }
    *found = k;
  }
  // hifamd_nsp_get_basis: the nsp_k columns of the basis in force, [n][nsp_k] into Q (row stride ldq)
  int64_t nsp_get_basis(T *Q, int64_t ldq) {
    if (nsp_k == 0) return 0;
    if (!Q || ldq < nsp_k) return -1;
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipMemcpy2DAsync(Q, ldq * sizeof(T), nsp_Q.p, nsp_kp * sizeof(T), (size_t)nsp_k * sizeof(T), lv[0]->n, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    return nsp_k;
  }

  void launch_part(const D *dB, int64_t ldb, D *dX, int64_t ldx, int64_t nrhs, int64_t rank, hipStream_t st, int kind,
                   int tfirst, int tstride) {
    if (!opt.use_graph) {
      last_launches = enqueue_apply(st, dB, ldb, dX, ldx, nrhs, rank, kind, nullptr, tfirst, tstride);
      last_map = cur_map;
      last_census = cur_census;
      return;
    }
    std::lock_guard<std::mutex> graph_lock(graph_mutex());
    GraphKey key{ldb, ldx, nrhs, host.has_dense ? eff_rank(rank) : 0, kind, tfirst, tstride};
    auto it = graphs.find(key);
    if (it == graphs.end()) {
      if (graphs.size() >= 8) {  // evict the least recently used
        auto old = graphs.begin();
        for (auto jt = graphs.begin(); jt != graphs.end(); ++jt)
          if (jt->second.stamp < old->second.stamp) old = jt;
        HIP_OK(hipStreamSynchronize(stream));
        (void)hipGraphExecDestroy(old->second.exec);
        (void)hipGraphDestroy(old->second.graph);
        (void)hipFree(old->second.slots);
        graphs.erase(old);
      }
      GraphEntry ge;
      const auto t_cap0 = std::chrono::steady_clock::now();
      HIP_OK(hipMalloc((void **)&ge.slots, 2 * sizeof(void *)));
      HIP_OK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
      try {
        ge.launches = enqueue_apply(stream, dB, ldb, dX, ldx, nrhs, rank, kind, (D *const *)ge.slots, tfirst, tstride);
        ge.map = cur_map;
        ge.census = cur_census;
      } catch (...) {
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(stream, &g);
        if (g) (void)hipGraphDestroy(g);
        (void)hipFree(ge.slots);
        throw;
      }
      HIP_OK(hipStreamEndCapture(stream, &ge.graph));
      HIP_OK(hipGraphInstantiate(&ge.exec, ge.graph, nullptr, nullptr, 0));
      capture_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_cap0).count();
      it = graphs.emplace(key, ge).first;
    }
    it->second.stamp = ++clock;
    last_launches = it->second.launches;
    last_map = it->second.map;
    last_census = it->second.census;
    // hand this call's pointers to the graph: a stream-ordered 16-byte copy from a pinned ring slot
    if (!io_ring) HIP_OK(hipHostMalloc((void **)&io_ring, kIoRing * 2 * sizeof(void *), hipHostMallocDefault));
    if (io_next && io_next % kIoRing == 0) HIP_OK(hipStreamSynchronize(st));  // never overtake a pending slot
    void **h = io_ring + 2 * (io_next++ % kIoRing);
    h[0] = (void *)dB;
    h[1] = (void *)dX;
    HIP_OK(hipMemcpyAsync(it->second.slots, h, 2 * sizeof(void *), hipMemcpyHostToDevice, st));
    HIP_OK(hipGraphLaunch(it->second.exec, st));
  }

  struct StreamWait {  // waits for the stream on every way out of a scope that enqueued work
    hipStream_t s;
    ~StreamWait() { (void)hipStreamSynchronize(s); }
  };
  // The host-pointer form of a batched entry: B [n][nrhs] (row stride ldb) is staged on the device, run(dB, dX) works
  // on the staged blocks (row stride nrhs), and X (row stride ldx) comes back.  pre() holds what must refuse the call
  // before anything is enqueued.  The stream is drained on every way out: when run() throws, no copy is left reading
  // the caller's B.  sticky: also report the band kernels' error word (the solvers' tiles have done so themselves).
  template <class Pre, class Run>
  void staged(const T *B, int64_t ldb, T *X, int64_t ldx, int64_t nrhs, bool sticky, Pre pre, Run run) {
    check_batch(B, ldb, X, ldx, nrhs);
    pre();
    HIP_OK(hipSetDevice(device));
    const int64_t n = lv[0]->n;
    const size_t need = (size_t)n * nrhs * sizeof(T);
    if (stage_b.bytes < need) stage_b.alloc(need);
    if (stage_x.bytes < need) stage_x.alloc(need);
    StreamWait wait{stream};
    HIP_OK(hipMemcpy2DAsync(stage_b.p, nrhs * sizeof(T), B, ldb * sizeof(T), nrhs * sizeof(T), n,
                            hipMemcpyHostToDevice, stream));
    run((const D *)stage_b.as<D>(), stage_x.as<D>());
    HIP_OK(hipMemcpy2DAsync(X, ldx * sizeof(T), stage_x.p, nrhs * sizeof(T), nrhs * sizeof(T), n,
                            hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    if (sticky) check_device_error();
  }

  void solve_host(const T *B, int64_t ldb, T *X, int64_t ldx, int64_t nrhs, int64_t rank) {
    staged(B, ldb, X, ldx, nrhs, true, [] {}, [&](const D *b, D *x) { solve_dev(b, nrhs, x, nrhs, nrhs, rank, nullptr); });
  }

  // ---- SpMV + iterative refinement -----------------------------------------------------------
  void spmv_dev(const D *dX, int64_t ldx, D *dY, int64_t ldy, int64_t nrhs, hipStream_t user) {
    if (!finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
    if (!has_A) throw Error(HIFAMD_BAD_PREC, "no matrix attached (hifamd_set_matrix)");
    if (!dX || !dY) throw Error(HIFAMD_NULL_OBJ, "NULL vector");
    HIP_OK(hipSetDevice(device));
    spmm_launch(A, dX, ldx, dY, ldy, nrhs, user ? user : stream);
  }
  // Y = B X with the mass matrix (set_mass_matrix), as spmv_dev runs it on A
  void spmv_mass_dev(const D *dX, int64_t ldx, D *dY, int64_t ldy, int64_t nrhs, hipStream_t user) {
    if (!finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
    if (!has_B) throw Error(HIFAMD_BAD_PREC, "no mass matrix attached (hifamd_set_mass_matrix)");
    if (!dX || !dY) throw Error(HIFAMD_NULL_OBJ, "NULL vector");
    HIP_OK(hipSetDevice(device));
    spmm_launch(Bm, dX, ldx, dY, ldy, nrhs, user ? user : stream);
  }
  void spmm_launch(const DevCsr &C, const D *dX, int64_t ldx, D *dY, int64_t ldy, int64_t nrhs, hipStream_t st) {
    for (int64_t c0 = 0; c0 < nrhs; c0 += 64) {
      const int nc = (int)std::min<int64_t>(64, nrhs - c0);
      const int logR = pick_logR(nc);
      hipLaunchKernelGGL((k_crs_spmm<D, false>), dim3(grid_for(C.nrows, logR)), dim3(256), 0, st, C.nrows,
                         C.ptr.as<int32_t>(), C.col.as<int32_t>(), C.val.as<D>(), dX + c0, ldx, (const D *)nullptr,
                         (int64_t)0, dY + c0, ldy, nc, logR);
    }
    HIP_OK(hipGetLastError());
  }

  // r = b - A x; mode 0: in working precision, mode 1: compensated (k_crs_resid_dd)
  void resid_dev(const D *dB, int64_t ldb, const D *dX, int64_t ldx, D *dR, int64_t ldr, int64_t nrhs, int mode,
                 hipStream_t user = nullptr) {
    hipStream_t st = user ? user : stream;
    for (int64_t c0 = 0; c0 < nrhs; c0 += 64) {
      const int nc = (int)std::min<int64_t>(64, nrhs - c0);
      const int logR = pick_logR(nc);
      if (mode == 1)  // (requests two nonzeros ahead: four and eight measured slower)
        hipLaunchKernelGGL((k_crs_resid_dd<D, 2>), dim3(grid_for(A.nrows, logR)), dim3(256), 0, st, A.nrows,
                           A.ptr.as<int32_t>(), A.col.as<int32_t>(), A.val.as<D>(), dX + c0, ldx, dB + c0, ldb,
                           dR + c0, ldr, nc, logR);
      else
        hipLaunchKernelGGL((k_crs_spmm<D, true>), dim3(grid_for(A.nrows, logR)), dim3(256), 0, st, A.nrows,
                           A.ptr.as<int32_t>(), A.col.as<int32_t>(), A.val.as<D>(), dX + c0, ldx, dB + c0, ldb,
                           dR + c0, ldr, nc, logR);
    }
    HIP_OK(hipGetLastError());
  }

  // hifamd_residual_batch(_dev) on this engine (the adjoint engine: r = b - A^H x); mode -1: the handle's
  void residual_check(const void *B, int64_t ldb, const void *X, int64_t ldx, const void *R, int64_t ldr, int64_t nrhs) const {
    if (!finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
    if (!has_A) throw Error(HIFAMD_BAD_PREC, "the residual needs the matrix (hifamd_set_matrix)");
    if (!B || !X || !R) throw Error(HIFAMD_NULL_OBJ, "NULL vector");
    if (nrhs < 1) throw Error(HIFAMD_MISMATCHED_SIZES, "nrhs must be >= 1");
    if (ldb < nrhs || ldx < nrhs || ldr < nrhs) throw Error(HIFAMD_MISMATCHED_SIZES, "row stride smaller than nrhs");
    if (R == B || R == X) throw Error(HIFAMD_BAD_PREC, "r must not alias b or x");
  }
  void residual_dev(const D *dB, int64_t ldb, const D *dX, int64_t ldx, D *dR, int64_t ldr, int64_t nrhs, int mode,
                    hipStream_t user) {
    residual_check(dB, ldb, dX, ldx, dR, ldr, nrhs);
    HIP_OK(hipSetDevice(device));
    resid_dev(dB, ldb, dX, ldx, dR, ldr, nrhs, mode < 0 ? opt.resid_mode : mode, user);
  }
  DevBuf stage_r;
  void residual_host(const T *B, int64_t ldb, const T *X, int64_t ldx, T *R, int64_t ldr, int64_t nrhs, int mode) {
    residual_check(B, ldb, X, ldx, R, ldr, nrhs);
    HIP_OK(hipSetDevice(device));
    const int64_t n = lv[0]->n;
    const size_t row = (size_t)nrhs * sizeof(T), need = (size_t)n * row;
    if (stage_b.bytes < need) stage_b.alloc(need);
    if (stage_x.bytes < need) stage_x.alloc(need);
    if (stage_r.bytes < need) stage_r.alloc(need);
    StreamWait wait{stream};
    HIP_OK(hipMemcpy2DAsync(stage_b.p, row, B, ldb * sizeof(T), row, n, hipMemcpyHostToDevice, stream));
    HIP_OK(hipMemcpy2DAsync(stage_x.p, row, X, ldx * sizeof(T), row, n, hipMemcpyHostToDevice, stream));
    resid_dev((const D *)stage_b.as<D>(), nrhs, (const D *)stage_x.as<D>(), nrhs, stage_r.as<D>(), nrhs, nrhs,
              mode < 0 ? opt.resid_mode : mode);
    HIP_OK(hipMemcpy2DAsync(R, ldr * sizeof(T), stage_r.p, row, row, n, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
  }

  void vec_op(int op, int64_t n, int64_t nrhs, D *y, int64_t ldy, const D *x, int64_t ldx, const D *z, int64_t ldz) {
    hipLaunchKernelGGL((k_vec_op<D>), dim3(vec_grid(n * nrhs)), dim3(256), 0, stream, op, n, (int)nrhs, y, ldy, x, ldx, z, ldz);
  }

  // per-column 2-norms of an [n][nrhs] block (nrhs <= 64 per pass); result on the host
  void col_norms(const D *x, int64_t ldx, int64_t n, int64_t nrhs, std::vector<double> &out) {
    out.assign((size_t)nrhs, 0.0);
    const int nblk = 512;
    if (ir_part.bytes < (size_t)nblk * 64 * sizeof(double)) ir_part.alloc((size_t)nblk * 64 * sizeof(double));
    for (int64_t c0 = 0; c0 < nrhs; c0 += 64) {
      const int nc = (int)std::min<int64_t>(64, nrhs - c0);
      hipLaunchKernelGGL((k_colnorm2_partial<D>), dim3(nblk), dim3(256), 0, stream, n, nc, x + c0, ldx,
                         ir_part.as<double>());
      const double *part = read_back<double>(ir_part.p, (size_t)nblk * nc);
      for (int c = 0; c < nc; ++c) {
        double tot = 0.0;
        for (int b = 0; b < nblk; ++b) tot += part[(size_t)b * nc + c];
        out[(size_t)(c0 + c)] = std::sqrt(tot);
      }
    }
  }

  // IterRefine::iter_refine for a whole block (IterRefine.hpp:77-105 and :121-165)
  void hifir_dev(const D *dB, int64_t ldb, D *dX, int64_t ldx, int64_t nrhs, int nirs, const double *betas,
                 int64_t rank, int *ir_status) {
    check_batch(dB, ldb, dX, ldx, nrhs);
    HIP_OK(hipSetDevice(device));
    const int64_t n = lv[0]->n;
    if (nirs <= 1) {  // :83-87 / :128-132
      solve_dev(dB, ldb, dX, ldx, nrhs, rank, nullptr);
      HIP_OK(hipStreamSynchronize(stream));
      check_device_error();
      if (ir_status)
        for (int64_t c = 0; c < nrhs; ++c) ir_status[2 * c] = 1, ir_status[2 * c + 1] = -1;
      return;
    }
    if (!has_A) throw Error(HIFAMD_BAD_PREC, "iterative refinement needs the matrix (hifamd_set_matrix)");
    const size_t need = (size_t)n * nrhs * sizeof(T);
    if (ir_r.bytes < need) ir_r.alloc(need);
    if (ir_xk.bytes < need) ir_xk.alloc(need);
    D *r = ir_r.as<D>(), *xk = ir_xk.as<D>();
    if (!betas) {
      // x = 0; repeat N: xk = x; r = (i ? b - A xk : b); x = M^{-1} r + xk
      vec_op(0, n, nrhs, dX, ldx, nullptr, 0, nullptr, 0);
      for (int i = 0; i < nirs; ++i) {
        vec_op(1, n, nrhs, xk, nrhs, dX, ldx, nullptr, 0);
        if (i)
          resid_dev(dB, ldb, xk, nrhs, r, nrhs, nrhs, opt.resid_mode);
        else
          vec_op(1, n, nrhs, r, nrhs, dB, ldb, nullptr, 0);
        // M.solve(x, _r): the reference solves into _r and then x = _r + _xk (:102-103)
        solve_dev(r, nrhs, dX, ldx, nrhs, rank, nullptr);
        vec_op(2, n, nrhs, dX, ldx, xk, nrhs, nullptr, 0);  // x = M^{-1} r + xk  (a + b commutes bitwise)
      }
      HIP_OK(hipStreamSynchronize(stream));
      check_device_error();
      if (ir_status)
        for (int64_t c = 0; c < nrhs; ++c) ir_status[2 * c] = nirs, ir_status[2 * c + 1] = -1;
      return;
    }
    // bounded variant, per column; columns that finished keep iterating harmlessly only until all
    // are done?  No: a finished column must keep the x it had -- freeze it by masking its update.
    std::vector<double> bnorm, rnorm;
    col_norms(dB, ldb, n, nrhs, bnorm);
    std::vector<int> iters((size_t)nrhs, 0), flag((size_t)nrhs, 0);
    std::vector<char> active((size_t)nrhs, 1);
    vec_op(0, n, nrhs, dX, ldx, nullptr, 0, nullptr, 0);
    for (int64_t c = 0; c < nrhs; ++c)
      if (bnorm[(size_t)c] == 0.0) active[(size_t)c] = 0;  // :134-137: x = 0, (0, 0)
    vec_op(1, n, nrhs, r, nrhs, dB, ldb, nullptr, 0);
    int nactive = 0;
    for (char a : active) nactive += a;
    while (nactive > 0) {
      solve_dev(r, nrhs, xk, nrhs, nrhs, rank, nullptr);  // xk = M^{-1} r
      const int *mask = column_mask((size_t)nrhs, [&](size_t c) { return active[c] != 0; });
      launch_masked_add(n, nrhs, dX, ldx, xk, nrhs, mask);  // x += xk on active columns
      for (int64_t c = 0; c < nrhs; ++c)
        if (active[(size_t)c] && ++iters[(size_t)c] >= nirs) {
          flag[(size_t)c] = -1;
          active[(size_t)c] = 0;
        }
      nactive = 0;
      for (char a : active) nactive += a;
      if (!nactive) break;
      resid_dev(dB, ldb, dX, ldx, r, nrhs, nrhs, opt.resid_mode);  // r = b - A x
      col_norms(r, nrhs, n, nrhs, rnorm);
      for (int64_t c = 0; c < nrhs; ++c) {
        if (!active[(size_t)c]) continue;
        const double res = rnorm[(size_t)c] / bnorm[(size_t)c];
        if (res <= betas[0])
          active[(size_t)c] = 0;
        else if (res > betas[1]) {
          flag[(size_t)c] = 1;
          active[(size_t)c] = 0;
        }
      }
      nactive = 0;
      for (char a : active) nactive += a;
    }
    HIP_OK(hipStreamSynchronize(stream));
    check_device_error();
    if (ir_status)
      for (int64_t c = 0; c < nrhs; ++c) ir_status[2 * c] = iters[(size_t)c], ir_status[2 * c + 1] = flag[(size_t)c];
  }

  // The column mask of the two refinement drivers (bounded refinement, GMRES-IR): mask[c] = pred(c) for c < nc, enqueued
  // for the launch that follows.  The source is pageable on purpose: the copy has read it when the call returns, so the
  // next mask may overwrite it at once.
  DevBuf ir_mask;
  std::vector<int> ir_hmask;
  template <class Pred>
  const int *column_mask(size_t nc, Pred pred) {
    if (ir_mask.bytes < nc * sizeof(int)) ir_mask.alloc(nc * sizeof(int));
    ir_hmask.resize(nc);
    for (size_t c = 0; c < nc; ++c) ir_hmask[c] = pred(c) ? 1 : 0;
    HIP_OK(hipMemcpyAsync(ir_mask.p, ir_hmask.data(), nc * sizeof(int), hipMemcpyHostToDevice, stream));
    return ir_mask.as<int>();
  }
  // masked axpy of the bounded IR variant: where mask[c], y[:, c] += x[:, c]
  void launch_masked_add(int64_t n, int64_t nrhs, D *y, int64_t ldy, const D *x, int64_t ldx, const int *mask) {
    hipLaunchKernelGGL((k_masked_add<D>), dim3(vec_grid(n * nrhs)), dim3(256), 0, stream, n, (int)nrhs, y, ldy, x, ldx, mask);
  }

  void hifir_host(const T *B, int64_t ldb, T *X, int64_t ldx, int64_t nrhs, int nirs, const double *betas,
                  int64_t rank, int *ir_status) {
    staged(B, ldb, X, ldx, nrhs, true, [] {},
           [&](const D *b, D *x) { hifir_dev(b, nrhs, x, nrhs, nrhs, nirs, betas, rank, ir_status); });
  }

  // ---- what the lock-step Krylov solvers share -------------------------------------------------------
  // The [n][64] work vectors of all of them: a tile asks for the first k (block GCR 1, GMRES 2, PCG and block CG 4, BiCGSTAB 5, symmetric QMR 7,
  // IDR(s) 2 s + 4), each grown to the tile's size and never shrunk.  One tile owns them from its first launch to its last read-back.
  // The same holds for the tile's scalars (kr_state) and for what read_back last returned.  It holds because no solver
  // runs inside another one's tile: the null-space search calls gmres_dev between its own local blocks, GMRES-IR calls
  // it between its residual (ir_r, ir_xk, gi_d) and its masked update with the bookkeeping on the host, and both copy
  // what they read back (col_norms, nsp_gram) into vectors of their own before the next call.  Flexible GMRES, the one
  // solver that calls out of a tile, calls the unbounded refinement (ir_r, ir_xk), which reads nothing back, and keeps
  // no read_back pointer across it; the projected PCG / QMR call apply_nsp (nsp_cpart, nsp_C).  None of these takes a
  // pool vector, the state block or a pointer into the pinned buffer.  Keep it so when adding a solver.
  DevBuf kr_vec[2 * kIdrMax + 4];
  void krylov_vectors(int k, size_t bytes) {
    for (int i = 0; i < k; ++i)
      if (kr_vec[i].bytes < bytes) kr_vec[i].alloc(bytes);
  }

  // The per-column scalars of every lock-step solver in one zeroed block: the slots of D, those of double, then
  // iter | flag | active | ctl and the solver's further int slots.  A slot is `rows` rows of [64] (IDR(s) keeps an s x s
  // matrix per column; GMRES indexes its slots [column][restart] and only needs the room).
  template <class V>
  struct Slot {
    V **p;
    int rows;
    Slot(V **p_, int rows_ = 1) : p(p_), rows(rows_) {}
  };
  DevBuf kr_state;
  void krylov_state(KrylovState &S, std::initializer_list<Slot<D>> ds, std::initializer_list<Slot<double>> rs, double rtol, int maxit,
                    std::initializer_list<int **> is = {}) {
    size_t nd = 0, nr = 0;
    for (const auto &slot : ds) nd += (size_t)slot.rows;
    for (const auto &slot : rs) nr += (size_t)slot.rows;
    const size_t o_re = nd * 64 * sizeof(D), o_int = o_re + nr * 64 * sizeof(double),
                 bytes = o_int + ((3 + is.size()) * 64 + 4) * sizeof(int);
    if (kr_state.bytes < bytes) kr_state.alloc(bytes);
    HIP_OK(hipMemsetAsync(kr_state.p, 0, bytes, stream));
    char *b = kr_state.as<char>();
    D *d = (D *)b;
    for (const auto &slot : ds) *slot.p = d, d += 64 * (size_t)slot.rows;
    double *r = (double *)(b + o_re);
    for (const auto &slot : rs) *slot.p = r, r += 64 * (size_t)slot.rows;
    int *ib = (int *)(b + o_int);
    S.iter = ib;
    S.flag = ib + 64;
    S.active = ib + 128;
    S.ctl = ib + 192;
    ib += 196;
    for (int **slot : is) *slot = ib, ib += 64;
    S.maxit = maxit;
    S.rtol = rtol;
  }
  // the four ctl ints of a tile: [0] columns still active, the rest the solver's own (valid until the next read_back)
  const int *krylov_ctl(const KrylovState &S) { return read_back<int>(S.ctl, 4); }
  int krylov_active(const KrylovState &S) { return krylov_ctl(S)[0]; }
  void krylov_result(const KrylovState &S, int nc, int *flags, int *iters) {
    const int *st = read_back<int>(S.iter, 128);  // iter | flag
    check_device_error();
    for (int c = 0; c < nc; ++c) {
      if (iters) iters[c] = st[c];
      if (flags) flags[c] = st[64 + c];
    }
  }

  // A device-pointer entry: the batch checks, the solver's own (check), then tile(b, x, nc, flags, iters, sweeps) on
  // every 64 columns (block CG: every `width` columns)
  template <class Check, class Tile>
  void krylov_batch(const D *dB, int64_t ldb, D *dX, int64_t ldx, int64_t nrhs, int *flags, int *iters, int *sweeps,
                    Check check, Tile tile, int width = 64) {
    check_batch(dB, ldb, dX, ldx, nrhs);
    check();
    HIP_OK(hipSetDevice(device));
    for (int64_t c0 = 0; c0 < nrhs; c0 += width) {
      const int nc = (int)std::min<int64_t>(width, nrhs - c0);
      auto at = [c0](int *p) { return p ? p + c0 : nullptr; };
      tile(dB + c0, dX + c0, nc, at(flags), at(iters), at(sweeps));
    }
  }
  void krylov_check(const std::string &who, int maxit, double rtol) {
    if (!has_A) throw Error(HIFAMD_BAD_PREC, who + " needs the matrix (hifamd_set_matrix)");
    if (maxit < 1 || !(rtol > 0.0)) throw Error(HIFAMD_MISMATCHED_SIZES, "need maxit >= 1, rtol > 0");
  }
  // for the solvers that need M^{-1} Hermitian; they run projected under a basis filter but not under the constant one
  void hermitian_check(const std::string &who, const char *instead, const char *filter) {
    const HermCheck &hc = hermitian();
    if (!hc.ok)
      throw Error(HIFAMD_BAD_PREC, who + " needs a Hermitian preconditioner and this hierarchy is not one (level " +
                                       std::to_string(hc.level) + ": " + hc.what +
                                       "); factorize a Hermitian matrix with is_symm, or use " + instead);
    if (nsp_on) throw Error(HIFAMD_BAD_PREC, who + " does not support " + filter + " (hifamd_set_nsp_const)");
  }

  // ---- what the block methods (block CG, block GCR, LOBPCG) share on top of that ------------------------------------
  // G = a^H b ([n][nc] each) through the kBcgBlocks partial matrices in pt
  void block_gram(const D *a, const D *b, int nc, D *pt, D *G) {
    hipLaunchKernelGGL((k_bcg_gram<D>), dim3(kBcgBlocks), dim3(256), 0, stream, lv[0]->n, nc, a, b, pt);
    hipLaunchKernelGGL((k_bcg_sum<D>), dim3(16), dim3(256), 0, stream, (const D *)pt, kBcgBlocks, nc, G);
  }
  // more than 64 KB of dynamic LDS: the function's limit is raised first, once per function whichever solvers share it
  std::map<const void *, size_t> lds_limit;
  void raise_lds(const void *fn, size_t bytes) {
    size_t &have = lds_limit[fn];
    if (bytes <= 64 * 1024 || bytes <= have) return;
    HIP_OK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    have = bytes;
  }
  // the tile's rank after its start and during its last step (ctl[1..2]) -> ranks[0..1] (may be null)
  void block_ranks(const KrylovState &S, int *ranks) {
    const int *ctl = krylov_ctl(S);
    if (ranks) ranks[0] = ctl[1], ranks[1] = ctl[2];
  }
  void block_check(int block, double deftol, int restart = 1) {
    if (block < 1 || block > 64) throw Error(HIFAMD_MISMATCHED_SIZES, "need 1 <= block <= 64");
    if (restart < 1 || restart > HIFAMD_BGCR_MAX_RESTART) throw Error(HIFAMD_MISMATCHED_SIZES, "need 1 <= restart <= HIFAMD_BGCR_MAX_RESTART");
    if (!(deftol > 0.0 && deftol < 1.0)) throw Error(HIFAMD_MISMATCHED_SIZES, "need 0 < deftol < 1");
  }
  // krylov_batch on tiles of `block` columns: tile(b, x, nc, flags, iters, ranks of tile t)
  template <class Check, class Tile>
  void block_batch(const D *dB, int64_t ldb, D *dX, int64_t ldx, int64_t nrhs, int block, int *flags, int *iters, int *ranks, Check check, Tile tile) {
    const int width = block >= 1 && block <= 64 ? block : 64;  // (a block out of range: check refuses it before any tile)
    auto one = [&](const D *b, D *x, int nc, int *fl, int *it, int *) { tile(b, x, nc, fl, it, ranks ? ranks + 2 * ((b - dB) / width) : nullptr); };
    krylov_batch(dB, ldb, dX, ldx, nrhs, flags, iters, nullptr, check, one, width);
  }

  // ---- right-preconditioned restarted GMRES, batched over columns ----------------------------------
  // The reference's driver (examples/advanced/gmres.hpp:19-123: MGS Arnoldi, Givens rotations, relative
  // residual |y_{j+1}| / ||b||, flags 0 converged / 1 stagnated / 2 reached maxit) run for up to 64
  // columns in lock step.  Everything lives in HBM: the vectors, the Krylov basis, AND the per-column
  // scalars (Hessenberg column, rotations, residuals, iteration counts, flags: GmState, kernels.hip.hpp,
  // carved out of kr_state like every lock-step solver's).
  // One inner step = one batched apply + one SpMM + j+2 fused axpy/dot passes (k_gm_step) each followed
  // by a one-workgroup finishing kernel, and ONE read-back of ctl (how many columns are still active).
  // A column that leaves the inner loop keeps a zero basis vector.  Real and complex handles (Hermitian
  // inner product; for real data identical to the reference's hif::inner).
  static constexpr int kGmBlocks = 1024;
  // v -= h q_prev (h = S.alpha, from the previous finish) fused with the reduction against q (nullptr: |v|^2)
  void gm_step(int64_t n, int nc, D *v, const D *qp, const D *q, const GmState<D> &S) {
    const size_t need = (size_t)kGmBlocks * kGmVals * 64 * sizeof(D);  // (what k_gm_block needs: no reallocation between the passes)
    if (ir_part.bytes < need) ir_part.alloc(need);
    hipLaunchKernelGGL((k_gm_step<D>), dim3(kGmBlocks), dim3(256), 0, stream, n, nc, v, qp, (const D *)S.alpha, q, ir_part.as<D>());
  }
  DevBuf gm_red, gm_hb;  // reduced value list of a Gram-Schmidt block; its coefficients h[kGmBlock][64]
  void gm_block(int64_t n, int nc, D *v, const D *Qp, int mp, const D *Qn, int mn, const GmState<D> &S) {
    (void)S;
    const size_t need = (size_t)kGmBlocks * kGmVals * 64 * sizeof(D);
    if (ir_part.bytes < need) ir_part.alloc(need);
    if (!gm_red.p) gm_red.alloc((size_t)kGmVals * 64 * sizeof(D));
    if (!gm_hb.p) gm_hb.alloc((size_t)kGmBlock * 64 * sizeof(D));
    hipLaunchKernelGGL((k_gm_block<D>), dim3(kGmBlocks), dim3(256), 0, stream, n, nc, v, Qp, mp, (const D *)gm_hb.as<D>(), Qn, mn,
                       ir_part.as<D>());
  }
  void gm_finish(int nc, int mode, int k, int nirs, const GmState<D> &S) {
    hipLaunchKernelGGL((k_gm_finish<D>), dim3(1), dim3(256), 0, stream, (const D *)ir_part.as<D>(), kGmBlocks, nc, mode, k, nirs, S);
  }
  void gm_colop(int op, int64_t n, int nc, D *y, int64_t ldy, const D *x, int64_t ldx, const GmState<D> &S) {
    int64_t g = (n * nc + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL((k_gm_colop<D>), dim3((unsigned)g), dim3(256), 0, stream, op, n, nc, y, ldy, x, ldx, (const D *)S.alpha);
  }
  void gmres_tile(const D *dB, int64_t ldb, D *dX, int64_t ldx, int nc, int restart, double rtol, int maxit,
                  int64_t rank, int *flags, int *iters, bool flexible, int *sweeps) {
    const int64_t n = lv[0]->n;
    const size_t vec = (size_t)n * nc * sizeof(D);
    krylov_vectors(2, vec);
    if (gm_Q.bytes < vec * (size_t)restart) gm_Q.alloc(vec * (size_t)restart);
    // flexible variant (fgmres_hifir, gmres.hpp:127-231): the preconditioned vectors are kept as well
    if (flexible && gm_Z.bytes < vec * (size_t)restart) gm_Z.alloc(vec * (size_t)restart);
    D *v = kr_vec[0].as<D>(), *w = kr_vec[1].as<D>(), *Q = gm_Q.as<D>(), *Z = gm_Z.as<D>();
    auto Qk = [&](int k) { return Q + (size_t)k * (size_t)n * nc; };
    auto Zk = [&](int k) { return Z + (size_t)k * (size_t)n * nc; };
    GmState<D> S;
    const size_t rs = (size_t)restart;
    auto rows = [nc](size_t per_column) { return (int)((nc * per_column + 63) / 64); };  // [nc][per_column] in rows of [64]
    krylov_state(S, {{&S.w2, rows(rs)}, {&S.Jc, rows(rs)}, {&S.y, rows(rs + 1)}, {&S.R, rows(rs * rs)}, &S.alpha},
                 {{&S.Js, rows(rs)}, &S.resid, &S.bnorm}, rtol, maxit, {&S.jfin, &S.done, &S.sweeps});
    S.restart = restart;
    int64_t grid = (n * nc + 255) / 256;
    if (grid > 4096) grid = 4096;
    vec_op(1, n, nc, v, nc, dB, ldb, nullptr, 0);  // v = b (contiguous copy: the first residual, :52)
    gm_step(n, nc, v, nullptr, nullptr, S);
    gm_finish(nc, 3, 0, 0, S);                     // beta0, quick return (:30-36)
    vec_op(0, n, nc, dX, ldx, nullptr, 0, nullptr, 0);  // x = 0  (:33-34)
    int not_done = krylov_ctl(S)[2];
    const int max_outer = (maxit + restart - 1) / restart;  // :43
    for (int outer = 0; outer < max_outer && not_done > 0; ++outer) {
      if (outer) {
        resid_dev(dB, ldb, (const D *)dX, ldx, v, nc, nc, opt.resid_mode);  // v = b - A x  (:48-50)
        gm_step(n, nc, v, nullptr, nullptr, S);
      }  // (outer == 0: the partial sums of |b|^2 are still in place)
      gm_finish(nc, 2, 0, 0, S);                        // beta, y[0], active mask  (:53-54)
      gm_colop(1, n, nc, Qk(0), nc, v, nc, S);          // Q(:,0) = v / beta  (:55)
      int j = 0;
      const int nirs = 1 << std::min(outer, 20);  // :157
      for (;;) {
        if (flexible) {
          // w = hifir(A, Q(:,j), 2^outer sweeps)  (:160); kept in Z (:164)
          hifir_dev((const D *)Qk(j), nc, w, nc, nc, nirs, nullptr, rank < 0 ? -1 : rank, nullptr);
          vec_op(1, n, nc, Zk(j), nc, (const D *)w, nc, nullptr, 0);
        } else {
          solve_dev((const D *)Qk(j), nc, w, nc, nc, rank, nullptr);  // w = M^{-1} Q(:,j)  (:58-59)
        }
        spmv_dev((const D *)w, nc, v, nc, nc, nullptr);  // v = A w  (:60)
        // modified Gram-Schmidt (:63-66), kGmBlock basis vectors per pass over v (k_gm_block)
        int kl = 0, ml = 0;
        for (int k = 0; k <= j; k += kGmBlock) {
          const int mn = std::min(kGmBlock, j + 1 - k);
          gm_block(n, nc, v, k ? Qk(k - kGmBlock) : nullptr, k ? kGmBlock : 0, Qk(k), mn, S);
          const int nv = mn + mn * (mn - 1) / 2;
          hipLaunchKernelGGL((k_gm_reduce<D>), dim3((unsigned)nv), dim3(256), 0, stream, (const D *)ir_part.as<D>(), kGmBlocks, nv, nc,
                             gm_red.as<D>());
          hipLaunchKernelGGL((k_gm_hblock<D>), dim3(1), dim3(64), 0, stream, (const D *)gm_red.as<D>(), nc, k, mn, S, gm_hb.as<D>());
          kl = k, ml = mn;
        }
        gm_block(n, nc, v, Qk(kl), ml, nullptr, 0, S);  // the last block's update + |v|^2  (:65,67)
        gm_finish(nc, 1, j, flexible ? nirs : 0, S);  // rotations, residual, stopping rules  (:73-103)
        if (j + 1 < restart) gm_colop(1, n, nc, Qk(j + 1), nc, v, nc, S);  // :69-70
        if (krylov_active(S) == 0) break;
        ++j;
      }
      hipLaunchKernelGGL((k_gm_backsolve<D>), dim3(1), dim3(64), 0, stream, nc, S);  // :106-110, :120
      const int *ctl = krylov_ctl(S);
      const int jmax = ctl[1];
      not_done = ctl[2];
      if (flexible) {  // x += Z y  (:214-218)
        hipLaunchKernelGGL((k_gm_combine<D>), dim3((unsigned)grid), dim3(256), 0, stream, n, nc, dX, ldx, 1, (const D *)Z, jmax, S);
      } else {
        hipLaunchKernelGGL((k_gm_combine<D>), dim3((unsigned)grid), dim3(256), 0, stream, n, nc, v, (int64_t)nc, 0, (const D *)Q, jmax, S);  // v = Q y  (:112-116)
        solve_dev((const D *)v, nc, w, nc, nc, rank, nullptr);  // :118
        gm_colop(0, n, nc, dX, ldx, (const D *)w, nc, S);       // x += w  (:119; alpha = 1 for the columns that took part)
      }
    }
    krylov_result(S, nc, flags, iters);
    if (sweeps) std::copy_n(read_back<int>(S.sweeps, (size_t)nc), nc, sweeps);
  }

  void gmres_check(int restart, int maxit, double rtol) {
    if (!has_A) throw Error(HIFAMD_BAD_PREC, "GMRES needs the matrix (hifamd_set_matrix)");
    if (restart < 1 || maxit < 1 || !(rtol > 0.0)) throw Error(HIFAMD_MISMATCHED_SIZES, "need restart >= 1, maxit >= 1, rtol > 0");
  }
  void gmres_dev(const D *dB, int64_t ldb, D *dX, int64_t ldx, int64_t nrhs, int restart, double rtol,
                 int maxit, int64_t rank, int *flags, int *iters, bool flexible = false, int *sweeps = nullptr) {
    krylov_batch(dB, ldb, dX, ldx, nrhs, flags, iters, sweeps, [&] { gmres_check(restart, maxit, rtol); },
                 [&](const D *b, D *x, int nc, int *fl, int *it, int *sw) {
                   gmres_tile(b, ldb, x, ldx, nc, restart, rtol, maxit, rank, fl, it, flexible, sw);
                 });
  }
  // (GMRES's own checks run in gmres_dev, behind the staging copy)
  void gmres_host(const T *B, int64_t ldb, T *X, int64_t ldx, int64_t nrhs, int restart, double rtol,
                  int maxit, int64_t rank, int *flags, int *iters, bool flexible = false, int *sweeps = nullptr) {
    staged(B, ldb, X, ldx, nrhs, false, [] {}, [&](const D *b, D *x) {
      gmres_dev(b, nrhs, x, nrhs, nrhs, restart, rtol, maxit, rank, flags, iters, flexible, sweeps);
    });
  }

  // ---- GMRES-based iterative refinement (Carson and Higham's GMRES-IR), batched over columns -----------
  // Refinement whose residual is formed as if in twice the working precision and whose correction equation A d = r is
  // solved by right-preconditioned GMRES:
  //   x = 0; bn = ||b||
  //   outer k = 0, 1, ...: r = b - A x, compensated whatever the handle's mode (k = 0: r = b); res = ||r|| / bn
  //     res <= rtol                       flag 0
  //     k > 0 and res >= res of step k-1  flag 1 (stagnated): the column gets back the iterate of step k-1 (ir_xk)
  //     k == max_outer                    flag 2
  //     the frozen columns of r are zeroed; d = gmres_dev(r) (x0 = 0, inner_rtol relative to ||r||); x += d on the
  //     active columns
  // Per 64-column tile, the per-column bookkeeping on the host as in hifir_dev's bounded branch: one read-back (the
  // column norms) per outer step.  A zero column: x = 0, flag 0, 0 steps; a column whose norm or residual is not finite:
  // flag 1 at once.  The restart residuals of the inner GMRES follow the handle's mode.  No pool vector is held while
  // gmres_dev runs (see kr_vec): r lives in ir_r, the previous iterate in ir_xk, the correction in gi_d.
  DevBuf gi_d;
  void launch_masked_set(int64_t n, int64_t nrhs, D *y, int64_t ldy, const D *x, int64_t ldx, const int *mask) {
    hipLaunchKernelGGL((k_masked_set<D>), dim3(vec_grid(n * nrhs)), dim3(256), 0, stream, n, (int)nrhs, y, ldy, x, ldx, mask);
  }
  void gmres_ir_tile(const D *dB, int64_t ldb, D *dX, int64_t ldx, int nc, int restart, double rtol, double inner_rtol,
                     int max_outer, int inner_maxit, int64_t rank, int *flags, int *outer, int *iters, double *relres) {
    const int64_t n = lv[0]->n;
    // The residual and the correction live in blocks of W columns whatever nc is, the columns behind nc zero: the
    // reductions of GMRES and of the norms deal rows to threads by the block's width, so a fixed width is what makes a
    // column's bits (x and relres) independent of the batch it came in.  W is the widest tile the handle takes.
    const int W = (int)std::min<int64_t>(64, std::max<int64_t>(Rmax, max_nrhs));
    const size_t vec = (size_t)n * W * sizeof(D);
    if (ir_r.bytes < vec) ir_r.alloc(vec);
    if (ir_xk.bytes < vec) ir_xk.alloc(vec);
    if (gi_d.bytes < vec) gi_d.alloc(vec);
    D *r = ir_r.as<D>(), *xk = ir_xk.as<D>(), *d = gi_d.as<D>();
    StreamWait wait{stream};
    const size_t w = (size_t)nc;
    std::vector<double> bn, rn, res(w, 0.0), prev(w, 0.0);
    std::vector<int> fl(w, 0), nout(w, 0), nit(w, 0), gfl((size_t)W), git((size_t)W);
    std::vector<char> active(w, 1);
    vec_op(0, n, nc, dX, ldx, nullptr, 0, nullptr, 0);  // x = 0
    HIP_OK(hipMemsetAsync(r, 0, vec, stream));
    vec_op(1, n, nc, r, W, dB, ldb, nullptr, 0);  // r = b
    col_norms(r, W, n, W, bn);
    for (size_t c = 0; c < w; ++c) {
      if (bn[c] == 0.0) active[c] = 0;  // x = 0, flag 0, 0 steps
      if (!std::isfinite(bn[c])) active[c] = 0, fl[c] = 1, res[c] = std::numeric_limits<double>::quiet_NaN();
    }
    rn = bn;
    for (int k = 0;; ++k) {
      int nactive = 0;
      for (char a : active) nactive += a;
      if (!nactive) break;
      if (k > 0) {
        resid_dev(dB, ldb, (const D *)dX, ldx, r, W, nc, 1);  // r = b - A x, compensated
        col_norms(r, W, n, W, rn);
      }
      std::vector<char> back(w, 0);
      int nback = 0;
      for (size_t c = 0; c < w; ++c) {
        if (!active[c]) continue;
        const double rc = rn[c] / bn[c];
        if (k > 0 && (!std::isfinite(rc) || rc >= prev[c])) {  // no better than the iterate before: that one is returned
          fl[c] = 1, active[c] = 0, back[c] = 1, ++nback;
          res[c] = prev[c], --nout[c];
          continue;
        }
        res[c] = prev[c] = rc;
        if (rc <= rtol)
          active[c] = 0;
        else if (k == max_outer)
          fl[c] = 2, active[c] = 0;
      }
      if (nback) {
        launch_masked_set(n, nc, dX, ldx, (const D *)xk, nc, column_mask(w, [&](size_t c) { return back[c] != 0; }));
      }
      nactive = 0;
      for (char a : active) nactive += a;
      if (!nactive) break;
      // the frozen columns take no part
      launch_masked_set(n, nc, r, W, (const D *)nullptr, 0, column_mask(w, [&](size_t c) { return !active[c]; }));
      gmres_dev((const D *)r, W, d, W, W, restart, inner_rtol, inner_maxit, rank, gfl.data(), git.data());
      vec_op(1, n, nc, xk, nc, (const D *)dX, ldx, nullptr, 0);  // the iterate of this step, should the next be no better
      // x += d on the active columns
      launch_masked_add(n, nc, dX, ldx, (const D *)d, W, column_mask(w, [&](size_t c) { return active[c] != 0; }));
      HIP_OK(hipGetLastError());
      for (size_t c = 0; c < w; ++c)
        if (active[c]) ++nout[c], nit[c] += git[c];
    }
    HIP_OK(hipStreamSynchronize(stream));
    check_device_error();
    for (size_t c = 0; c < w; ++c) {
      if (flags) flags[c] = fl[c];
      if (outer) outer[c] = nout[c];
      if (iters) iters[c] = nit[c];
      if (relres) relres[c] = res[c];
    }
  }
  void gmres_ir_check(int restart, double rtol, double inner_rtol, int max_outer, int inner_maxit) {
    gmres_check(restart, inner_maxit, rtol);
    if (!(inner_rtol > 0.0 && inner_rtol < 1.0) || max_outer < 1)
      throw Error(HIFAMD_MISMATCHED_SIZES, "need 0 < inner_rtol < 1 and max_outer >= 1");
  }
  void gmres_ir_dev(const D *dB, int64_t ldb, D *dX, int64_t ldx, int64_t nrhs, int restart, double rtol, double inner_rtol,
                    int max_outer, int inner_maxit, int64_t rank, int *flags, int *outer, int *iters, double *relres) {
    krylov_batch(dB, ldb, dX, ldx, nrhs, flags, iters, outer, [&] { gmres_ir_check(restart, rtol, inner_rtol, max_outer, inner_maxit); },
                 [&](const D *b, D *x, int nc, int *fl, int *it, int *ou) {
                   gmres_ir_tile(b, ldb, x, ldx, nc, restart, rtol, inner_rtol, max_outer, inner_maxit, rank, fl, ou, it,
                                 relres ? relres + (b - dB) : nullptr);
                 });
  }
  void gmres_ir_host(const T *B, int64_t ldb, T *X, int64_t ldx, int64_t nrhs, int restart, double rtol, double inner_rtol,
                     int max_outer, int inner_maxit, int64_t rank, int *flags, int *outer, int *iters, double *relres) {
    staged(B, ldb, X, ldx, nrhs, false, [&] { gmres_ir_check(restart, rtol, inner_rtol, max_outer, inner_maxit); },
           [&](const D *b, D *x) {
             gmres_ir_dev(b, nrhs, x, nrhs, nrhs, restart, rtol, inner_rtol, max_outer, inner_maxit, rank, flags, outer, iters, relres);
           });
  }

  // ---- preconditioned CG, batched over columns ------------------------------------------------------
  // x0 = 0; r = b; z = M^{-1} r; p = z; rho = r^H z; then per step q = A p, sigma = p^H q, alpha = rho / sigma,
  // x += alpha p, r -= alpha q, stop on ||r|| / ||b|| <= rtol, z = M^{-1} r, rho' = r^H z, p = z + (rho' / rho) p.
  // Up to 64 columns in lock step: one batched apply, one SpMM and four fused vector passes (k_cg_*) per step, each
  // pass followed by a one-workgroup finishing kernel; the per-column scalars live in HBM (CgState) and the host reads
  // ctl once per step (how many columns are still active) through the pinned buffer of the engine.  Only for a
  // Hermitian M^{-1} (import.hpp check_hermitian); flags 0 converged / 1 breakdown / 2 reached maxit.
  void pcg_tile(const D *dB, int64_t ldb, D *dX, int64_t ldx, int nc, double rtol, int maxit, int64_t rank, int *flags,
                int *iters) {
    const int64_t n = lv[0]->n;
    const size_t vec = (size_t)n * nc * sizeof(D), part = (size_t)kCgBlocks * 64 * sizeof(D);
    krylov_vectors(4, vec);
    if (ir_part.bytes < part) ir_part.alloc(part);
    D *r = kr_vec[0].as<D>(), *z = kr_vec[1].as<D>(), *p = kr_vec[2].as<D>(), *q = kr_vec[3].as<D>(), *pt = ir_part.as<D>();
    StreamWait wait{stream};
    CgState<D> S;
    krylov_state(S, {&S.rho, &S.alpha, &S.beta}, {&S.bnorm}, rtol, maxit);
    auto dot = [&](const D *a, const D *b) {
      hipLaunchKernelGGL((k_cg_dot<D>), dim3(kCgBlocks), dim3(256), 0, stream, n, nc, a, (int64_t)nc, b, pt);
    };
    auto finish = [&](int mode, int k) {
      hipLaunchKernelGGL((k_cg_finish<D>), dim3(1), dim3(1024), 0, stream, (const D *)pt, nc, mode, k, S);
    };
    vec_op(1, n, nc, r, nc, dB, ldb, nullptr, 0);  // r = b
    // projected PCG: with a basis filter P = I - Q Q^H on the solve the iteration runs on the complement of span(Q):
    // r0 = P b, ||b|| := ||P b||, and every z = M^{-1} r below is already P M^{-1} r (solve_dev filters it)
    if (nsp_k > 0) apply_nsp(r, nc, nc, stream);
    dot(r, nullptr);
    finish(0, 0);                                        // ||b||
    vec_op(0, n, nc, dX, ldx, nullptr, 0, nullptr, 0);   // x = 0
    solve_dev((const D *)r, nc, z, nc, nc, rank, nullptr);  // z = M^{-1} r
    dot(r, z);
    finish(1, 0);                                        // rho = r^H z
    vec_op(1, n, nc, p, nc, (const D *)z, nc, nullptr, 0);  // p = z
    HIP_OK(hipGetLastError());
    // (one read-back per step, after the convergence test; a column that breaks down in mode 4 costs one frozen step)
    for (int k = 0, go = krylov_active(S); k < maxit && go > 0; ++k) {
      spmv_dev((const D *)p, nc, q, nc, nc, nullptr);    // q = A p
      dot(p, q);
      finish(2, k);                                      // alpha = rho / p^H q
      hipLaunchKernelGGL((k_cg_xr<D>), dim3(kCgBlocks), dim3(256), 0, stream, n, nc, dX, ldx, r, (const D *)p, (const D *)q,
                         (const D *)S.alpha, (const int *)S.active, pt);
      finish(3, k);                                      // ||r|| / ||b||, maxit
      if ((go = krylov_active(S)) == 0) break;
      solve_dev((const D *)r, nc, z, nc, nc, rank, nullptr);
      dot(r, z);
      finish(4, k);                                      // beta = rho' / rho
      hipLaunchKernelGGL((k_cg_p<D>), dim3(kCgBlocks), dim3(256), 0, stream, n, nc, p, (const D *)z, (const D *)S.beta,
                         (const int *)S.active);
      HIP_OK(hipGetLastError());
    }
    krylov_result(S, nc, flags, iters);
  }

  void pcg_check(int maxit, double rtol) {
    krylov_check("PCG", maxit, rtol);
    hermitian_check("PCG", "GMRES", "a null-space filter");
  }
  void pcg_dev(const D *dB, int64_t ldb, D *dX, int64_t ldx, int64_t nrhs, double rtol, int maxit, int64_t rank,
               int *flags, int *iters) {
    krylov_batch(dB, ldb, dX, ldx, nrhs, flags, iters, nullptr, [&] { pcg_check(maxit, rtol); },
                 [&](const D *b, D *x, int nc, int *fl, int *it, int *) { pcg_tile(b, ldb, x, ldx, nc, rtol, maxit, rank, fl, it); });
  }
  void pcg_host(const T *B, int64_t ldb, T *X, int64_t ldx, int64_t nrhs, double rtol, int maxit, int64_t rank,
                int *flags, int *iters) {
    staged(B, ldb, X, ldx, nrhs, false, [&] { pcg_check(maxit, rtol); },
           [&](const D *b, D *x) { pcg_dev(b, nrhs, x, nrhs, nrhs, rtol, maxit, rank, flags, iters); });
  }

  // ---- breakdown-free block CG: the columns of a tile share one block Krylov space ---------------------------
  // Dubrulle's BCGrQ, preconditioned.  The block residual is kept factored, R = Q C with Q^H M^{-1} Q = I, and a pivoted
  // Cholesky of the Gram shrinks the block where its columns become dependent (duplicate, zero or converged directions):
  //   start: beta_j = ||b_j||, R = B diag(1 / beta) (zero and non-finite columns enter as exact zeros), Z = M^{-1} R,
  //          G = R^H Z = S^H S (pivoted, rank r), E = I[:, piv] inv(S[:, piv]), Q = R E, P = Z E, C = S;
  //   step:  T = A P, alpha = (P^H T)^{-1}, X += P alpha C diag(beta), Q -= T alpha, relres_j = sqrt(c_j^H Q^H Q c_j), test;
  //          W = M^{-1} Q, G = Q^H W = S^H S (pivoted, rank r'), Q <- Q E, P <- W E + P S^H, C <- S C.
  // Per step one batched apply, one SpMM, two Gram passes (k_bcg_gram), two row-local passes (k_bcg_xq, which also gives
  // Q^H Q, and k_bcg_qp), three one-workgroup kernels (k_bcg_small) and ONE read-back, after the test.  The vectors are
  // kr_vec[0..3] = Q, W, P, T at [n][nc]; the small matrices live beside the KrylovState (BcgState).  flags 0 converged /
  // 1 breakdown or excluded / 2 reached maxit; the iteration count is the tile's.  ranks (may be null): the tile's rank
  // after the start and during its last step.
  void bcg_tile(const D *dB, int64_t ldb, D *dX, int64_t ldx, int nc, double rtol, double deftol, int maxit, int64_t rank,
                int *flags, int *iters, int *ranks) {
    const int64_t n = lv[0]->n;
    const size_t vec = (size_t)n * nc * sizeof(D), mat = (size_t)64 * 64 * sizeof(D);
    const size_t part = std::max((size_t)kBcgBlocks * mat, (size_t)kCgBlocks * 64 * sizeof(D));
    krylov_vectors(4, vec);
    if (ir_part.bytes < part) ir_part.alloc(part);
    D *Q = kr_vec[0].as<D>(), *W = kr_vec[1].as<D>(), *P = kr_vec[2].as<D>(), *Tm = kr_vec[3].as<D>(), *pt = ir_part.as<D>();
    const size_t lds_pass = 2 * mat, lds_small = bcg::Work<D>::bytes();  // (the small kernel's 65 KB; a complex handle's 129 KB)
    raise_lds((const void *)k_bcg_xq<D>, lds_pass);
    raise_lds((const void *)k_bcg_qp<D>, lds_pass);
    raise_lds((const void *)k_bcg_small<D>, lds_small);
    StreamWait wait{stream};
    BcgState<D> S;
    krylov_state(S, {{&S.C, 64}, {&S.E1, 64}, {&S.E2, 64}, {&S.G, 64}}, {&S.bnorm, &S.relres}, rtol, maxit);
    S.deftol = deftol;
    auto small = [&](int mode, int k) {
      hipLaunchKernelGGL((k_bcg_small<D>), dim3(1), dim3(256), lds_small, stream, mode, k, nc, S);
    };
    auto qp = [&] {  // Q <- Q E1, P <- W E1 + P E2
      hipLaunchKernelGGL((k_bcg_qp<D>), dim3(kBcgBlocks), dim3(256), lds_pass, stream, n, nc, Q, (const D *)W, P, (const D *)S.E1,
                         (const D *)S.E2);
    };
    vec_op(1, n, nc, Q, nc, dB, ldb, nullptr, 0);  // R = b (R lives in Q, Z in W)
    if (nsp_k > 0) apply_nsp(Q, nc, nc, stream);  // projected, as PCG: R = P b, beta = ||P b||
    hipLaunchKernelGGL((k_cg_dot<D>), dim3(kCgBlocks), dim3(256), 0, stream, n, nc, (const D *)Q, (int64_t)nc, (const D *)nullptr, pt);
    hipLaunchKernelGGL((k_bcg_beta<D>), dim3(1), dim3(1024), 0, stream, (const D *)pt, nc, S);
    hipLaunchKernelGGL((k_bcg_norm<D>), dim3(vec_grid(n * nc)), dim3(256), 0, stream, n, nc, Q, (const double *)S.bnorm,
                       (const int *)S.active);
    vec_op(0, n, nc, dX, ldx, nullptr, 0, nullptr, 0);  // x = 0
    HIP_OK(hipMemsetAsync(P, 0, vec, stream));
    solve_dev((const D *)Q, nc, W, nc, nc, rank, nullptr);  // Z = M^{-1} R
    block_gram(Q, W, nc, pt, S.G);
    small(1, 0);
    qp();  // Q = R E, P = Z E (E2 = 0)
    HIP_OK(hipGetLastError());
    for (int k = 1, go = krylov_active(S); k <= maxit && go > 0; ++k) {
      spmv_dev((const D *)P, nc, Tm, nc, nc, nullptr);  // T = A P
      block_gram(P, Tm, nc, pt, S.G);
      small(2, k);  // alpha = (P^H T)^{-1}
      hipLaunchKernelGGL((k_bcg_xq<D>), dim3(kBcgBlocks), dim3(256), lds_pass, stream, n, nc, dX, ldx, Q, (const D *)P,
                         (const D *)Tm, (const D *)S.E1, (const D *)S.E2, pt);
      hipLaunchKernelGGL((k_bcg_sum<D>), dim3(16), dim3(256), 0, stream, (const D *)pt, kBcgBlocks, nc, S.G);
      small(3, k);  // the residual test
      if ((go = krylov_active(S)) == 0) break;
      solve_dev((const D *)Q, nc, W, nc, nc, rank, nullptr);  // W = M^{-1} Q
      block_gram(Q, W, nc, pt, S.G);
      small(4, k);  // the next block: rank, E, S^H, C
      qp();
      HIP_OK(hipGetLastError());
    }
    krylov_result(S, nc, flags, iters);
    block_ranks(S, ranks);
  }

  void bcg_check(int block, double deftol, int maxit, double rtol) {
    krylov_check("block CG", maxit, rtol);
    hermitian_check("block CG", "GMRES", "a null-space filter");
    block_check(block, deftol);
  }
  void bcg_dev(const D *dB, int64_t ldb, D *dX, int64_t ldx, int64_t nrhs, int block, double rtol, double deftol, int maxit,
               int64_t rank, int *flags, int *iters, int *ranks) {
    block_batch(dB, ldb, dX, ldx, nrhs, block, flags, iters, ranks, [&] { bcg_check(block, deftol, maxit, rtol); },
                [&](const D *b, D *x, int nc, int *fl, int *it, int *rk) { bcg_tile(b, ldb, x, ldx, nc, rtol, deftol, maxit, rank, fl, it, rk); });
  }
  void bcg_host(const T *B, int64_t ldb, T *X, int64_t ldx, int64_t nrhs, int block, double rtol, double deftol, int maxit,
                int64_t rank, int *flags, int *iters, int *ranks) {
    staged(B, ldb, X, ldx, nrhs, false, [&] { bcg_check(block, deftol, maxit, rtol); },
           [&](const D *b, D *x) { bcg_dev(b, nrhs, x, nrhs, nrhs, block, rtol, deftol, maxit, rank, flags, iters, ranks); });
  }

  // ---- LOBPCG: the nev smallest eigenpairs of a Hermitian pair (A, M), a block of k <= 16 candidates --------------
  // Knyazev's locally optimal block PCG with a Rayleigh-Ritz step on the orthonormalized basis [X W P]:
  //   start: X = X0 (or generated from seed), filtered under a basis filter; G = X^H X = S^H S (pivoted Cholesky, rank < k or
  //          not finite: refused), X <- X E; AX = A X; X^H AX = V Theta V^H, X <- X V, AX <- AX V, lambda = Theta, P = AP = 0;
  //   loop:  R = AX - X diag(lambda), res_j = ||r_j|| / ||A||_inf, conv_j = res_j <= tol; all j < nev converged or
  //          steps == maxit: end.  W = M^{-1} R (converged columns exact zeros), AW = A W; GB = S^H S, GA = S^H AS on
  //          S = [X W P]; D = diag(GB)^(-1/2), D GB D = T^H T (pivoted, stopped at deftol, rank r; r < k: breakdown),
  //          E = D I[:, piv] inv(T[:, piv]); E^H GA E = V Theta V^H ascending; C = E V[:, :k], lambda = Theta[:k], Cp = C with its
  //          first k rows zero; X, P <- S [C Cp], AX, AP <- AS [C Cp].
  // Per step one batched apply, one SpMM, one Gram pass (k_lob_gram), one row-local pass (k_lob_update), the residual pass
  // (k_lob_resid, k_lob_lock), two one-workgroup kernels (k_lob_small) and ONE read-back, after the test.  The vectors are
  // kr_vec[0..2] = S [n][3 k], AS [n][3 k], R [n][k]; the small matrices live beside the KrylovState (LobState).  flags
  // 0 converged / 1 breakdown / 2 not converged at maxit, per column by its own last res_j.  info3: steps, rank of the basis
  // in the last step, largest Jacobi sweep count.
  // GEN: the generalized problem A x = lambda B x, B the mass matrix of set_mass_matrix.  The same iteration and the same
  // kernels with a third block BS = [BX BW BP] = B S in kr_vec[3] (one more SpMM on k columns at the start and per step; the
  // row pass carries it along), GB = S^H BS in the places of S^H S, so that the Ritz vectors are B-orthonormal, X^H B X = I;
  // R = AX - BX diag(lambda) and res_j = ||r_j|| / ((||A||_inf + |lambda_j| ||B||_inf) ||x_j||), the normwise backward error
  // of the pair (X is B-normalized, so ||x_j|| is in the scale).  No filter of any kind (lobpcg_check).  With B = I given
  // explicitly BS is a bitwise copy of S and every iterate is the standard problem's, bit for bit, until the two stopping
  // tests differ.
  // lock (m > 0): the constraint block of the locked sweeps (eigs_dev): X is projected once, behind the start's filter and in
  // front of BX = B X, and W once per step, behind W = M^{-1} R and in front of AW = A W, both with P = I - Y (BY)^H
  // (eig_project).  The converged columns of W are exact zeros and stay exact zeros.  m = 0 launches nothing.
  struct EigLock {
    const D *Y = nullptr, *BY = nullptr;  // [n][kEigMaxM]; BY == Y on the standard problem
    int m = 0;
  };
  template <bool GEN>
  void lobpcg_tile(const D *dX0, int64_t ldx0, uint64_t seed, int k, int nev, double tol, double deftol, int maxit, int64_t rank,
                   D *dX, int64_t ldx, double *lambda, double *res, int *flags, int *info3, const EigLock &lock = EigLock()) {
    static const char *const refusal[2][3] = {
      {"LOBPCG: the start block is rank deficient", "LOBPCG: the start block is not finite",
       "LOBPCG: X^H A X of the start block is not finite, or its eigendecomposition did not end"},
      {"generalized LOBPCG: X^H B X of the start block has Cholesky rank below k: the start block is rank deficient, or B is not "
       "positive definite",
       "generalized LOBPCG: X^H B X of the start block is not finite (the start block or B is not finite)",
       "generalized LOBPCG: X^H A X of the start block is not finite, or its eigendecomposition did not end"}};
    const int64_t n = lv[0]->n;
    const int s = 3 * k;
    const size_t blk = (size_t)n * s * sizeof(D), mat = (size_t)64 * 64 * sizeof(D);
    const size_t part = std::max(2 * (size_t)kBcgBlocks * mat, (size_t)kLobResBlocks * (GEN ? 32 : 16) * sizeof(double));
    krylov_vectors(2, blk);
    if (kr_vec[2].bytes < blk / 3) kr_vec[2].alloc(blk / 3);  // R is [n][k]
    if (GEN && kr_vec[3].bytes < blk) kr_vec[3].alloc(blk);
    if (ir_part.bytes < part) ir_part.alloc(part);
    D *Sb = kr_vec[0].as<D>(), *ASb = kr_vec[1].as<D>(), *R = kr_vec[2].as<D>(), *pt = ir_part.as<D>();
    D *BSb = GEN ? kr_vec[3].as<D>() : nullptr;  // (the standard problem's kernels never read it)
    const size_t lds_small = lob::RitzScratch<D>::bytes();  // (68 KB; a complex handle's 133 KB)
    raise_lds((const void *)k_lob_small<D>, lds_small);
    StreamWait wait{stream};
    LobState<D> S;
    krylov_state(S, {{&S.GB, 64}, {&S.GA, 64}, {&S.CC, 64}, {&S.X1, 64}, {&S.X2, 64}, {&S.X3, 64}}, {&S.bnorm, &S.lam, &S.res}, tol,
                 maxit);
    S.deftol = deftol, S.anorm = A_norm_inf, S.b_inf = GEN ? B_norm_inf : 0.0, S.k = k, S.nev = nev, S.gen = GEN;
    auto gram = [&] {  // S.GB = S^H S (GEN: S^H BS), S.GA = S^H AS
      hipLaunchKernelGGL((k_lob_gram<D, GEN>), dim3(kBcgBlocks), dim3(256), 0, stream, n, s, s, (const D *)Sb, (const D *)BSb,
                         (const D *)ASb, pt);
      hipLaunchKernelGGL((k_bcg_sum<D>), dim3(16), dim3(256), 0, stream, (const D *)pt, kBcgBlocks, s, S.GB);
      hipLaunchKernelGGL((k_bcg_sum<D>), dim3(16), dim3(256), 0, stream, (const D *)(pt + (size_t)kBcgBlocks * 64 * 64), kBcgBlocks,
                         s, S.GA);
    };
    auto small = [&](int mode, int step) {
      hipLaunchKernelGGL((k_lob_small<D>), dim3(1), dim3(256), lds_small, stream, mode, step, (const double *)pt, S);
    };
    auto update = [&] {
      hipLaunchKernelGGL((k_lob_update<D, GEN ? 3 : 2>), dim3(kBcgBlocks), dim3(256), 0, stream, n, s, s, k, Sb, ASb, BSb,
                         (const D *)S.CC);
    };
    auto refused = [&] {  // the start's verdict
      const int verdict = krylov_ctl(S)[3];
      check_device_error();
      if (verdict >= 1 && verdict <= 3) throw Error(HIFAMD_BAD_PREC, refusal[GEN][verdict - 1]);
    };
    HIP_OK(hipMemsetAsync(Sb, 0, blk, stream));
    HIP_OK(hipMemsetAsync(ASb, 0, blk, stream));
    if (GEN) HIP_OK(hipMemsetAsync(BSb, 0, blk, stream));
    if (dX0) {
      vec_op(1, n, k, Sb, s, dX0, ldx0, nullptr, 0);
    } else {
      hipLaunchKernelGGL((k_idr_pfill<D>), dim3(vec_grid(n * k)), dim3(256), 0, stream, n, k, k, seed, R);
      vec_op(1, n, k, Sb, s, (const D *)R, k, nullptr, 0);
    }
    if (!GEN && nsp_k > 0) apply_nsp(Sb, s, k, stream);  // on the complement of span(Q)
    if (lock.m > 0) eig_project(lock.m, lock.Y, lock.BY, kEigMaxM, k, Sb, s, pt);
    if (GEN) spmm_launch(Bm, (const D *)Sb, s, BSb, s, k, stream);  // BX = B X
    gram();
    small(0, 0);
    refused();
    update();  // X <- X E (GEN: and BX)
    spmv_dev((const D *)Sb, s, ASb, s, k, nullptr);  // AX = A X
    gram();
    small(1, 0);
    refused();
    update();  // X <- X V, AX <- AX V, P = AP = 0 (GEN: and BX, BP)
    HIP_OK(hipGetLastError());
    for (int step = 0;; ++step) {
      hipLaunchKernelGGL((k_lob_resid<D, GEN>), dim3(kLobResBlocks), dim3(256), 0, stream, n, s, k, (const D *)Sb, (const D *)ASb,
                         (const D *)BSb, (const double *)S.lam, R, (double *)pt);
      small(2, step);
      if (krylov_active(S) == 0) break;
      hipLaunchKernelGGL((k_lob_lock<D>), dim3(vec_grid(n * k)), dim3(256), 0, stream, n, k, R, (const int *)S.active);
      solve_dev((const D *)R, k, Sb + k, s, k, rank, nullptr);  // W = M^{-1} R
      if (lock.m > 0) eig_project(lock.m, lock.Y, lock.BY, kEigMaxM, k, Sb + k, s, pt);
      spmv_dev((const D *)(Sb + k), s, ASb + k, s, k, nullptr);  // AW = A W
      if (GEN) spmm_launch(Bm, (const D *)(Sb + k), s, BSb + k, s, k, stream);  // BW = B W
      gram();
      small(3, step);
      update();
      HIP_OK(hipGetLastError());
    }
    vec_op(1, n, k, dX, ldx, (const D *)Sb, s, nullptr, 0);
    int its[64];
    krylov_result(S, k, flags, its);
    const int *ctl = krylov_ctl(S);
    if (info3) info3[0] = its[0], info3[1] = ctl[1], info3[2] = ctl[2];
    const double *out = read_back<double>(S.lam, 128);  // lam | res (ctl is gone with this read)
    for (int c = 0; c < k; ++c) {
      if (lambda) lambda[c] = out[c];
      if (res) res[c] = out[64 + c];
    }
  }

  // gen: the generalized problem's checks: the mass matrix directly after the matrix, no filter of any kind
  void lobpcg_check(int64_t k, int64_t nev, double tol, double deftol, int maxit, int64_t ldx0, bool has_x0, int64_t ldx, bool gen) {
    lobpcg_args(k, nev, tol, deftol, maxit, ldx0, has_x0, ldx);
    lobpcg_handle(k, gen);
  }
  // (the two halves of lobpcg_check: the arguments come first, then the handle; the locked sweeps put theirs in between)
  void lobpcg_args(int64_t k, int64_t nev, double tol, double deftol, int maxit, int64_t ldx0, bool has_x0, int64_t ldx) {
    if (k < 1 || k > 16) throw Error(HIFAMD_MISMATCHED_SIZES, "LOBPCG: need 1 <= k <= 16");
    if (nev < 1 || nev > k) throw Error(HIFAMD_MISMATCHED_SIZES, "LOBPCG: need 1 <= nev <= k");
    if (!(tol > 0.0)) throw Error(HIFAMD_MISMATCHED_SIZES, "LOBPCG: need tol > 0");
    if (maxit < 1) throw Error(HIFAMD_MISMATCHED_SIZES, "LOBPCG: need maxit >= 1");
    if (!(deftol > 0.0 && deftol < 1.0)) throw Error(HIFAMD_MISMATCHED_SIZES, "LOBPCG: need 0 < deftol < 1");
    if ((has_x0 && ldx0 < k) || ldx < k) throw Error(HIFAMD_MISMATCHED_SIZES, "LOBPCG: row stride smaller than k");
  }
  void lobpcg_handle(int64_t k, bool gen) {
    if (!finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
    if (k > std::max<int64_t>(Rmax, max_nrhs))
      throw Error(HIFAMD_MISMATCHED_SIZES, "block wider than the max_nrhs given to hifamd_finalize");
    if (!has_A) throw Error(HIFAMD_BAD_PREC, "LOBPCG needs the matrix (hifamd_set_matrix)");
    if (!gen) return hermitian_check("LOBPCG", "hifamd_nsp_find for null vectors", "a constant-mode null-space filter");
    if (!has_B) throw Error(HIFAMD_BAD_PREC, "generalized LOBPCG needs the mass matrix (hifamd_set_mass_matrix)");
    static const char *const filter =
      "a null-space filter: the Euclidean projector I - Q Q^H solves the pencil (A, P B P), not (A, B), and the B-orthogonal "
      "projector I - Q (Q^H B Q)^{-1} Q^H B is not implemented";
    hermitian_check("generalized LOBPCG", "hifamd_nsp_find for null vectors", filter);
    if (nsp_k > 0) throw Error(HIFAMD_BAD_PREC, std::string("generalized LOBPCG does not support ") + filter + " (hifamd_set_nsp_basis)");
  }
  void lobpcg_dev(bool gen, int64_t k, int64_t nev, const D *dX0, int64_t ldx0, uint64_t seed, double tol, double deftol, int maxit,
                  int64_t rank, double *lambda, D *dX, int64_t ldx, double *res, int *flags, int *info3) {
    lobpcg_check(k, nev, tol, deftol, maxit, ldx0, dX0 != nullptr, ldx, gen);
    if (!dX) throw Error(HIFAMD_NULL_OBJ, "NULL vector");
    HIP_OK(hipSetDevice(device));
    if (gen)
      lobpcg_tile<true>(dX0, ldx0, seed, (int)k, (int)nev, tol, deftol, maxit, rank, dX, ldx, lambda, res, flags, info3);
    else
      lobpcg_tile<false>(dX0, ldx0, seed, (int)k, (int)nev, tol, deftol, maxit, rank, dX, ldx, lambda, res, flags, info3);
  }
  void lobpcg_host(bool gen, int64_t k, int64_t nev, const T *X0, int64_t ldx0, uint64_t seed, double tol, double deftol, int maxit,
                   int64_t rank, double *lambda, T *X, int64_t ldx, double *res, int *flags, int *info3) {
    lobpcg_check(k, nev, tol, deftol, maxit, ldx0, X0 != nullptr, ldx, gen);
    if (!X) throw Error(HIFAMD_NULL_OBJ, "NULL vector");
    HIP_OK(hipSetDevice(device));
    const int64_t n = lv[0]->n;
    const size_t need = (size_t)n * k * sizeof(T);
    if (stage_b.bytes < need) stage_b.alloc(need);
    if (stage_x.bytes < need) stage_x.alloc(need);
    StreamWait wait{stream};
    if (X0) HIP_OK(hipMemcpy2DAsync(stage_b.p, k * sizeof(T), X0, ldx0 * sizeof(T), k * sizeof(T), n, hipMemcpyHostToDevice, stream));
    lobpcg_dev(gen, k, nev, X0 ? (const D *)stage_b.as<D>() : nullptr, k, seed, tol, deftol, maxit, rank, lambda, stage_x.as<D>(), k, res,
               flags, info3);
    HIP_OK(hipMemcpy2DAsync(X, ldx * sizeof(T), stage_x.p, k * sizeof(T), k * sizeof(T), n, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
  }

  // ---- the B-orthogonal projector and the locked LOBPCG sweeps (up to 128 eigenpairs) --------------------------------
  // W <- W - Y C, C = (BY)^H W: Y, BY [n][m] (m <= 128; the same pointer on the standard problem), W [n][kw] (kw <= 16), any
  // row strides.  k_eig_cgram's kBcgBlocks partials of C go through pt (kBcgBlocks x [128][16]) and are added in block
  // order; k_eig_cproj subtracts the row-local product.  Three launches, nothing read back.
  DevBuf eig_C, eig_Y, eig_BY, eig_blk;
  static constexpr size_t kEigPart = (size_t)kBcgBlocks * kEigMaxM * 16;  // elements of the partials
  void eig_coeff(int m, const D *BY, int64_t ldby, int kw, const D *W, int64_t ldw, D *pt) {
    if (eig_C.bytes < (size_t)kEigMaxM * 16 * sizeof(D)) eig_C.alloc((size_t)kEigMaxM * 16 * sizeof(D));
    const int rows = 16 * ((m + 15) / 16);
    hipLaunchKernelGGL((k_eig_cgram<D>), dim3(kBcgBlocks), dim3(256), 0, stream, lv[0]->n, m, BY, ldby, kw, W, ldw, pt);
    hipLaunchKernelGGL((k_eig_csum<D>), dim3((rows * 16 + 255) / 256), dim3(256), 0, stream, (const D *)pt, kBcgBlocks, rows,
                       eig_C.as<D>());
  }
  void eig_project(int m, const D *Y, const D *BY, int64_t ldy, int kw, D *W, int64_t ldw, D *pt) {
    eig_coeff(m, BY, ldy, kw, (const D *)W, ldw, pt);
    hipLaunchKernelGGL((k_eig_cproj<D>), dim3(kBcgBlocks), dim3(256), 0, stream, lv[0]->n, m, Y, ldy, kw, W, ldw,
                       (const D *)eig_C.as<D>());
    HIP_OK(hipGetLastError());
  }
  D *eig_partials() {
    if (ir_part.bytes < kEigPart * sizeof(D)) ir_part.alloc(kEigPart * sizeof(D));
    return ir_part.as<D>();
  }
  // the [n][128] blocks of the locked vectors and of their images under B: allocated on first use, freed with the engine
  void eig_blocks(bool y, bool by) {
    const size_t need = (size_t)lv[0]->n * kEigMaxM * sizeof(D);
    if (y && eig_Y.bytes < need) eig_Y.alloc(need);
    if (by && eig_BY.bytes < need) eig_BY.alloc(need);
  }

  // hifamd_eig_project(_dev): the projector alone.  gen: BY = B Y is formed here (spmm_launch: 64 columns a launch).
  void eig_project_check(bool gen, int64_t m, int64_t ldy, int64_t kw, int64_t ldw) {
    if (m < 1 || m > kEigMaxM) throw Error(HIFAMD_MISMATCHED_SIZES, "eig_project: need 1 <= m <= 128");
    if (kw < 1 || kw > 16) throw Error(HIFAMD_MISMATCHED_SIZES, "eig_project: need 1 <= kw <= 16");
    if (ldy < m || ldw < kw) throw Error(HIFAMD_MISMATCHED_SIZES, "eig_project: row stride smaller than the block");
    if (!finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
    if (gen && !has_B) throw Error(HIFAMD_BAD_PREC, "the B-orthogonal projector needs the mass matrix (hifamd_set_mass_matrix)");
  }
  void eig_project_dev(bool gen, int64_t m, const D *dY, int64_t ldy, int64_t kw, D *dW, int64_t ldw) {
    eig_project_check(gen, m, ldy, kw, ldw);
    if (!dY || !dW) throw Error(HIFAMD_NULL_OBJ, "NULL vector");
    HIP_OK(hipSetDevice(device));
    StreamWait wait{stream};
    D *pt = eig_partials();
    if (gen) {
      eig_blocks(false, true);  // (BY alone: the caller's Y is read where it lies)
      spmm_launch(Bm, dY, ldy, eig_BY.as<D>(), kEigMaxM, m, stream);
      eig_coeff((int)m, (const D *)eig_BY.as<D>(), kEigMaxM, (int)kw, (const D *)dW, ldw, pt);
      hipLaunchKernelGGL((k_eig_cproj<D>), dim3(kBcgBlocks), dim3(256), 0, stream, lv[0]->n, (int)m, dY, ldy, (int)kw, dW, ldw,
                         (const D *)eig_C.as<D>());
      HIP_OK(hipGetLastError());
    } else {
      eig_project((int)m, dY, dY, ldy, (int)kw, dW, ldw, pt);
    }
    HIP_OK(hipStreamSynchronize(stream));
    check_device_error();
  }
  void eig_project_host(bool gen, int64_t m, const T *Y, int64_t ldy, int64_t kw, T *W, int64_t ldw) {
    eig_project_check(gen, m, ldy, kw, ldw);
    if (!Y || !W) throw Error(HIFAMD_NULL_OBJ, "NULL vector");
    HIP_OK(hipSetDevice(device));
    const int64_t n = lv[0]->n;
    const size_t ny = (size_t)n * m * sizeof(T), nw = (size_t)n * kw * sizeof(T);
    if (stage_r.bytes < ny) stage_r.alloc(ny);
    if (stage_x.bytes < nw) stage_x.alloc(nw);
    StreamWait wait{stream};
    HIP_OK(hipMemcpy2DAsync(stage_r.p, m * sizeof(T), Y, ldy * sizeof(T), m * sizeof(T), n, hipMemcpyHostToDevice, stream));
    HIP_OK(hipMemcpy2DAsync(stage_x.p, kw * sizeof(T), W, ldw * sizeof(T), kw * sizeof(T), n, hipMemcpyHostToDevice, stream));
    eig_project_dev(gen, m, (const D *)stage_r.as<D>(), m, kw, stage_x.as<D>(), kw);
    HIP_OK(hipMemcpy2DAsync(W, ldw * sizeof(T), stage_x.p, kw * sizeof(T), kw * sizeof(T), n, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
  }

  // max |Y^H BY - I| of the first m columns of eig_Y / BY, sixteen columns of Y a pass (k_eig_cgram), read back per pass
  double eig_orthonormality(int m, const D *Y, const D *BY, D *pt) {
    double worst = 0.0;
    const int rows = 16 * ((m + 15) / 16);
    for (int j0 = 0; j0 < m; j0 += 16) {
      const int kw = std::min(16, m - j0);
      eig_coeff(m, BY, kEigMaxM, kw, Y + j0, kEigMaxM, pt);
      HIP_OK(hipGetLastError());
      const D *Ch = read_back<D>(eig_C.p, (size_t)rows * 16);
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < kw; ++j) {
          const double *z = (const double *)&Ch[i * 16 + j];  // (re | im of a complex handle)
          const double re = z[0] - (i == j0 + j ? 1.0 : 0.0), im = sizeof(D) > sizeof(double) ? z[sizeof(D) / sizeof(double) - 1] : 0.0;
          const double d = std::sqrt(re * re + im * im);
          if (!(d <= worst)) worst = d;  // (a NaN stays)
        }
    }
    return worst;
  }

  // The locked sweeps: the nev <= 128 - m0 smallest eigenpairs through tiles of k <= 16 candidates, `guard` of them guard
  // columns.  Y (m0 >= 0 columns, B-orthonormal: checked to 1e-10) seeds the constraint block; every sweep runs the
  // constrained tile for want = min(nev - L, k - guard) columns, locks the leading run of p converged ones (projected once
  // more; generalized: their image under B is recomputed) and restarts from the unconverged columns plus p generated ones
  // (seed + sweep).  Host decisions (lobpcg_small.hpp) only between sweeps.  p = 0 ends the run: the tile's candidates and flags
  // fill the columns it was asked for, what was never reached stays zero with lambda = NaN and flag 2.
  // info4: total steps, sweeps, locked, smallest basis rank seen.  eig_sweeps keeps (want, locked, steps) per sweep.
  std::vector<int> eig_sweeps;
  void eigs_check(bool gen, int64_t nev, int64_t k, int64_t guard, bool has_y, int64_t ldy, int64_t m0, bool has_x0, int64_t ldx0,
                  double tol, double deftol, int maxit, int64_t ldx) {
    const int64_t room = std::max<int64_t>(1, std::min<int64_t>(k, k - guard));
    lobpcg_args(k, std::max<int64_t>(1, std::min(nev, room)), tol, deftol, maxit, ldx0, has_x0, k);
    if (const char *bad = lob::sweep_args(nev, k, guard, m0)) throw Error(HIFAMD_MISMATCHED_SIZES, bad);
    if ((m0 > 0 && ldy < m0) || ldx < nev) throw Error(HIFAMD_MISMATCHED_SIZES, "eigs: row stride smaller than the block");
    if (m0 > 0 && !has_y) throw Error(HIFAMD_NULL_OBJ, "NULL vector");
    lobpcg_handle(k, gen);
  }
  template <bool GEN>
  void eigs_run(int nev, int k, int guard, const D *dY, int64_t ldy, int m0, const D *dX0, int64_t ldx0, uint64_t seed, double tol,
                double deftol, int maxit, int64_t rank, double *lambda, D *dX, int64_t ldx, double *res, int *flags, int *info4) {
    const int64_t n = lv[0]->n;
    StreamWait wait{stream};
    eig_sweeps.clear();
    const size_t blk = (size_t)n * lob::kMaxK * sizeof(D);
    if (eig_blk.bytes < 3 * blk) eig_blk.alloc(3 * blk);
    D *Tx = eig_blk.as<D>(), *X0b = Tx + n * lob::kMaxK, *Gn = X0b + n * lob::kMaxK;  // the tile's X, the next start, generated columns
    // (the partials are asked for at every use: the tile grows ir_part, and a pointer taken before it would dangle)
    D *Y = nullptr, *BY = nullptr;
    auto blocks = [&] {  // (allocated at the first use: a run of one sweep without constraints never needs them)
      eig_blocks(true, GEN);
      Y = eig_Y.as<D>(), BY = GEN ? eig_BY.as<D>() : Y;
    };
    if (m0 > 0) {
      blocks();
      vec_op(1, n, m0, Y, kEigMaxM, dY, ldy, nullptr, 0);
      if (GEN) spmm_launch(Bm, (const D *)Y, kEigMaxM, BY, kEigMaxM, m0, stream);
      const double off = eig_orthonormality(m0, Y, BY, eig_partials());
      check_device_error();
      if (!(off <= 1e-10)) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "eigs: the constraint block Y is not B-orthonormal (max |Y^H B Y - I| = %.3g > 1e-10); "
                      "orthonormalize it first", off);
        throw Error(HIFAMD_BAD_PREC, msg);
      }
    }
    vec_op(0, n, nev, dX, ldx, nullptr, 0, nullptr, 0);
    for (int c = 0; c < nev; ++c) {
      if (lambda) lambda[c] = std::nan("");
      if (res) res[c] = std::nan("");
      if (flags) flags[c] = 2;
    }
    int m = m0, L = 0, steps = 0, minrank = 3 * k;
    const D *x0 = dX0;
    int64_t ld0 = ldx0;
    for (int t = 0;; ++t) {
      const int want = lob::sweep_want(nev, L, k, guard);
      double lam[lob::kMaxK], rs[lob::kMaxK];
      int fl[lob::kMaxK], info3[3];
      EigLock lock;
      lock.Y = Y, lock.BY = BY, lock.m = m;
      lobpcg_tile<GEN>(x0, ld0, seed, k, want, tol, deftol, maxit, rank, Tx, k, lam, rs, fl, info3, lock);
      steps += info3[0], minrank = std::min(minrank, info3[1]);
      const int p = lob::lock_prefix(fl, want);
      eig_sweeps.insert(eig_sweeps.end(), {want, p, info3[0]});
      const int shown = p > 0 ? p : want;  // columns of the tile that reach the output
      if (p > 0 && m > 0) eig_project(m, Y, BY, kEigMaxM, p, Tx, k, eig_partials());
      vec_op(1, n, shown, dX + L, ldx, (const D *)Tx, k, nullptr, 0);
      for (int c = 0; c < shown; ++c) {
        if (lambda) lambda[L + c] = lam[c];
        if (res) res[L + c] = rs[c];
        if (flags) flags[L + c] = p > 0 ? 0 : lob::unlocked_flag(fl[c]);
      }
      if (p == 0) break;
      if (L + p == nev) {
        L += p;
        break;
      }
      blocks();
      vec_op(1, n, p, Y + m, kEigMaxM, (const D *)Tx, k, nullptr, 0);
      if (GEN) spmm_launch(Bm, (const D *)(Y + m), kEigMaxM, BY + m, kEigMaxM, p, stream);
      m += p, L += p;
      // the next start block: the unconverged columns p .. k - 1 in their order, then p generated ones (the generator
      // fills a whole [n][p] block, so they pass through Gn)
      if (k - p > 0) vec_op(1, n, k - p, X0b, k, (const D *)(Tx + p), k, nullptr, 0);
      hipLaunchKernelGGL((k_idr_pfill<D>), dim3(vec_grid(n * p)), dim3(256), 0, stream, n, p, p, seed + (uint64_t)t + 1, Gn);
      vec_op(1, n, p, X0b + (k - p), k, (const D *)Gn, p, nullptr, 0);
      HIP_OK(hipGetLastError());
      x0 = X0b, ld0 = k;
    }
    HIP_OK(hipStreamSynchronize(stream));
    check_device_error();
    if (info4) info4[0] = steps, info4[1] = (int)(eig_sweeps.size() / 3), info4[2] = L, info4[3] = minrank;
  }
  void eigs_dev(bool gen, int64_t nev, int64_t k, int64_t guard, const D *dY, int64_t ldy, int64_t m0, const D *dX0, int64_t ldx0,
                uint64_t seed, double tol, double deftol, int maxit, int64_t rank, double *lambda, D *dX, int64_t ldx, double *res,
                int *flags, int *info4) {
    eigs_check(gen, nev, k, guard, dY != nullptr, ldy, m0, dX0 != nullptr, ldx0, tol, deftol, maxit, ldx);
    if (!dX) throw Error(HIFAMD_NULL_OBJ, "NULL vector");
    HIP_OK(hipSetDevice(device));
    if (gen)
      eigs_run<true>((int)nev, (int)k, (int)guard, dY, ldy, (int)m0, dX0, ldx0, seed, tol, deftol, maxit, rank, lambda, dX, ldx, res,
                     flags, info4);
    else
      eigs_run<false>((int)nev, (int)k, (int)guard, dY, ldy, (int)m0, dX0, ldx0, seed, tol, deftol, maxit, rank, lambda, dX, ldx, res,
                      flags, info4);
  }
  void eigs_host(bool gen, int64_t nev, int64_t k, int64_t guard, const T *Y, int64_t ldy, int64_t m0, const T *X0, int64_t ldx0,
                 uint64_t seed, double tol, double deftol, int maxit, int64_t rank, double *lambda, T *X, int64_t ldx, double *res,
                 int *flags, int *info4) {
    eigs_check(gen, nev, k, guard, Y != nullptr, ldy, m0, X0 != nullptr, ldx0, tol, deftol, maxit, ldx);
    if (!X) throw Error(HIFAMD_NULL_OBJ, "NULL vector");
    HIP_OK(hipSetDevice(device));
    const int64_t n = lv[0]->n;
    const size_t nx0 = (size_t)n * k * sizeof(T), nx = (size_t)n * nev * sizeof(T), ny = (size_t)n * std::max<int64_t>(m0, 1) * sizeof(T);
    if (stage_b.bytes < nx0) stage_b.alloc(nx0);
    if (stage_x.bytes < nx) stage_x.alloc(nx);
    if (m0 > 0 && stage_r.bytes < ny) stage_r.alloc(ny);
    StreamWait wait{stream};
    if (X0) HIP_OK(hipMemcpy2DAsync(stage_b.p, k * sizeof(T), X0, ldx0 * sizeof(T), k * sizeof(T), n, hipMemcpyHostToDevice, stream));
    if (m0 > 0) HIP_OK(hipMemcpy2DAsync(stage_r.p, m0 * sizeof(T), Y, ldy * sizeof(T), m0 * sizeof(T), n, hipMemcpyHostToDevice, stream));
    eigs_dev(gen, nev, k, guard, m0 > 0 ? (const D *)stage_r.as<D>() : nullptr, m0, m0, X0 ? (const D *)stage_b.as<D>() : nullptr, k, seed,
             tol, deftol, maxit, rank, lambda, stage_x.as<D>(), nev, res, flags, info4);
    HIP_OK(hipMemcpy2DAsync(X, ldx * sizeof(T), stage_x.p, nev * sizeof(T), nev * sizeof(T), n, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
  }
  // (want, locked, steps) of every sweep of the last eigs call on this engine -> the number of sweeps; at most cap triples are written
  int eigs_sweeps(int *out, int cap) const {
    const int ns = (int)(eig_sweeps.size() / 3);
    for (int i = 0; out && i < std::min(ns, cap) * 3; ++i) out[i] = eig_sweeps[(size_t)i];
    return ns;
  }

  // ---- restarted block GCR for a general pair (A, M): block CG's shared space without its conditions ------------
  // Block GMRES(m) with right preconditioning in exact arithmetic, flexible by construction.  Per cycle the true residual
  // R = B - A X (resid_dev, the handle's residual precision) is tested, normalized and factored, relative residual = Rh C
  // with Rh^H Rh = I (pivoted Cholesky, rank r); per step Z = M^{-1} Rh, W = A Z, both orthogonalized against the cycle's
  // stored blocks (C_i = Q_i^H W all from the same W), W = Q_j S1 (pivoted, rank q), P_j = Z E, D = Q_j^H Rh,
  // X += P_j D C diag(beta), Rh -= Q_j D, rel_j = sqrt(c_j^H Rh^H Rh c_j); the cycle ends on all rel <= rtol, maxit or its
  // last step, otherwise Rh is re-factored (rank r').  A flag 0 is only ever decided on a true residual at a cycle's start.
  // Q and P live in gm_Q / gm_Z (`restart` slots of [n][nc]); solve_dev and spmv_dev write Z and W straight into slot j and
  // k_bgcr_rmul turns them into P_j and Q_j in place.  Rh (and the cycle-start residual it is made from, in place) is
  // kr_vec[0].  Per step: one batched apply, one SpMM, the stacked Gram (k_bgcr_gram), the fused projection (k_bgcr_proj), a
  // Gram (k_bcg_gram), the update (k_bcg_xq), two in-place products (k_bgcr_rmul), three one-workgroup kernels and ONE
  // read-back; per cycle start one more.  Flags 0 converged / 1 stagnated, bad Gram or excluded / 2 reached maxit.
  void bgcr_tile(const D *dB, int64_t ldb, D *dX, int64_t ldx, int nc, int restart, double rtol, double deftol, int maxit,
                 int64_t rank, int *flags, int *iters, int *ranks) {
    const int64_t n = lv[0]->n, slot = n * nc;
    const size_t vec = (size_t)n * nc * sizeof(D), mat = (size_t)64 * 64 * sizeof(D);
    const size_t part = std::max((size_t)kBcgBlocks * mat, (size_t)kCgBlocks * 64 * sizeof(D));
    krylov_vectors(1, vec);
    if (gm_Q.bytes < vec * (size_t)restart) gm_Q.alloc(vec * (size_t)restart);
    if (gm_Z.bytes < vec * (size_t)restart) gm_Z.alloc(vec * (size_t)restart);
    if (ir_part.bytes < part) ir_part.alloc(part);
    D *Rh = kr_vec[0].as<D>(), *Qs = gm_Q.as<D>(), *Ps = gm_Z.as<D>(), *pt = ir_part.as<D>();
    const size_t lds_pass = 2 * mat, lds_small = bcg::Work<D>::bytes();
    const size_t lds_proj = (size_t)kBgcrGroup<D> * mat;
    raise_lds((const void *)k_bcg_xq<D>, lds_pass);
    raise_lds((const void *)k_bgcr_proj<D>, lds_proj);
    raise_lds((const void *)k_bgcr_small<D>, lds_small);
    StreamWait wait{stream};
    BgcrState<D> S;
    double *ints = nullptr;  // (a [64] double slot that holds live | aux as integers)
    krylov_state(S, {{&S.C, 64}, {&S.E1, 64}, {&S.E2, 64}, {&S.G, 64}, {&S.Cs, 64 * restart}},
                 {&S.bnorm, &S.relres, &S.rho, &S.tres, &S.mu, &ints}, rtol, maxit);
    S.deftol = deftol;
    S.live = (int *)ints;
    S.aux = S.live + 64;
    auto small = [&](int mode, int steps, bool flag) {
      hipLaunchKernelGGL((k_bgcr_small<D>), dim3(1), dim3(256), lds_small, stream, mode, steps, flag ? 1 : 0, nc, S);
    };
    auto rmul = [&](D *x1, D *x2) {  // x1 <- x1 E1 (and x2)
      hipLaunchKernelGGL((k_bgcr_rmul<D>), dim3(kBcgBlocks), dim3(256), mat, stream, n, nc, x1, x2, (const D *)S.E1);
    };
    auto state = [&] {  // ctl[0]: 0 the tile is over, 1 inside a cycle, 2 the cycle has ended
      const int go = krylov_active(S);
      HIP_OK(hipGetLastError());
      return go;
    };
    vec_op(1, n, nc, Rh, nc, dB, ldb, nullptr, 0);  // R = b
    hipLaunchKernelGGL((k_cg_dot<D>), dim3(kCgBlocks), dim3(256), 0, stream, n, nc, (const D *)Rh, (int64_t)nc, (const D *)nullptr, pt);
    hipLaunchKernelGGL((k_bcg_beta<D>), dim3(1), dim3(1024), 0, stream, (const D *)pt, nc, (BcgState<D>)S);
    vec_op(0, n, nc, dX, ldx, nullptr, 0, nullptr, 0);  // x = 0
    int steps = 0, go = 1;
    for (int cycle = 0; go != 0; ++cycle) {
      if (cycle > 0) resid_dev(dB, ldb, (const D *)dX, ldx, Rh, nc, nc, opt.resid_mode);  // the true residual
      hipLaunchKernelGGL((k_cg_dot<D>), dim3(kCgBlocks), dim3(256), 0, stream, n, nc, (const D *)Rh, (int64_t)nc,
                         (const D *)nullptr, pt);
      hipLaunchKernelGGL((k_bgcr_rho<D>), dim3(1), dim3(1024), 0, stream, (const D *)pt, nc, cycle, steps, S);
      hipLaunchKernelGGL((k_bcg_norm<D>), dim3(vec_grid(n * nc)), dim3(256), 0, stream, n, nc, Rh, (const double *)S.rho,
                         (const int *)S.live);
      block_gram(Rh, Rh, nc, pt, S.G);
      small(1, steps, cycle == 0);
      rmul(Rh, nullptr);  // Rh = Rn E
      if ((go = state()) != 1) break;
      for (int j = 0; j < restart && go == 1; ++j) {
        D *Pj = Ps + (int64_t)j * slot, *Qj = Qs + (int64_t)j * slot;
        solve_dev((const D *)Rh, nc, Pj, nc, nc, rank, nullptr);  // Z = M^{-1} Rh, into the slot
        spmv_dev((const D *)Pj, nc, Qj, nc, nc, nullptr);         // W = A Z
        ++steps;
        if (j > 0) {
          // (row blocks per stack entry: fewer as the stack grows, never more partial matrices than kBcgBlocks)
          const int nb = std::max(1, kBcgBlocks / j);
          hipLaunchKernelGGL((k_bgcr_gram<D>), dim3(j, nb), dim3(256), 0, stream, n, nc, (const D *)Qs, slot, (const D *)Qj, pt);
          hipLaunchKernelGGL((k_bgcr_sum<D>), dim3(16, j), dim3(256), 0, stream, (const D *)pt, nb, nc, S.Cs);
        }
        hipLaunchKernelGGL((k_bgcr_proj<D>), dim3(kBcgBlocks), dim3(256), lds_proj, stream, n, nc, j, (const D *)Qs,
                           (const D *)Ps, slot, (const D *)S.Cs, Qj, Pj, pt);
        hipLaunchKernelGGL((k_bcg_sum<D>), dim3(16), dim3(256), 0, stream, (const D *)pt, kBcgBlocks, nc, S.G);
        small(2, steps, false);  // W^H W -> rank q, E1
        rmul(Qj, Pj);            // Q_j = W E, P_j = Z E
        block_gram(Qj, Rh, nc, pt, S.G);
        small(3, steps, false);  // D -> E1 = D C diag(beta), E2 = D
        hipLaunchKernelGGL((k_bcg_xq<D>), dim3(kBcgBlocks), dim3(256), lds_pass, stream, n, nc, dX, ldx, Rh, (const D *)Pj,
                           (const D *)Qj, (const D *)S.E1, (const D *)S.E2, pt);
        hipLaunchKernelGGL((k_bcg_sum<D>), dim3(16), dim3(256), 0, stream, (const D *)pt, kBcgBlocks, nc, S.G);
        small(4, steps, j == restart - 1);  // rel, the end of the cycle, or the next factor of Rh
        if ((go = state()) == 1) rmul(Rh, nullptr);
      }
    }
    krylov_result(S, nc, flags, iters);
    block_ranks(S, ranks);
  }

  void bgcr_check(int block, int restart, double deftol, int maxit, double rtol) {
    krylov_check("block GCR", maxit, rtol);
    block_check(block, deftol, restart);
  }
  void bgcr_dev(const D *dB, int64_t ldb, D *dX, int64_t ldx, int64_t nrhs, int block, int restart, double rtol, double deftol,
                int maxit, int64_t rank, int *flags, int *iters, int *ranks) {
    block_batch(dB, ldb, dX, ldx, nrhs, block, flags, iters, ranks, [&] { bgcr_check(block, restart, deftol, maxit, rtol); },
                [&](const D *b, D *x, int nc, int *fl, int *it, int *rk) { bgcr_tile(b, ldb, x, ldx, nc, restart, rtol, deftol, maxit, rank, fl, it, rk); });
  }
  void bgcr_host(const T *B, int64_t ldb, T *X, int64_t ldx, int64_t nrhs, int block, int restart, double rtol, double deftol,
                 int maxit, int64_t rank, int *flags, int *iters, int *ranks) {
    staged(B, ldb, X, ldx, nrhs, false, [&] { bgcr_check(block, restart, deftol, maxit, rtol); },
           [&](const D *b, D *x) { bgcr_dev(b, nrhs, x, nrhs, nrhs, block, restart, rtol, deftol, maxit, rank, flags, iters, ranks); });
  }

  // ---- right-preconditioned BiCGSTAB, batched over columns ----------------------------------------
  // x0 = 0, r^ = b, r = b, rho = (r^, r), p = r; per iteration y = M^{-1} p, v = A y, alpha = rho / (r^, v),
  // x += alpha y, r -= alpha v, test; y = M^{-1} r, t = A y, omega = (t, r) / (t, t), x += omega y, r -= omega t, test;
  // rho' = (r^, r), beta = (rho' / rho)(alpha / omega), p = r + beta (p - omega v).  A step is one apply plus one SpMM
  // (two per iteration, maxit and iters count steps); the tests are ||r|| / ||b|| <= rtol and steps == maxit.  Up to 64
  // columns in lock step, per-column scalars in HBM (BsState), the fused k_bs_* passes each closed by k_bs_finish; the
  // host reads the active count after each of the two tests.  r^ is b itself, read in place, so the work vectors are
  // r, p, v, y, t.  Every apply goes through solve_dev, so a null-space filter on HIFAMD_S filters it.
  // Flags 0 converged / 1 breakdown / 2 reached maxit.
  DevBuf bs_part2;  // the block partials of a pass's second sum

  void bicgstab_tile(const D *dB, int64_t ldb, D *dX, int64_t ldx, int nc, double rtol, int maxit, int64_t rank,
                     int *flags, int *iters) {
    const int64_t n = lv[0]->n;
    const size_t vec = (size_t)n * nc * sizeof(D), part = (size_t)kCgBlocks * 64 * sizeof(D);
    krylov_vectors(5, vec);
    if (ir_part.bytes < part) ir_part.alloc(part);
    if (bs_part2.bytes < part) bs_part2.alloc(part);
    D *r = kr_vec[0].as<D>(), *p = kr_vec[1].as<D>(), *v = kr_vec[2].as<D>(), *y = kr_vec[3].as<D>(), *t = kr_vec[4].as<D>();
    D *pt = ir_part.as<D>(), *pt2 = bs_part2.as<D>();
    const D *rh = dB;  // r^ = b
    StreamWait wait{stream};
    BsState<D> S;
    krylov_state(S, {&S.rho, &S.alpha, &S.omega, &S.beta}, {&S.bnorm}, rtol, maxit);
    const dim3 grid(kCgBlocks), blk(256);
    auto finish = [&](int mode, int k, const D *p1) {
      hipLaunchKernelGGL((k_bs_finish<D>), dim3(1), dim3(1024), 0, stream, (const D *)pt, p1, nc, mode, k, S);
    };
    vec_op(1, n, nc, r, nc, dB, ldb, nullptr, 0);            // r = b
    hipLaunchKernelGGL((k_cg_dot<D>), grid, blk, 0, stream, n, nc, (const D *)r, (int64_t)nc, (const D *)nullptr, pt);
    finish(0, 0, nullptr);                                    // ||b||, rho = ||b||^2
    vec_op(0, n, nc, dX, ldx, nullptr, 0, nullptr, 0);        // x = 0
    vec_op(1, n, nc, p, nc, (const D *)r, nc, nullptr, 0);    // p = r
    HIP_OK(hipGetLastError());
    for (int k = 0, go = krylov_active(S); go > 0 && 2 * k < maxit; ++k) {
      solve_dev((const D *)p, nc, y, nc, nc, rank, nullptr);  // y = M^{-1} p           step 2k + 1
      spmv_dev((const D *)y, nc, v, nc, nc, nullptr);         // v = A y
      hipLaunchKernelGGL((k_cg_dot<D>), grid, blk, 0, stream, n, nc, rh, ldb, (const D *)v, pt);  // (r^, v)
      finish(1, k, nullptr);                                  // alpha = rho / (r^, v)
      hipLaunchKernelGGL((k_cg_xr<D>), grid, blk, 0, stream, n, nc, dX, ldx, r, (const D *)y, (const D *)v,
                         (const D *)S.alpha, (const int *)S.active, pt);  // x += alpha y, r -= alpha v: r holds s
      finish(2, k, nullptr);                                  // ||s|| / ||b||, maxit
      if ((go = krylov_active(S)) == 0) break;
      solve_dev((const D *)r, nc, y, nc, nc, rank, nullptr);  // y = M^{-1} s           step 2k + 2
      spmv_dev((const D *)y, nc, t, nc, nc, nullptr);         // t = A y
      hipLaunchKernelGGL((k_bs_tr<D>), grid, blk, 0, stream, n, nc, (const D *)t, (const D *)r, pt, pt2);
      finish(3, k, pt2);                                      // omega = (t, r) / (t, t)
      hipLaunchKernelGGL((k_bs_xr_full<D>), grid, blk, 0, stream, n, nc, dX, ldx, r, (const D *)y, (const D *)t, rh, ldb,
                         S, pt, pt2);
      finish(4, k, pt2);                                      // ||r|| / ||b||, maxit, beta
      if ((go = krylov_active(S)) == 0) break;
      hipLaunchKernelGGL((k_bs_p<D>), grid, blk, 0, stream, n, nc, p, (const D *)r, (const D *)v, S);
      HIP_OK(hipGetLastError());
    }
    krylov_result(S, nc, flags, iters);
  }

  void bicgstab_dev(const D *dB, int64_t ldb, D *dX, int64_t ldx, int64_t nrhs, double rtol, int maxit, int64_t rank,
                    int *flags, int *iters) {
    krylov_batch(dB, ldb, dX, ldx, nrhs, flags, iters, nullptr, [&] { krylov_check("BiCGSTAB", maxit, rtol); },
                 [&](const D *b, D *x, int nc, int *fl, int *it, int *) { bicgstab_tile(b, ldb, x, ldx, nc, rtol, maxit, rank, fl, it); });
  }
  void bicgstab_host(const T *B, int64_t ldb, T *X, int64_t ldx, int64_t nrhs, double rtol, int maxit, int64_t rank,
                     int *flags, int *iters) {
    staged(B, ldb, X, ldx, nrhs, false, [&] { krylov_check("BiCGSTAB", maxit, rtol); },
           [&](const D *b, D *x) { bicgstab_dev(b, nrhs, x, nrhs, nrhs, rtol, maxit, rank, flags, iters); });
  }

  // ---- right-preconditioned IDR(s) with biorthogonalization, batched over columns --------------------
  // van Gijzen / Sonneveld (ACM TOMS 38(1), 2011) with the "maintaining convergence" omega (kappa = 0.7), x0 = 0:
  //   r = b; G = U = 0; M = I; omega = 1
  //   cycle: f = P^H r; for k = 0 .. s-1: c = forward substitution on M[k:, k:] c = f[k:]; v = r - sum_{i>=k} c_i g_i;
  //     v^ = M^{-1} v; u = omega v^ + sum_{i>=k} c_i u_i; g = A u (a step); raw = P^H g (one pass);
  //     alpha, the new column of M and beta from raw and the stored M (k_idr_finish mode 2: no second pass over G);
  //     g_k = g - sum_{l<k} alpha_l g_l; u_k likewise; r -= beta g_k; x += beta u_k; test;
  //   v^ = M^{-1} r; t = A v^ (a step); omega from (t, r), (t, t); r -= omega t; x += omega v^; test.
  // Up to 64 columns in lock step sharing k, per-column scalars in HBM (IdState), work vectors r, v, v^, t, G_0 .., U_0 ..
  // (2 s + 4 of the pool; u is built in U_k and g = A u lands in G_k, so neither needs a vector of its own).  The shadow
  // block P [n][K] (K = s padded to 1, 2, 4, 8) is shared by all columns and tiles of a call.  The host reads the
  // active count once per step, after the stopping test.  Every apply goes through solve_dev, so a null-space filter on
  // HIFAMD_S filters it.  Flags 0 converged / 1 breakdown / 2 reached maxit.
  DevBuf id_P, id_cpart, id_C;  // P, the block partials of P^H x [K][kCgBlocks][64], P^H x [K][64]
  int id_K = 0;

  void idrs_check(int s, const T *P, int64_t ldp, int maxit, double rtol) {
    krylov_check("IDR(s)", maxit, rtol);
    if (s < 1 || s > HIFAMD_IDRS_MAX) throw Error(HIFAMD_MISMATCHED_SIZES, "need 1 <= s <= HIFAMD_IDRS_MAX");
    if (P && ldp < s) throw Error(HIFAMD_MISMATCHED_SIZES, "row stride of the shadow block smaller than s");
    if (P) {
      const int64_t n = lv[0]->n;
      for (int64_t i = 0; i < n; ++i)
        for (int j = 0; j < s; ++j)
          if (!std::isfinite(abs1_(P[i * ldp + j]))) throw Error(HIFAMD_BAD_PREC, "the shadow block has a non-finite entry");
    }
  }
  // P as [n][K] on the device: the caller's block as it is (host pointer), or the generated one
  void idrs_shadow(int s, const T *P, int64_t ldp, uint64_t seed) {
    HIP_OK(hipSetDevice(device));
    const int64_t n = lv[0]->n;
    const int K = (int)nsp_padded(s);
    if (P) {
      std::vector<T> h((size_t)n * K, T(0));
      for (int64_t i = 0; i < n; ++i)
        for (int j = 0; j < s; ++j) h[(size_t)(i * K + j)] = P[i * ldp + j];
      id_P.upload(h);
    } else {
      if (id_P.bytes < (size_t)n * K * sizeof(T)) id_P.alloc((size_t)n * K * sizeof(T));
      hipLaunchKernelGGL((k_idr_pfill<D>), dim3(vec_grid(n * K)), dim3(256), 0, stream, n, s, K, seed, id_P.as<D>());
      HIP_OK(hipGetLastError());
    }
    if (id_cpart.bytes < (size_t)K * kCgBlocks * 64 * sizeof(T)) id_cpart.alloc((size_t)K * kCgBlocks * 64 * sizeof(T));
    if (id_C.bytes < (size_t)K * 64 * sizeof(T)) id_C.alloc((size_t)K * 64 * sizeof(T));
    id_K = K;
  }
  // id_C = P^H x, x [n][nc] contiguous
  template <int K>
  void idr_coef_k(const D *x, int nc) {
    hipLaunchKernelGGL((k_nsp_coef<D, K>), dim3(kCgBlocks), dim3(256), 0, stream, lv[0]->n, nc, x, (int64_t)nc,
                       (const D *)id_P.as<D>(), id_cpart.as<D>());
    hipLaunchKernelGGL((k_nsp_finish<D>), dim3(K), dim3(1024), 0, stream, (const D *)id_cpart.as<D>(), id_C.as<D>());
  }
  void idr_coef(const D *x, int nc) {
    switch (id_K) {
      case 1: idr_coef_k<1>(x, nc); break;
      case 2: idr_coef_k<2>(x, nc); break;
      case 4: idr_coef_k<4>(x, nc); break;
      default: idr_coef_k<8>(x, nc); break;
    }
  }
  template <int S, bool U>
  void idr_comb_s(int nc, D *y, const D *z, D *const *W, const D *coef, const D *omega) {
    IdRun<D, S> run;
    for (int j = 0; j < S; ++j) run.w[j] = W[j];
    hipLaunchKernelGGL((k_idr_comb<D, S, U>), dim3(kCgBlocks), dim3(256), 0, stream, lv[0]->n, nc, y, z, run, coef, omega);
  }
  template <bool U>
  void idr_comb(int m, int nc, D *y, const D *z, D *const *W, const D *coef, const D *omega) {
    switch (m) {
      case 1: idr_comb_s<1, U>(nc, y, z, W, coef, omega); break;
      case 2: idr_comb_s<2, U>(nc, y, z, W, coef, omega); break;
      case 3: idr_comb_s<3, U>(nc, y, z, W, coef, omega); break;
      case 4: idr_comb_s<4, U>(nc, y, z, W, coef, omega); break;
      case 5: idr_comb_s<5, U>(nc, y, z, W, coef, omega); break;
      case 6: idr_comb_s<6, U>(nc, y, z, W, coef, omega); break;
      case 7: idr_comb_s<7, U>(nc, y, z, W, coef, omega); break;
      default: idr_comb_s<8, U>(nc, y, z, W, coef, omega); break;
    }
  }
  template <int S>
  void idr_gu_s(int nc, D *x, int64_t ldx, D *r, D *const *G, D *const *U, const IdState<D> &St, D *pt) {
    IdRun<D, S> g, u;
    for (int l = 0; l < S; ++l) g.w[l] = G[l], u.w[l] = U[l];
    hipLaunchKernelGGL((k_idr_gu<D, S>), dim3(kCgBlocks), dim3(256), 0, stream, lv[0]->n, nc, x, ldx, r, G[S], U[S], g, u, St, pt);
  }
  void idr_gu(int k, int nc, D *x, int64_t ldx, D *r, D *const *G, D *const *U, const IdState<D> &St, D *pt) {
    switch (k) {
      case 0: idr_gu_s<0>(nc, x, ldx, r, G, U, St, pt); break;
      case 1: idr_gu_s<1>(nc, x, ldx, r, G, U, St, pt); break;
      case 2: idr_gu_s<2>(nc, x, ldx, r, G, U, St, pt); break;
      case 3: idr_gu_s<3>(nc, x, ldx, r, G, U, St, pt); break;
      case 4: idr_gu_s<4>(nc, x, ldx, r, G, U, St, pt); break;
      case 5: idr_gu_s<5>(nc, x, ldx, r, G, U, St, pt); break;
      case 6: idr_gu_s<6>(nc, x, ldx, r, G, U, St, pt); break;
      default: idr_gu_s<7>(nc, x, ldx, r, G, U, St, pt); break;
    }
  }

  void idrs_tile(const D *dB, int64_t ldb, D *dX, int64_t ldx, int nc, int s, double rtol, int maxit, int64_t rank,
                 int *flags, int *iters) {
    const int64_t n = lv[0]->n;
    const size_t vec = (size_t)n * nc * sizeof(D), part = (size_t)kCgBlocks * 64 * sizeof(D);
    krylov_vectors(2 * s + 4, vec);
    if (ir_part.bytes < part) ir_part.alloc(part);
    if (bs_part2.bytes < part) bs_part2.alloc(part);
    D *r = kr_vec[0].as<D>(), *v = kr_vec[1].as<D>(), *vh = kr_vec[2].as<D>(), *t = kr_vec[3].as<D>();
    D *G[kIdrMax], *U[kIdrMax];
    for (int i = 0; i < s; ++i) G[i] = kr_vec[4 + i].as<D>(), U[i] = kr_vec[4 + s + i].as<D>();
    D *pt = ir_part.as<D>(), *pt2 = bs_part2.as<D>();
    const D *C = id_C.as<D>();
    StreamWait wait{stream};
    IdState<D> S;
    S.s = s;
    krylov_state(S, {{&S.M, s * s}, {&S.f, s}, {&S.c, s}, {&S.alpha, s}, {&S.omega, 1}, {&S.beta, 1}}, {&S.bnorm, &S.rr}, rtol,
                 maxit);
    const dim3 grid(kCgBlocks), blk(256);
    auto finish = [&](int mode, int k, int step, const D *p0, const D *p1) {
      hipLaunchKernelGGL((k_idr_finish<D>), dim3(1), dim3(1024), 0, stream, p0, p1, C, nc, mode, k, step, S);
    };
    vec_op(1, n, nc, r, nc, dB, ldb, nullptr, 0);            // r = b
    hipLaunchKernelGGL((k_cg_dot<D>), grid, blk, 0, stream, n, nc, (const D *)r, (int64_t)nc, (const D *)nullptr, pt);
    finish(0, 0, 0, pt, nullptr);                             // ||b||, omega = 1, M = I
    vec_op(0, n, nc, dX, ldx, nullptr, 0, nullptr, 0);        // x = 0
    for (int i = 0; i < s; ++i) {                             // G = U = 0
      HIP_OK(hipMemsetAsync(G[i], 0, vec, stream));
      HIP_OK(hipMemsetAsync(U[i], 0, vec, stream));
    }
    HIP_OK(hipGetLastError());
    int step = 0, go = krylov_active(S);
    while (go > 0 && step < maxit) {
      idr_coef(r, nc);
      finish(1, 0, step, nullptr, nullptr);                   // f = P^H r, c
      for (int k = 0; k < s && go > 0; ++k, ++step) {
        idr_comb<false>(s - k, nc, v, r, G + k, S.c + k * 64, nullptr);       // v = r - sum c_i g_i
        solve_dev((const D *)v, nc, vh, nc, nc, rank, nullptr);               // v^ = M^{-1} v
        idr_comb<true>(s - k, nc, U[k], vh, U + k, S.c + k * 64, S.omega);    // u = omega v^ + sum c_i u_i, in U_k
        spmv_dev((const D *)U[k], nc, G[k], nc, nc, nullptr);                 // g = A u, in G_k
        idr_coef(G[k], nc);
        finish(2, k, step, nullptr, nullptr);                 // alpha, M[:, k], beta, f, the next c
        idr_gu(k, nc, dX, ldx, r, G, U, S, pt);
        finish(3, k, step, pt, nullptr);                      // ||r|| / ||b||, maxit
        HIP_OK(hipGetLastError());
        go = krylov_active(S);
      }
      if (go == 0) break;
      solve_dev((const D *)r, nc, vh, nc, nc, rank, nullptr);  // v^ = M^{-1} r
      spmv_dev((const D *)vh, nc, t, nc, nc, nullptr);         // t = A v^
      hipLaunchKernelGGL((k_bs_tr<D>), grid, blk, 0, stream, n, nc, (const D *)t, (const D *)r, pt, pt2);
      finish(4, 0, step, pt, pt2);                             // omega
      hipLaunchKernelGGL((k_cg_xr<D>), grid, blk, 0, stream, n, nc, dX, ldx, r, (const D *)vh, (const D *)t,
                         (const D *)S.omega, (const int *)S.active, pt);  // x += omega v^, r -= omega t
      finish(3, 0, step, pt, nullptr);
      HIP_OK(hipGetLastError());
      ++step;
      go = krylov_active(S);
    }
    krylov_result(S, nc, flags, iters);
  }

  void idrs_dev(const D *dB, int64_t ldb, D *dX, int64_t ldx, int64_t nrhs, int s, const T *P, int64_t ldp, uint64_t seed,
                double rtol, int maxit, int64_t rank, int *flags, int *iters) {
    krylov_batch(dB, ldb, dX, ldx, nrhs, flags, iters, nullptr,
                 [&] {
                   idrs_check(s, P, ldp, maxit, rtol);
                   idrs_shadow(s, P, ldp, seed);
                 },
                 [&](const D *b, D *x, int nc, int *fl, int *it, int *) { idrs_tile(b, ldb, x, ldx, nc, s, rtol, maxit, rank, fl, it); });
  }
  void idrs_host(const T *B, int64_t ldb, T *X, int64_t ldx, int64_t nrhs, int s, const T *P, int64_t ldp, uint64_t seed,
                 double rtol, int maxit, int64_t rank, int *flags, int *iters) {
    staged(B, ldb, X, ldx, nrhs, false, [&] { idrs_check(s, P, ldp, maxit, rtol); },
           [&](const D *b, D *x) { idrs_dev(b, nrhs, x, nrhs, nrhs, s, P, ldp, seed, rtol, maxit, rank, flags, iters); });
  }

  // ---- symmetric QMR for a Hermitian indefinite pair, batched over columns ---------------------------
  // PCG's coupled two-term recurrence without the positivity requirement, plus the quasi-minimal-residual smoothing of
  // Freund and Nachtigal: x0 = 0, r = s = b, tau = ||b||, theta = 0, d = g = 0, z = M^{-1} r, rho = r^H z, p = z; per
  // iteration q = A p, sigma = p^H q, alpha = rho / sigma, r -= alpha q, theta' = ||r|| / tau, c^2 = 1 / (1 + theta'^2),
  // tau = tau theta' sqrt(c^2), eta = c^2 theta^2, zeta = c^2 alpha, theta = theta', d = eta d + zeta p,
  // g = eta g + zeta q, x += d, s -= g (s = b - A x by recurrence), stop on ||s|| / ||b|| <= rtol, z = M^{-1} r,
  // rho' = r^H z, p = z + (rho' / rho) p.  One apply and one SpMM per iteration (PCG's unit), seven work vectors
  // r, z, p, q, d, g, s.  Up to 64 columns in lock step, per-column scalars in HBM (QmState), every reduction closed by
  // k_qm_finish; the host reads the active count once per iteration, after the convergence test.  Only for a Hermitian
  // M^{-1} (import.hpp check_hermitian); a breakdown is rho or sigma exactly zero or not finite.  With a basis filter on
  // HIFAMD_S the iteration runs projected as PCG's does.  Flags 0 converged / 1 breakdown / 2 reached maxit.

  void sqmr_tile(const D *dB, int64_t ldb, D *dX, int64_t ldx, int nc, double rtol, int maxit, int64_t rank, int *flags,
                 int *iters) {
    const int64_t n = lv[0]->n;
    const size_t vec = (size_t)n * nc * sizeof(D), part = (size_t)kCgBlocks * 64 * sizeof(D);
    krylov_vectors(7, vec);
    if (ir_part.bytes < part) ir_part.alloc(part);
    D *r = kr_vec[0].as<D>(), *z = kr_vec[1].as<D>(), *p = kr_vec[2].as<D>(), *q = kr_vec[3].as<D>(), *d = kr_vec[4].as<D>(),
      *g = kr_vec[5].as<D>(), *s = kr_vec[6].as<D>(), *pt = ir_part.as<D>();
    StreamWait wait{stream};
    QmState<D> S;
    krylov_state(S, {&S.rho, &S.alpha, &S.beta, &S.zeta}, {&S.eta, &S.tau, &S.theta, &S.bnorm}, rtol, maxit);
    const dim3 grid(kCgBlocks), blk(256);
    auto dot = [&](const D *a, const D *b) {
      hipLaunchKernelGGL((k_cg_dot<D>), grid, blk, 0, stream, n, nc, a, (int64_t)nc, b, pt);
    };
    auto finish = [&](int mode, int k) {
      hipLaunchKernelGGL((k_qm_finish<D>), dim3(1), dim3(1024), 0, stream, (const D *)pt, nc, mode, k, S);
    };
    vec_op(1, n, nc, r, nc, dB, ldb, nullptr, 0);  // r = b
    // projected: with a basis filter P = I - Q Q^H on the solve, r0 = s0 = P b, ||b|| := ||P b||, and every
    // z = M^{-1} r below is already P M^{-1} r (solve_dev filters it)
    if (nsp_k > 0) apply_nsp(r, nc, nc, stream);
    dot(r, nullptr);
    finish(0, 0);                                           // ||b||, tau
    vec_op(1, n, nc, s, nc, (const D *)r, nc, nullptr, 0);  // s = r
    vec_op(0, n, nc, d, nc, nullptr, 0, nullptr, 0);        // d = g = 0, x = 0
    vec_op(0, n, nc, g, nc, nullptr, 0, nullptr, 0);
    vec_op(0, n, nc, dX, ldx, nullptr, 0, nullptr, 0);
    solve_dev((const D *)r, nc, z, nc, nc, rank, nullptr);  // z = M^{-1} r
    dot(r, z);
    finish(1, 0);                                           // rho = r^H z
    vec_op(1, n, nc, p, nc, (const D *)z, nc, nullptr, 0);  // p = z
    HIP_OK(hipGetLastError());
    // (one read-back per iteration, after the convergence test; a column that breaks down in mode 5 costs one frozen pass)
    for (int k = 0, go = krylov_active(S); k < maxit && go > 0; ++k) {
      spmv_dev((const D *)p, nc, q, nc, nc, nullptr);       // q = A p
      dot(p, q);
      finish(2, k);                                         // alpha = rho / p^H q
      hipLaunchKernelGGL((k_qm_r<D>), grid, blk, 0, stream, n, nc, r, (const D *)q, (const D *)S.alpha, (const int *)S.active, pt);
      finish(3, k);                                         // theta, c^2, tau, eta, zeta
      hipLaunchKernelGGL((k_qm_ds<D>), grid, blk, 0, stream, n, nc, dX, ldx, s, d, g, (const D *)p, (const D *)q, S, pt);
      finish(4, k);                                         // ||s|| / ||b||, maxit
      if ((go = krylov_active(S)) == 0) break;
      solve_dev((const D *)r, nc, z, nc, nc, rank, nullptr);
      dot(r, z);
      finish(5, k);                                         // beta = rho' / rho
      hipLaunchKernelGGL((k_cg_p<D>), grid, blk, 0, stream, n, nc, p, (const D *)z, (const D *)S.beta, (const int *)S.active);
      HIP_OK(hipGetLastError());
    }
    krylov_result(S, nc, flags, iters);
  }

  void sqmr_check(int maxit, double rtol) {
    krylov_check("symmetric QMR", maxit, rtol);
    hermitian_check("symmetric QMR", "GMRES or BiCGSTAB", "a constant null-space filter");
  }
  void sqmr_dev(const D *dB, int64_t ldb, D *dX, int64_t ldx, int64_t nrhs, double rtol, int maxit, int64_t rank,
                int *flags, int *iters) {
    krylov_batch(dB, ldb, dX, ldx, nrhs, flags, iters, nullptr, [&] { sqmr_check(maxit, rtol); },
                 [&](const D *b, D *x, int nc, int *fl, int *it, int *) { sqmr_tile(b, ldb, x, ldx, nc, rtol, maxit, rank, fl, it); });
  }
  void sqmr_host(const T *B, int64_t ldb, T *X, int64_t ldx, int64_t nrhs, double rtol, int maxit, int64_t rank,
                 int *flags, int *iters) {
    staged(B, ldb, X, ldx, nrhs, false, [&] { sqmr_check(maxit, rtol); },
           [&](const D *b, D *x) { sqmr_dev(b, nrhs, x, nrhs, nrhs, rtol, maxit, rank, flags, iters); });
  }

  // ---- on-disk form of the imported hierarchy (import.hpp save_hierarchy / load_hierarchy) -----------------
  void save(std::FILE *f, int flags = 0) const {
    if (adjoint || is_twin) throw Error(HIFAMD_HIFIR_ERROR, "internal engines are not saved");
    save_hierarchy(f, host);
    if (flags & HIFAMD_SAVE_ANALYSIS) save_analysis(f, host, opt.band);
  }
  void load(std::FILE *f) {
    if (env_int("HIFIR_AMD_LOAD_ANALYSIS", 1)) load_analysis<T>(f, opt.band, cached_analysis);
    try {
      load_hierarchy<T>(f, *this);
    } catch (...) {
      std::vector<LevelAnalysis<T>>().swap(cached_analysis);
      throw;
    }
    std::vector<LevelAnalysis<T>>().swap(cached_analysis);
  }

  // development aid: one checksum per device-resident array (order documented in tests), to tell which
  // upload differs when two handles built from the same hierarchy disagree
  static uint64_t cksum(const DevBuf &b) {
    if (!b.p || !b.bytes) return 0;
    std::vector<unsigned char> h(b.bytes);
    copy_d2h(h.data(), b.p, b.bytes);
    uint64_t s = 1469598103934665603ull;
    for (unsigned char c : h) s = (s ^ c) * 1099511628211ull;
    return s;
  }
  int debug_checksums(uint64_t *out, int cap) const {
    std::vector<uint64_t> v;
    for (const auto &Lp : lv) {
      const DevLevel &L = *Lp;
      for (const DevCsr *M : {&L.L, &L.U, &L.E, &L.F})
        for (const DevBuf *b : {&M->ptr, &M->col, &M->val, &M->rowid, &M->srcslot, &M->split, &M->wg_grp_ptr, &M->grp_slot_ptr, &M->tinv})
          v.push_back(cksum(*b));
      for (const DevBuf *b : {&L.d, &L.s, &L.t, &L.p, &L.qinv, &L.topG}) v.push_back(cksum(*b));
    }
    v.push_back(cksum(tailG));
    for (const DevBuf *b : {&dn.QH, &dn.Rinv, &dn.jpvt0}) v.push_back(cksum(*b));
    v.push_back((uint64_t)dn.rank);
    for (int i = 0; i < cap && i < (int)v.size(); ++i) out[i] = v[(size_t)i];
    return (int)v.size();
  }

  // operator selection of lhf?Apply (libhifir.cpp:447-472): S on this engine, SH on the adjoint one
  Engine<T> &for_op(int op) {
    if (op == HIFAMD_S || op == HIFAMD_M) return *this;
    if (op == HIFAMD_SH || op == HIFAMD_MH) return adjoint_engine();
    throw Error(HIFAMD_MISMATCHED_SIZES, "unknown operator tag");
  }
  static int kind_of(int op) { return (op == HIFAMD_M || op == HIFAMD_MH) ? 1 : 0; }

  // host-pointer product (lhf?Apply with LHF_M / LHF_MH: direct, no refinement, libhifir.cpp:457-460)
  void prod_host(const T *B, int64_t ldb, T *X, int64_t ldx, int64_t nrhs, int64_t rank) {
    staged(B, ldb, X, ldx, nrhs, true, [] {}, [&](const D *b, D *x) { solve_dev(b, nrhs, x, nrhs, nrhs, rank, nullptr, 1); });
  }

  // ---- stats ----------------------------------------------------------------------------------
  void stats(double *o) const {
    for (int i = 0; i < 16; ++i) o[i] = 0.0;
    const double sv = sizeof(T), si = 4, sp = 8, ss = 8;
    double bmat = 0, bvec = 0;
    int64_t wfL = 0, wfU = 0;
    for (const auto &H : host.levels) {
      const double m = (double)H.m, n = (double)H.n;
      const double nl = (double)H.L.nnz(), nu = (double)H.U.nnz(), ne = (double)H.E.nnz(), nf = (double)H.F.nnz();
      o[0] += n;
      o[1] += m;
      o[2] += nl + nu;
      o[3] += ne + nf;
      // matrices streamed once per use (LU twice), vectors once per stage
      bmat += 2 * (nl + nu) * (sv + si) + (ne + nf) * (sv + si) + 2 * m * sv + 4 * (m + 1) * sp + (n + 2) * sp +
              n * (2 * si + 2 * ss);
      bvec += sv * (7 * n + 4 * m);
      wfL += H.Ls.nwf();
      wfU += H.Us.nwf();
      o[11] += (double)(H.Lp.nbands() + H.Up.nbands());
      o[12] += (double)(H.Lp.nwg() + H.Up.nwg());
    }
    if (host.has_dense) {
      o[4] = (double)host.dense.n;
      bmat += (double)host.dense.n * (double)host.dense.n * sv;
    }
    o[5] = bmat;
    o[6] = bvec;
    o[7] = (double)wfL;
    o[8] = (double)wfU;
    o[9] = (double)last_launches;
    o[10] = (double)host.levels.size();
    o[13] = finalize_seconds;
    o[14] = bytes_inverses + bytes_top + bytes_tail;
    o[15] = capture_ms;
  }
  // of this handle's last batched apply, whichever of its two engines ran it
  int kernel_census(int32_t *o, int cap) const {
    const Engine<T> &E = (adj && adj->census_seq > census_seq) ? *adj : *this;
    for (int i = 0; i < cap && i < (int)E.last_census.size(); ++i) o[i] = E.last_census[(size_t)i];
    return (int)E.last_census.size();
  }
  int launch_map(int32_t *o, int cap) const {
    for (int i = 0; i < cap && i < (int)last_map.size(); ++i) o[i] = last_map[(size_t)i];
    return (int)last_map.size();
  }
  int level_stats(int level, double *o, int cap) const {
    if (level < 0 || level >= (int)host.levels.size()) return -1;
    const auto &H = host.levels[(size_t)level];
    const double v[] = {(double)H.m, (double)H.n, (double)H.L.nnz(), (double)H.U.nnz(), (double)H.E.nnz(), (double)H.F.nnz(),
                        (double)H.Ls.nwf(), (double)H.Us.nwf(), (double)H.Lp.nbands(), (double)H.Up.nbands(), (double)H.top_n};
    const int nv = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < cap && i < nv; ++i) o[i] = v[i];
    return nv;
  }
  // set-up / operator accounting beyond the 16 slots of hifamd_stats (hifir_amd.h hifamd_stats_ext)
  int stats_ext(double *o, int cap) const {
    // resident bytes of this handle beside the explicit operators: the work arena of every level (w + v, Rmax columns),
    // the coefficient tiles of the component bands, the factors with their plan arrays
    double arena = 0.0, tiles = 0.0, factors = 0.0, skip_w = 0.0, skip_v = 0.0;
    double ls_src = 0.0, ls_dep = 0.0, ls_c = 0.0;  // k_band_ls: rows streamed, rows kept in LDS, the largest chunk (rows)
    double cd_comps = 0.0, cd_shared = 0.0, ls_nch = 0.0;  // components of component bands, workgroups with several, most chunks (k_band_ls)
    for (const auto &L : lv) {
      for (size_t b = 0; b < L->L.ls_band_ok.size() && b < L->L.ls_band_nch.size(); ++b)
        if (L->L.ls_band_ok[b]) ls_nch = std::max(ls_nch, (double)L->L.ls_band_nch[b]);
      ls_src += (double)L->L.ls_sources, ls_dep += (double)L->L.ls_deps, ls_c = std::max(ls_c, (double)L->L.ls_chunk_rows);
      arena += (double)L->arena.bytes;
      skip_w += (double)L->skip_w;
      skip_v += (double)L->skip_v;
      for (const DevCsr *M : {&L->L, &L->U, &L->E, &L->F}) {
        for (size_t b = 0; b < M->band_cd.size() && b + 1 < M->band_wg_ptr.size(); ++b) {
          if (!M->band_cd[b]) continue;
          for (int32_t g = M->band_wg_ptr[b]; g < M->band_wg_ptr[b + 1] && (size_t)g + 1 < M->host_wg_grp_ptr.size(); ++g) {
            const int32_t nc = M->host_wg_grp_ptr[(size_t)g + 1] - M->host_wg_grp_ptr[(size_t)g];
            cd_comps += (double)nc, cd_shared += nc > 1 ? 1.0 : 0.0;
          }
        }
        tiles += (double)(M->ct_sptr.bytes + M->ct_src.bytes + M->ct_coef.bytes + M->ct_desc.bytes);
        factors += (double)(M->ptr.bytes + M->col.bytes + M->val.bytes + M->rowid.bytes + M->srcslot.bytes + M->split.bytes + M->csplit.bytes +
                            M->cd_desc.bytes + M->mid_col.bytes + M->mid_val.bytes + M->mid_lrow.bytes + M->own_val.bytes + M->f_col.bytes +
                            M->f_val.bytes + M->tl_ucol.bytes + M->tl_coef.bytes);
      }
    }
    const double v[] = {finalize_seconds, capture_ms,     bytes_inverses,  bytes_top,     bytes_tail,           (double)tail_n,
                        (double)tail_level, tail_probe_err, tail_max_abs, (double)tail_rejected, opt.tail_probe_tol, opt.tail_max_growth,
                        (double)levels_from_cache, analysis_seconds, arena, (double)Rmax, tiles, factors, (double)max_nrhs,
                        skip_w, skip_v, (double)host_repairs,
                        (double)(nsp_Q.bytes + (adj ? adj->nsp_Q.bytes : 0)), ls_src, ls_dep, ls_c,
                        cd_comps, cd_shared, ls_nch, (double)opt.zop_flags};
    const int nv = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < cap && i < nv; ++i) o[i] = v[i];
    return nv;
  }

  int64_t nnz_total() const {
    int64_t z = 0;
    for (const auto &H : host.levels) {
      if (H.m) z += H.L.nnz() + H.U.nnz() + H.m;
      if (H.n - H.m) z += H.E.nnz() + H.F.nnz();
    }
    if (host.has_dense) z += host.dense.n * host.dense.n;
    return z;
  }
};

}  // namespace hifamd

// =============================================================================================
// C ABI
// =============================================================================================
using namespace hifamd;

struct HifAmdPrec {
  int vt;
  EngineBase *eng;
};

#define API_BEGIN                                      \
  if (!h || !h->eng) {                                 \
    set_err("NULL handle");                            \
    return HIFAMD_NULL_OBJ;                            \
  }                                                    \
  try {
#define API_END                                        \
  }                                                    \
  catch (const Error &e) {                             \
    set_err(e.what());                                 \
    return (HifAmdStatus)e.code;                       \
  }                                                    \
  catch (const std::exception &e) {                    \
    set_err(e.what());                                 \
    return HIFAMD_HIFIR_ERROR;                         \
  }                                                    \
  return HIFAMD_SUCCESS;

// f(the handle's engine under its own type); the casts of an entry's untyped blocks come from that type (Engine::val, dev)
template <class F>
static decltype(auto) visit(HifAmdPrec *h, F &&f) {
  if (h->vt == HIFAMD_D) return f(*(Engine<double> *)h->eng);
  return f(*(Engine<zdouble> *)h->eng);
}

template <class E>
static int64_t q_nrows(E *e) {
  return e->host.levels.empty() ? 0 : e->host.levels[0].n;
}

template <class E>
static int64_t q_levels(E *e) {
  return (int64_t)e->host.levels.size() + (e->host.has_dense ? 1 : 0);
}

template <class E>
static int64_t q_schur_size(E *e) {
  return e->host.levels.empty() ? 0 : e->host.levels.back().n - e->host.levels.back().m;
}

template <class E>
static int64_t q_schur_rank(E *e) {
  return e->host.has_dense ? e->host.dense.rank : 0;
}

template <class E>
static void do_schedule(E *e, int level, int which, int64_t *nwf, int32_t *order, int64_t *wf_ptr) {
  if (level < 0 || level >= (int)e->host.levels.size()) throw Error(HIFAMD_MISMATCHED_SIZES, "level out of range");
  const Schedule &S = which == 0 ? e->host.levels[(size_t)level].Ls : e->host.levels[(size_t)level].Us;
  if (nwf) *nwf = S.nwf();
  if (order) std::copy(S.order.begin(), S.order.end(), order);
  if (wf_ptr) std::copy(S.wf_ptr.begin(), S.wf_ptr.end(), wf_ptr);
}

template <class E, class D>
static void do_time(E *e, const D *dB, int64_t ldb, D *dX, int64_t ldx, int64_t nrhs, int64_t rank, int warmup, int reps,
                    double *ms_avg) {
  if (!ms_avg) throw Error(HIFAMD_NULL_OBJ, "NULL output");
  for (int i = 0; i < warmup; ++i) e->solve_dev(dB, ldb, dX, ldx, nrhs, rank, nullptr);
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  HIP_OK(hipEventRecord(e0, e->stream));
  for (int i = 0; i < reps; ++i) e->solve_dev(dB, ldb, dX, ldx, nrhs, rank, nullptr);
  HIP_OK(hipEventRecord(e1, e->stream));
  HIP_OK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  e->check_device_error();
  *ms_avg = (double)ms / (reps > 0 ? reps : 1);
}

template <class E>
static void do_copy_columns(E *e, const void *src, int64_t lds, int64_t ncols, void *dst, int64_t ldd, int64_t col0) {
  if (!e->finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
  if (!src || !dst) throw Error(HIFAMD_NULL_OBJ, "NULL vector");
  if (ncols < 1 || lds < ncols || col0 < 0 || ldd < col0 + ncols) throw Error(HIFAMD_MISMATCHED_SIZES, "column block does not fit");
  HIP_OK(hipSetDevice(e->device));
  const int64_t n = e->lv[0]->n;
  const size_t elem = sizeof(typename E::value_type);
  // a destination on ANOTHER device: the copy is a peer copy and needs peer access from this handle's device (enabled
  // once per pair; "already enabled" is fine); where the platform grants none the call fails loudly instead of a copy
  // that the runtime would stage or refuse at its own discretion
  hipPointerAttribute_t pa;
  if (hipPointerGetAttributes(&pa, dst) == hipSuccess && pa.type == hipMemoryTypeDevice && pa.device != e->device) {
    int can = 0;
    HIP_OK(hipDeviceCanAccessPeer(&can, e->device, pa.device));
    if (!can) throw Error(HIFAMD_HIFIR_ERROR, "no peer access between the two devices of a column-block copy");
    const hipError_t pe = hipDeviceEnablePeerAccess(pa.device, 0);
    if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) HIP_OK(pe);
    (void)hipGetLastError();
  } else {
    (void)hipGetLastError();  // (a host pointer: not an error here)
  }
  HIP_OK(hipMemcpy2DAsync((char *)dst + (size_t)col0 * elem, (size_t)ldd * elem, src, (size_t)lds * elem, (size_t)ncols * elem,
                          (size_t)n, hipMemcpyDefault, e->stream));
}
template <class E>
static void do_sync(E *e) {
  if (!e->finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
  HIP_OK(hipSetDevice(e->device));
  HIP_OK(hipStreamSynchronize(e->stream));
  e->check_device_error();
}

// the engine whose filter op names, or NULL when that is the adjoint engine and it was never built (no filter then)
template <class E>
static E *nsp_engine(E *e, HifAmdOp op) {
  if (op != HIFAMD_S && op != HIFAMD_SH) throw Error(HIFAMD_MISMATCHED_SIZES, "the filter belongs to HIFAMD_S or HIFAMD_SH");
  if (!e->finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
  if (op == HIFAMD_S) return e;
  return e->adj ? e->adj.get() : nullptr;
}

// what refuses a residual call before the adjoint engine would be built for it
template <class E>
static void residual_pre(E *e, HifAmdOp op, int mode) {
  if (op != HIFAMD_S && op != HIFAMD_SH) throw Error(HIFAMD_MISMATCHED_SIZES, "the residual belongs to HIFAMD_S (A) or HIFAMD_SH (A^H)");
  if (mode < -1 || mode > HIFAMD_RESID_COMPENSATED) throw Error(HIFAMD_MISMATCHED_SIZES, "residual mode: -1, 0 or 1");
  if (!e->finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
  if (!e->has_A) throw Error(HIFAMD_BAD_PREC, "the residual needs the matrix (hifamd_set_matrix)");
}

extern "C" {

const char *hifamd_version(void) { return "hifir_amd 0.1.0 (gfx950)"; }

const char *hifamd_last_error(void) {
  if (!g_has_err) return nullptr;
  g_has_err = false;
  return g_err.c_str();
}

int hifamd_device_count(void) {
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
  return cnt;
}

HifAmdStatus hifamd_create(HifAmdValueType vt, int device, HifAmdHdl *out) {
  if (!out) {
    set_err("NULL output handle");
    return HIFAMD_NULL_OBJ;
  }
  *out = nullptr;
  try {
    EngineBase *e = nullptr;
    if (vt == HIFAMD_D)
      e = new Engine<double>(device, EngineOptions::from_env(false));
    else if (vt == HIFAMD_Z)
      e = new Engine<zdouble>(device, EngineOptions::from_env(true));
    else
      throw Error(HIFAMD_BAD_PREC, "unknown value type");
    HifAmdPrec *h = new HifAmdPrec{(int)vt, e};
    *out = h;
  } catch (const Error &e) {
    set_err(e.what());
    return (HifAmdStatus)e.code;
  } catch (const std::exception &e) {
    set_err(e.what());
    return HIFAMD_HIFIR_ERROR;
  }
  return HIFAMD_SUCCESS;
}

HifAmdStatus hifamd_destroy(HifAmdHdl h) {
  if (!h) return HIFAMD_SUCCESS;
  delete h->eng;
  delete h;
  return HIFAMD_SUCCESS;
}

HifAmdStatus hifamd_add_level(HifAmdHdl h, int64_t m, int64_t n, const int64_t *Lcp, const int32_t *Lri,
                              const void *Lv, const int64_t *Ucp, const int32_t *Uri, const void *Uv,
                              const int64_t *Ecp, const int32_t *Eri, const void *Ev, int64_t F_ncols,
                              const int64_t *Fcp, const int32_t *Fri, const void *Fv, const void *d,
                              const double *s, const double *t, const int32_t *p, const int32_t *p_inv,
                              const int32_t *q, const int32_t *q_inv) {
  API_BEGIN
  visit(h, [&](auto &E) {
    E.add_level(m, n, Lcp, Lri, E.val(Lv), Ucp, Uri, E.val(Uv), Ecp, Eri, E.val(Ev), F_ncols, Fcp, Fri, E.val(Fv), E.val(d), s,
                t, p, p_inv, q, q_inv);
  });
  API_END
}

HifAmdStatus hifamd_set_nsp_const(HifAmdHdl h, HifAmdOp op, int64_t start, int64_t end) {
  API_BEGIN
  if (op != HIFAMD_S && op != HIFAMD_SH) throw Error(HIFAMD_MISMATCHED_SIZES, "the filter belongs to HIFAMD_S or HIFAMD_SH");
  const bool on = !(end >= 0 && start > end);
  // (one filter per op: a constant-mode filter that is switched on replaces a basis)
  visit(h, [&](auto &P) {
    auto &E = P.for_op(op);
    E.nsp_on = on, E.nsp_r0 = start, E.nsp_r1 = end;
    if (on && E.nsp_k > 0) E.set_nsp_basis(0, nullptr, 0);
  });
  API_END
}

HifAmdStatus hifamd_set_nsp_basis(HifAmdHdl h, HifAmdOp op, int64_t k, const void *V, int64_t ldv) {
  API_BEGIN
  if (op != HIFAMD_S && op != HIFAMD_SH) throw Error(HIFAMD_MISMATCHED_SIZES, "the filter belongs to HIFAMD_S or HIFAMD_SH");
  if (k < 0 || k > HIFAMD_NSP_MAX) throw Error(HIFAMD_MISMATCHED_SIZES, "a null-space basis has 0 to 16 vectors (HIFAMD_NSP_MAX)");
  if (k > 0 && (!V || ldv < k)) throw Error(HIFAMD_MISMATCHED_SIZES, "null-space basis: NULL array or row stride smaller than k");
  visit(h, [&](auto &E) {
    if (!E.finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
    // (removing a filter from an adjoint engine that was never built has nothing to do)
    if (k == 0 && op == HIFAMD_SH && !E.adj) return;
    E.for_op(op).set_nsp_basis(k, E.val(V), ldv);
  });
  API_END
}

int64_t hifamd_nsp_dim(HifAmdHdl h, HifAmdOp op) {
  if (!h || !h->eng) return -1;
  return visit(h, [&](auto &E) -> int64_t {
    if (op == HIFAMD_S) return E.nsp_k;
    if (op == HIFAMD_SH) return E.adj ? E.adj->nsp_k : 0;
    return 0;
  });
}

HifAmdStatus hifamd_nsp_filter_batch(HifAmdHdl h, HifAmdOp op, void *X, int64_t ldx, int64_t nrhs) {
  API_BEGIN
  visit(h, [&](auto &E) {
    if (auto *F = nsp_engine(&E, op)) F->nsp_filter_host(E.val(X), ldx, nrhs);
  });
  API_END
}

HifAmdStatus hifamd_nsp_filter_batch_dev(HifAmdHdl h, HifAmdOp op, void *dX, int64_t ldx, int64_t nrhs, void *stream) {
  API_BEGIN
  visit(h, [&](auto &E) {
    if (auto *F = nsp_engine(&E, op)) F->nsp_filter_dev(E.dev(dX), ldx, nrhs, (hipStream_t)stream);
  });
  API_END
}

HifAmdStatus hifamd_nsp_find(HifAmdHdl h, HifAmdOp op, int64_t kmax, double tol, double rtol, int restart, int maxit,
                             int64_t rank, const void *X0, int64_t ldx0, uint64_t seed, int install, int64_t *found, void *Q,
                             int64_t ldq, double *resid16, int *info4) {
  API_BEGIN
  if (op != HIFAMD_S && op != HIFAMD_SH) throw Error(HIFAMD_MISMATCHED_SIZES, "a null space belongs to HIFAMD_S (A) or HIFAMD_SH (A^H)");
  if (kmax < 1 || kmax > HIFAMD_NSP_MAX) throw Error(HIFAMD_MISMATCHED_SIZES, "kmax must be 1 to 16 (HIFAMD_NSP_MAX)");
  if (!(tol > 0.0) || !(rtol > 0.0)) throw Error(HIFAMD_MISMATCHED_SIZES, "need tol > 0 and rtol > 0");
  if (restart < 1 || maxit < 1) throw Error(HIFAMD_MISMATCHED_SIZES, "need restart >= 1 and maxit >= 1");
  if (X0 && ldx0 < HIFAMD_NSP_MAX) throw Error(HIFAMD_MISMATCHED_SIZES, "probe block: row stride smaller than 16 (HIFAMD_NSP_MAX)");
  if (Q && ldq < kmax) throw Error(HIFAMD_MISMATCHED_SIZES, "basis output: row stride smaller than kmax");
  if (!found) throw Error(HIFAMD_MISMATCHED_SIZES, "found: NULL output");
  *found = 0;
  visit(h, [&](auto &E) {
    // (before for_op: asking for the adjoint engine of a handle that cannot serve the call would build it first)
    if (!E.finalized) throw Error(HIFAMD_BAD_PREC, "hierarchy not finalized (hifamd_finalize)");
    if (!E.has_A) throw Error(HIFAMD_BAD_PREC, "the null-space search needs the matrix (hifamd_set_matrix)");
    E.for_op(op).nsp_find(kmax, tol, rtol, restart, maxit, rank, E.val(X0), ldx0, seed, install != 0, found, E.val(Q), ldq,
                          resid16, info4);
  });
  API_END
}

int64_t hifamd_nsp_get_basis(HifAmdHdl h, HifAmdOp op, void *Q, int64_t ldq) {
  if (!h || !h->eng) return -1;
  try {
    return visit(h, [&](auto &E) -> int64_t {
      if (op == HIFAMD_S) return E.nsp_get_basis(E.val(Q), ldq);
      if (op == HIFAMD_SH) return E.adj ? E.adj->nsp_get_basis(E.val(Q), ldq) : 0;
      return 0;
    });
  } catch (const std::exception &e) {
    set_err(e.what());
    return -1;
  }
}

int hifamd_debug_checksums(HifAmdHdl h, uint64_t *out, int cap) {
  if (!h || !h->eng) return -1;
  return visit(h, [&](auto &E) { return E.debug_checksums(out, cap); });
}

HifAmdStatus hifamd_set_complex_operators(HifAmdHdl h, int flags) {
  API_BEGIN
  visit(h, [&](auto &E) { E.set_complex_operators(flags); });
  API_END
}

static const char kFileMagic[8] = {'H', 'I', 'F', 'A', 'M', 'D', '1', 0};

HifAmdStatus hifamd_save(HifAmdHdl h, const char *path) { return hifamd_save_ex(h, path, 0); }

HifAmdStatus hifamd_save_ex(HifAmdHdl h, const char *path, int flags) {
  API_BEGIN
  if (!path) throw Error(HIFAMD_NULL_OBJ, "NULL path");
  if (flags & ~HIFAMD_SAVE_ANALYSIS) throw Error(HIFAMD_BAD_PREC, "unknown hifamd_save_ex flag");
  std::FILE *f = std::fopen(path, "wb");
  if (!f) throw Error(HIFAMD_HIFIR_ERROR, std::string("cannot open for writing: ") + path);
  try {
    const int64_t vt = h->vt;
    if (std::fwrite(kFileMagic, 8, 1, f) != 1 || std::fwrite(&vt, 8, 1, f) != 1) throw Error(HIFAMD_HIFIR_ERROR, "short write");
    visit(h, [&](auto &E) { E.save(f, flags); });
  } catch (...) {
    std::fclose(f);
    throw;
  }
  if (std::fclose(f) != 0) throw Error(HIFAMD_HIFIR_ERROR, "write failed");
  API_END
}

HifAmdStatus hifamd_load(const char *path, int device, HifAmdHdl *out) { return hifamd_load_ex(path, device, 0, out); }

HifAmdStatus hifamd_load_ex(const char *path, int device, int complex_operators, HifAmdHdl *out) {
  if (!out || !path) {
    set_err("NULL argument");
    return HIFAMD_NULL_OBJ;
  }
  *out = nullptr;
  std::FILE *f = std::fopen(path, "rb");
  if (!f) {
    set_err(std::string("cannot open hierarchy file: ") + path);
    return HIFAMD_HIFIR_ERROR;
  }
  char magic[8];
  int64_t vt = -1;
  if (std::fread(magic, 8, 1, f) != 1 || std::memcmp(magic, kFileMagic, 8) != 0 || std::fread(&vt, 8, 1, f) != 1 ||
      (vt != HIFAMD_D && vt != HIFAMD_Z)) {
    std::fclose(f);
    set_err("not a hifir_amd hierarchy file");
    return HIFAMD_BAD_PREC;
  }
  HifAmdHdl h = nullptr;
  HifAmdStatus st = hifamd_create((HifAmdValueType)vt, device, &h);
  if (st != HIFAMD_SUCCESS) {
    std::fclose(f);
    return st;
  }
  if (complex_operators != 0) {  // (a planner choice, not data: between create and the replayed add_level calls)
    st = hifamd_set_complex_operators(h, complex_operators);
    if (st != HIFAMD_SUCCESS) {
      std::fclose(f);
      hifamd_destroy(h);
      return st;
    }
  }
  try {
    visit(h, [&](auto &E) { E.load(f); });
  } catch (const Error &e) {
    std::fclose(f);
    hifamd_destroy(h);
    set_err(e.what());
    return (HifAmdStatus)e.code;
  } catch (const std::exception &e) {
    std::fclose(f);
    hifamd_destroy(h);
    set_err(e.what());
    return HIFAMD_HIFIR_ERROR;
  }
  std::fclose(f);
  *out = h;
  return HIFAMD_SUCCESS;
}

HifAmdStatus hifamd_set_dense(HifAmdHdl h, int64_t nd, const void *mat, double rrqr_cond) {
  API_BEGIN
  visit(h, [&](auto &E) { E.set_dense(nd, E.val(mat), rrqr_cond); });
  API_END
}

HifAmdStatus hifamd_set_dense_symm(HifAmdHdl h, int64_t nd, const void *mat, int spd) {
  API_BEGIN
  visit(h, [&](auto &E) { E.set_dense_symm(nd, E.val(mat), spd); });
  API_END
}

HifAmdStatus hifamd_set_dense_lup(HifAmdHdl h, int64_t nd, const void *mat) {
  API_BEGIN
  visit(h, [&](auto &E) { E.set_dense_lup(nd, E.val(mat)); });
  API_END
}

HifAmdStatus hifamd_finalize(HifAmdHdl h, int64_t max_nrhs) {
  API_BEGIN
  visit(h, [&](auto &E) { E.finalize(max_nrhs); });
  API_END
}

int hifamd_value_type(HifAmdHdl h) { return (h && h->eng) ? h->vt : -1; }
int hifamd_device(HifAmdHdl h) {
  if (!h || !h->eng) return -1;
  return visit(h, [](auto &E) { return E.device; });
}
int64_t hifamd_nrows(HifAmdHdl h) {
  if (!h || !h->eng) return 0;
  return visit(h, [](auto &E) { return q_nrows(&E); });
}
int64_t hifamd_levels(HifAmdHdl h) {
  if (!h || !h->eng) return 0;
  return visit(h, [](auto &E) { return q_levels(&E); });
}
int64_t hifamd_nnz(HifAmdHdl h) {
  if (!h || !h->eng) return 0;
  return visit(h, [](auto &E) { return E.nnz_total(); });
}
int64_t hifamd_schur_size(HifAmdHdl h) {
  if (!h || !h->eng) return 0;
  return visit(h, [](auto &E) { return q_schur_size(&E); });
}
int64_t hifamd_schur_rank(HifAmdHdl h) {
  if (!h || !h->eng) return 0;
  return visit(h, [](auto &E) { return q_schur_rank(&E); });
}

int hifamd_launch_map(HifAmdHdl h, int32_t *out, int cap) {
  if (!h || !h->eng || (cap > 0 && !out)) return -1;
  return visit(h, [&](auto &E) { return E.launch_map(out, cap); });
}
int hifamd_kernel_census(HifAmdHdl h, int32_t *out, int cap) {
  if (!h || !h->eng || (cap > 0 && !out)) return -1;
  return visit(h, [&](auto &E) { return E.finalized ? E.kernel_census(out, cap) : 0; });
}
const char *hifamd_kernel_family_name(int family) {
  return (family >= 0 && family < hifamd::KF_COUNT) ? hifamd::kFamilyNames[family] : nullptr;
}
int hifamd_level_stats(HifAmdHdl h, int level, double *out, int cap) {
  if (!h || !h->eng || (cap > 0 && !out)) return -1;
  return visit(h, [&](auto &E) { return E.level_stats(level, out, cap); });
}
int hifamd_stats_ext(HifAmdHdl h, double *out, int cap) {
  if (!h || !h->eng || (cap > 0 && !out)) return -1;
  return visit(h, [&](auto &E) { return E.stats_ext(out, cap); });
}

HifAmdStatus hifamd_stats(HifAmdHdl h, double *stats16) {
  API_BEGIN
  if (!stats16) throw Error(HIFAMD_NULL_OBJ, "NULL stats array");
  visit(h, [&](auto &E) { E.stats(stats16); });
  API_END
}


HifAmdStatus hifamd_level_schedule(HifAmdHdl h, int level, int which, int64_t *nwf, int32_t *order, int64_t *wf_ptr) {
  API_BEGIN
  visit(h, [&](auto &E) { do_schedule(&E, level, which, nwf, order, wf_ptr); });
  API_END
}

HifAmdStatus hifamd_solve(HifAmdHdl h, const void *b, void *x, int64_t rank) {
  API_BEGIN
  visit(h, [&](auto &E) { E.solve_host(E.val(b), 1, E.val(x), 1, 1, rank); });
  API_END
}

HifAmdStatus hifamd_solve_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs, int64_t rank) {
  API_BEGIN
  visit(h, [&](auto &E) { E.solve_host(E.val(B), ldb, E.val(X), ldx, nrhs, rank); });
  API_END
}

HifAmdStatus hifamd_solve_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs,
                                    int64_t rank, void *stream) {
  API_BEGIN
  visit(h, [&](auto &E) { E.solve_dev(E.dev(dB), ldb, E.dev(dX), ldx, nrhs, rank, (hipStream_t)stream); });
  API_END
}

HifAmdStatus hifamd_set_matrix(HifAmdHdl h, int64_t n, const int64_t *indptr, const int32_t *indices, const void *vals) {
  API_BEGIN
  visit(h, [&](auto &E) { E.set_matrix(n, indptr, indices, E.val(vals)); });
  API_END
}

HifAmdStatus hifamd_spmv_batch_dev(HifAmdHdl h, const void *dX, int64_t ldx, void *dY, int64_t ldy, int64_t nrhs,
                                   void *stream) {
  API_BEGIN
  visit(h, [&](auto &E) { E.spmv_dev(E.dev(dX), ldx, E.dev(dY), ldy, nrhs, (hipStream_t)stream); });
  API_END
}

HifAmdStatus hifamd_hifir_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs, int nirs,
                                const double *betas, int64_t rank, int *ir_status) {
  API_BEGIN
  visit(h, [&](auto &E) { E.hifir_host(E.val(B), ldb, E.val(X), ldx, nrhs, nirs, betas, rank, ir_status); });
  API_END
}

HifAmdStatus hifamd_hifir_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs,
                                    int nirs, const double *betas, int64_t rank, int *ir_status) {
  API_BEGIN
  visit(h, [&](auto &E) { E.hifir_dev(E.dev(dB), ldb, E.dev(dX), ldx, nrhs, nirs, betas, rank, ir_status); });
  API_END
}


HifAmdStatus hifamd_apply_batch(HifAmdHdl h, HifAmdOp op, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs,
                                int nirs, const double *betas, int64_t rank, int *ir_status) {
  API_BEGIN
  const bool prod = (op == HIFAMD_M || op == HIFAMD_MH);
  if (rank == -2) rank = (prod || nirs > 1) ? -1 : 0;  // LHF_DEFAULT_RANK, libhifir.cpp:453-455
  if (prod) {
    visit(h, [&](auto &E) { E.for_op(op).prod_host(E.val(B), ldb, E.val(X), ldx, nrhs, rank); });
    if (ir_status)
      for (int64_t c = 0; c < nrhs; ++c) ir_status[2 * c] = 1, ir_status[2 * c + 1] = -1;
  } else {
    visit(h, [&](auto &E) { E.for_op(op).hifir_host(E.val(B), ldb, E.val(X), ldx, nrhs, nirs, betas, rank, ir_status); });
  }
  API_END
}

HifAmdStatus hifamd_apply_batch_dev(HifAmdHdl h, HifAmdOp op, const void *dB, int64_t ldb, void *dX, int64_t ldx,
                                    int64_t nrhs, int64_t rank, void *stream) {
  API_BEGIN
  const int kind = (op == HIFAMD_M || op == HIFAMD_MH) ? 1 : 0;
  if (rank == -2) rank = kind ? -1 : 0;
  visit(h, [&](auto &E) { E.for_op(op).solve_dev(E.dev(dB), ldb, E.dev(dX), ldx, nrhs, rank, (hipStream_t)stream, kind); });
  API_END
}

HifAmdStatus hifamd_gmres_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs, int restart,
                                double rtol, int maxit, int64_t rank, int *flags, int *iters) {
  API_BEGIN
  visit(h, [&](auto &E) { E.gmres_host(E.val(B), ldb, E.val(X), ldx, nrhs, restart, rtol, maxit, rank, flags, iters); });
  API_END
}

HifAmdStatus hifamd_gmres_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs,
                                    int restart, double rtol, int maxit, int64_t rank, int *flags, int *iters) {
  API_BEGIN
  visit(h, [&](auto &E) { E.gmres_dev(E.dev(dB), ldb, E.dev(dX), ldx, nrhs, restart, rtol, maxit, rank, flags, iters); });
  API_END
}

HifAmdStatus hifamd_set_residual_precision(HifAmdHdl h, int mode) {
  API_BEGIN
  if (mode != HIFAMD_RESID_WORKING && mode != HIFAMD_RESID_COMPENSATED)
    throw Error(HIFAMD_MISMATCHED_SIZES, "residual precision: HIFAMD_RESID_WORKING or HIFAMD_RESID_COMPENSATED");
  visit(h, [&](auto &E) { E.set_resid_mode(mode); });
  API_END
}

int hifamd_residual_precision(HifAmdHdl h) {
  if (!h || !h->eng) return -1;
  return visit(h, [](auto &E) { return E.opt.resid_mode; });
}

HifAmdStatus hifamd_residual_batch(HifAmdHdl h, HifAmdOp op, const void *B, int64_t ldb, const void *X, int64_t ldx, void *R,
                                   int64_t ldr, int64_t nrhs, int mode) {
  API_BEGIN
  visit(h, [&](auto &E) {
    residual_pre(&E, op, mode);
    E.for_op(op).residual_host(E.val(B), ldb, E.val(X), ldx, E.val(R), ldr, nrhs, mode);
  });
  API_END
}

HifAmdStatus hifamd_residual_batch_dev(HifAmdHdl h, HifAmdOp op, const void *dB, int64_t ldb, const void *dX, int64_t ldx,
                                       void *dR, int64_t ldr, int64_t nrhs, int mode, void *stream) {
  API_BEGIN
  visit(h, [&](auto &E) {
    residual_pre(&E, op, mode);
    E.for_op(op).residual_dev(E.dev(dB), ldb, E.dev(dX), ldx, E.dev(dR), ldr, nrhs, mode, (hipStream_t)stream);
  });
  API_END
}

HifAmdStatus hifamd_gmres_ir_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs, int restart,
                                   double rtol, double inner_rtol, int max_outer, int inner_maxit, int64_t rank, int *flags,
                                   int *outer, int *iters, double *relres) {
  API_BEGIN
  visit(h, [&](auto &E) {
    E.gmres_ir_host(E.val(B), ldb, E.val(X), ldx, nrhs, restart, rtol, inner_rtol, max_outer, inner_maxit, rank, flags, outer, iters,
                    relres);
  });
  API_END
}

HifAmdStatus hifamd_gmres_ir_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs,
                                       int restart, double rtol, double inner_rtol, int max_outer, int inner_maxit,
                                       int64_t rank, int *flags, int *outer, int *iters, double *relres) {
  API_BEGIN
  visit(h, [&](auto &E) {
    E.gmres_ir_dev(E.dev(dB), ldb, E.dev(dX), ldx, nrhs, restart, rtol, inner_rtol, max_outer, inner_maxit, rank, flags, outer, iters,
                   relres);
  });
  API_END
}

HifAmdStatus hifamd_fgmres_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs, int restart,
                                 double rtol, int maxit, int64_t rank, int *flags, int *iters, int *sweeps) {
  API_BEGIN
  visit(h, [&](auto &E) { E.gmres_host(E.val(B), ldb, E.val(X), ldx, nrhs, restart, rtol, maxit, rank, flags, iters, true, sweeps); });
  API_END
}

HifAmdStatus hifamd_bcg_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs, int block,
                              double rtol, double deftol, int maxit, int64_t rank, int *flags, int *iters, int *ranks) {
  API_BEGIN
  visit(h, [&](auto &E) { E.bcg_host(E.val(B), ldb, E.val(X), ldx, nrhs, block, rtol, deftol, maxit, rank, flags, iters, ranks); });
  API_END
}

HifAmdStatus hifamd_bcg_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs, int block,
                                  double rtol, double deftol, int maxit, int64_t rank, int *flags, int *iters, int *ranks) {
  API_BEGIN
  visit(h, [&](auto &E) { E.bcg_dev(E.dev(dB), ldb, E.dev(dX), ldx, nrhs, block, rtol, deftol, maxit, rank, flags, iters, ranks); });
  API_END
}

HifAmdStatus hifamd_bgcr_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs, int block,
                               int restart, double rtol, double deftol, int maxit, int64_t rank, int *flags, int *iters,
                               int *ranks) {
  API_BEGIN
  visit(h, [&](auto &E) {
    E.bgcr_host(E.val(B), ldb, E.val(X), ldx, nrhs, block, restart, rtol, deftol, maxit, rank, flags, iters, ranks);
  });
  API_END
}

HifAmdStatus hifamd_bgcr_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs, int block,
                                   int restart, double rtol, double deftol, int maxit, int64_t rank, int *flags, int *iters,
                                   int *ranks) {
  API_BEGIN
  visit(h, [&](auto &E) {
    E.bgcr_dev(E.dev(dB), ldb, E.dev(dX), ldx, nrhs, block, restart, rtol, deftol, maxit, rank, flags, iters, ranks);
  });
  API_END
}

HifAmdStatus hifamd_lobpcg(HifAmdHdl h, int64_t k, int64_t nev, const void *X0, int64_t ldx0, uint64_t seed, double tol,
                           double deftol, int maxit, int64_t rank, double *lambda, void *X, int64_t ldx, double *res, int *flags,
                           int *info3) {
  API_BEGIN
  visit(h, [&](auto &E) {
    E.lobpcg_host(false, k, nev, E.val(X0), ldx0, seed, tol, deftol, maxit, rank, lambda, E.val(X), ldx, res, flags, info3);
  });
  API_END
}

HifAmdStatus hifamd_lobpcg_dev(HifAmdHdl h, int64_t k, int64_t nev, const void *dX0, int64_t ldx0, uint64_t seed, double tol,
                               double deftol, int maxit, int64_t rank, double *lambda, void *dX, int64_t ldx, double *res,
                               int *flags, int *info3) {
  API_BEGIN
  visit(h, [&](auto &E) {
    E.lobpcg_dev(false, k, nev, E.dev(dX0), ldx0, seed, tol, deftol, maxit, rank, lambda, E.dev(dX), ldx, res, flags, info3);
  });
  API_END
}

HifAmdStatus hifamd_eig_project(HifAmdHdl h, int gen, int64_t m, const void *Y, int64_t ldy, int64_t kw, void *W, int64_t ldw) {
  API_BEGIN
  visit(h, [&](auto &E) { E.eig_project_host(gen != 0, m, E.val(Y), ldy, kw, E.val(W), ldw); });
  API_END
}

HifAmdStatus hifamd_eig_project_dev(HifAmdHdl h, int gen, int64_t m, const void *dY, int64_t ldy, int64_t kw, void *dW, int64_t ldw) {
  API_BEGIN
  visit(h, [&](auto &E) { E.eig_project_dev(gen != 0, m, E.dev(dY), ldy, kw, E.dev(dW), ldw); });
  API_END
}

HifAmdStatus hifamd_eigs(HifAmdHdl h, int gen, int64_t nev, int64_t k, int64_t guard, const void *Y, int64_t ldy, int64_t m0,
                         const void *X0, int64_t ldx0, uint64_t seed, double tol, double deftol, int maxit, int64_t rank,
                         double *lambda, void *X, int64_t ldx, double *res, int *flags, int *info4) {
  API_BEGIN
  visit(h, [&](auto &E) {
    E.eigs_host(gen != 0, nev, k, guard, E.val(Y), ldy, m0, E.val(X0), ldx0, seed, tol, deftol, maxit, rank, lambda, E.val(X), ldx, res,
                flags, info4);
  });
  API_END
}

HifAmdStatus hifamd_eigs_dev(HifAmdHdl h, int gen, int64_t nev, int64_t k, int64_t guard, const void *dY, int64_t ldy, int64_t m0,
                             const void *dX0, int64_t ldx0, uint64_t seed, double tol, double deftol, int maxit, int64_t rank,
                             double *lambda, void *dX, int64_t ldx, double *res, int *flags, int *info4) {
  API_BEGIN
  visit(h, [&](auto &E) {
    E.eigs_dev(gen != 0, nev, k, guard, E.dev(dY), ldy, m0, E.dev(dX0), ldx0, seed, tol, deftol, maxit, rank, lambda, E.dev(dX), ldx,
               res, flags, info4);
  });
  API_END
}

int hifamd_eigs_sweeps(HifAmdHdl h, int *out, int cap) {
  if (!h || !h->eng) return -1;
  return visit(h, [&](auto &E) { return E.eigs_sweeps(out, cap); });
}

HifAmdStatus hifamd_set_mass_matrix(HifAmdHdl h, int64_t n, const int64_t *indptr, const int32_t *indices, const void *vals) {
  API_BEGIN
  visit(h, [&](auto &E) { E.set_mass_matrix(n, indptr, indices, E.val(vals)); });
  API_END
}

HifAmdStatus hifamd_lobpcg_gen(HifAmdHdl h, int64_t k, int64_t nev, const void *X0, int64_t ldx0, uint64_t seed, double tol,
                               double deftol, int maxit, int64_t rank, double *lambda, void *X, int64_t ldx, double *res,
                               int *flags, int *info3) {
  API_BEGIN
  visit(h, [&](auto &E) {
    E.lobpcg_host(true, k, nev, E.val(X0), ldx0, seed, tol, deftol, maxit, rank, lambda, E.val(X), ldx, res, flags, info3);
  });
  API_END
}

HifAmdStatus hifamd_lobpcg_gen_dev(HifAmdHdl h, int64_t k, int64_t nev, const void *dX0, int64_t ldx0, uint64_t seed, double tol,
                                   double deftol, int maxit, int64_t rank, double *lambda, void *dX, int64_t ldx, double *res,
                                   int *flags, int *info3) {
  API_BEGIN
  visit(h, [&](auto &E) {
    E.lobpcg_dev(true, k, nev, E.dev(dX0), ldx0, seed, tol, deftol, maxit, rank, lambda, E.dev(dX), ldx, res, flags, info3);
  });
  API_END
}

HifAmdStatus hifamd_pcg_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs, double rtol,
                              int maxit, int64_t rank, int *flags, int *iters) {
  API_BEGIN
  visit(h, [&](auto &E) { E.pcg_host(E.val(B), ldb, E.val(X), ldx, nrhs, rtol, maxit, rank, flags, iters); });
  API_END
}

HifAmdStatus hifamd_pcg_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs,
                                  double rtol, int maxit, int64_t rank, int *flags, int *iters) {
  API_BEGIN
  visit(h, [&](auto &E) { E.pcg_dev(E.dev(dB), ldb, E.dev(dX), ldx, nrhs, rtol, maxit, rank, flags, iters); });
  API_END
}

HifAmdStatus hifamd_bicgstab_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs,
                                   double rtol, int maxit, int64_t rank, int *flags, int *iters) {
  API_BEGIN
  visit(h, [&](auto &E) { E.bicgstab_host(E.val(B), ldb, E.val(X), ldx, nrhs, rtol, maxit, rank, flags, iters); });
  API_END
}

HifAmdStatus hifamd_bicgstab_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs,
                                       double rtol, int maxit, int64_t rank, int *flags, int *iters) {
  API_BEGIN
  visit(h, [&](auto &E) { E.bicgstab_dev(E.dev(dB), ldb, E.dev(dX), ldx, nrhs, rtol, maxit, rank, flags, iters); });
  API_END
}

HifAmdStatus hifamd_idrs_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs, int s,
                               const void *P, int64_t ldp, uint64_t seed, double rtol, int maxit, int64_t rank, int *flags,
                               int *iters) {
  API_BEGIN
  visit(h, [&](auto &E) { E.idrs_host(E.val(B), ldb, E.val(X), ldx, nrhs, s, E.val(P), ldp, seed, rtol, maxit, rank, flags, iters); });
  API_END
}

HifAmdStatus hifamd_idrs_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs, int s,
                                   const void *P, int64_t ldp, uint64_t seed, double rtol, int maxit, int64_t rank,
                                   int *flags, int *iters) {
  API_BEGIN
  // (the shadow block P is a host array on both entries)
  visit(h, [&](auto &E) { E.idrs_dev(E.dev(dB), ldb, E.dev(dX), ldx, nrhs, s, E.val(P), ldp, seed, rtol, maxit, rank, flags, iters); });
  API_END
}

HifAmdStatus hifamd_sqmr_batch(HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs, double rtol,
                               int maxit, int64_t rank, int *flags, int *iters) {
  API_BEGIN
  visit(h, [&](auto &E) { E.sqmr_host(E.val(B), ldb, E.val(X), ldx, nrhs, rtol, maxit, rank, flags, iters); });
  API_END
}

HifAmdStatus hifamd_sqmr_batch_dev(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs,
                                   double rtol, int maxit, int64_t rank, int *flags, int *iters) {
  API_BEGIN
  visit(h, [&](auto &E) { E.sqmr_dev(E.dev(dB), ldb, E.dev(dX), ldx, nrhs, rtol, maxit, rank, flags, iters); });
  API_END
}

int hifamd_hermitian(HifAmdHdl h) {
  if (!h || !h->eng) return -1;
  try {
    const HermCheck &hc = visit(h, [](auto &E) -> const HermCheck & { return E.hermitian(); });
    if (hc.ok) return 1;
    set_err("level " + std::to_string(hc.level) + ": " + hc.what);
    return 0;
  } catch (const std::exception &e) {  // (allocation failure of the O(nnz) pass)
    set_err(e.what());
    return -1;
  }
}

HifAmdStatus hifamd_time_apply(HifAmdHdl h, const void *dB, int64_t ldb, void *dX, int64_t ldx, int64_t nrhs,
                               int64_t rank, int warmup, int reps, double *ms_avg) {
  API_BEGIN
  visit(h, [&](auto &E) { do_time(&E, E.dev(dB), ldb, E.dev(dX), ldx, nrhs, rank, warmup, reps, ms_avg); });
  API_END
}


HifAmdStatus hifamd_sync(HifAmdHdl h) {
  API_BEGIN
  visit(h, [&](auto &E) { do_sync(&E); });
  API_END
}

HifAmdStatus hifamd_copy_columns_dev(HifAmdHdl h, const void *src, int64_t lds, int64_t ncols, void *dst, int64_t ldd,
                                     int64_t col0) {
  API_BEGIN
  visit(h, [&](auto &E) { do_copy_columns(&E, src, lds, ncols, dst, ldd, col0); });
  API_END
}

}  // extern "C"
