// options.hpp -- what a handle reads from the environment when it is created: one struct (EngineOptions), one table with
// a row per variable (kOptionRows), one reader (EngineOptions::from_env).  The handle's engine is built from the struct,
// and so are the adjoint engine and the twin lanes it builds on first use: they never look at the environment.
//
// Pure C++17, no HIP: engine.hip uses it for the product, tests/cpp/options_test.cpp compiles the same code with g++.
//
// Every variable the library reads is in the table below, except
//   * the residual mode a handle starts with, read by import.hpp's resid_mode_from_env (from_env calls it);
//   * HIFIR_AMD_THREADS (host.hpp, import.hpp: host threads of the analysis, read where the threads are started);
//   * HIFIR_AMD_PLAN_DUMP, HIFIR_AMD_FINALIZE_DUMP, HIFIR_AMD_PROBE_OUT, HIFIR_AMD_CSPROBE_OUT (diagnostics) and
//     HIFIR_AMD_LOAD_ANALYSIS (read inside load()): they select output and a cache, not an engine, and engine.hip reads
//     them where and when they take effect.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "host.hpp"
#include "import.hpp"

namespace hifamd {

inline int env_int(const char *name, int dflt) {
  const char *v = std::getenv(name);
  return v ? std::atoi(v) : dflt;
}

constexpr int64_t kMaxWgRows = 16384;  // BandOptions::max_wg_rows: LDS flags per workgroup (kernels.hip.hpp HIFAMD_TAIL_MAX)

// The defaults are those of the table; from_env sets every member but the BandOptions members no variable reaches.
struct EngineOptions {
  int use_twin;   // number of EXTRA lanes (HIFIR_AMD_TWIN: 0 = tiles strictly one after the other)
  // HIFIR_AMD_LIST_EARLY=1 (round 4, measured, OFF): 3.66 -> 3.77 ms on the 1M default hierarchy -- the five fork / join pairs of
  // the captured graph cost more than the 0.12 ms of list kernels they hide
  int list_early;
  bool use_graph;
  int min_logR;
  int gemm_waves;   // split-K width of the block-inverse GEMM
  bool spmm_tiles;       // E / F products on the matrix cores where rows share columns (HIFIR_AMD_SPMM_TILES=0: off)
  bool fuse_gather;  // S1 fused into the L solve (HIFIR_AMD_FUSE_S1=0: separate k_gather_scale launches)
  // The hierarchy's tail as ONE dense operator: from the first level of at most tail_rows rows downwards (the small
  // levels and the dense block behind them are a chain of ~15 dependent launches per solve for a few thousand rows),
  // G = M_tail^{-1}, formed at finalize by running the device's own apply on the identity, one product per solve.
  // Only where the effective rank of the dense block equals its numerical rank (the operator bakes that rank in; the graph
  // cache keys on the effective rank too).  HIFIR_AMD_TAIL_ROWS=0: off.
  int64_t tail_rows;
  double tail_probe_tol, tail_max_growth;  // HIFIR_AMD_TAIL_PROBE_TOL / HIFIR_AMD_TAIL_GROWTH
  bool fuse_out;    // S7 fused into the last band of the final U solve (HIFIR_AMD_FUSE_S7=0: k_scatter_scale over all rows)
  int spmm_tiles_z;     // HIFIR_AMD_SPMM_TILES_Z=0: complex coupling blocks keep the row-gather products
  int spmm_rb;          // HIFIR_AMD_SPMM_RB: 16-row tiles per block of the tiled Schur products (1; 2 measured slower: fewer, longer chains)
  int spmm_split_blocks;  // HIFIR_AMD_SPMM_SPLIT_BLOCKS: fewer blocks than this -> one block per workgroup (k_spmm_tile4)
  bool spmm_split;  // tiled Schur products: one 16-row block per workgroup (k_spmm_tile4); HIFIR_AMD_SPMM_SPLIT=0: per wave
  int carry_wgs;   // workgroups a band's launch may add for the carried prefix of the next band (HIFIR_AMD_CARRY_WGS)
  bool fuse_f;    // S5 fused into the second L solve where the plan allows (HIFIR_AMD_FUSE_F=0: separate k_spmm_epi launch)
  int top_gemm;      // top / tail operator product: 4 k_top_gemm (64-row tiles, panel through LDS, K splits); 1 k_strip_gemm_d<4>,
                     // 2 k_strip_gemm4_d<2>, 3 k_strip_gemm4_d<4> (HIFIR_AMD_TOP_GEMM)
  // HIFIR_AMD_TOP_LAST=1 (round 4, measured, OFF): the K splits summed inside k_top_gemm by the last split to arrive -- nine
  // launches fewer, same bits, but the agent-scope release / acquire fences write back and invalidate a whole L2 per
  // workgroup: k_top_gemm 40 -> 147 us, the apply 3.67 -> 4.61 ms
  int top_last_arriver;
  // Complex handles have both operators on request only (hifamd_set_complex_operators, before the first level): bit 0 the
  // tail operator, bit 1 the combined tops.  Their products run through k_top_gemm_z / k_top_reduce_z whatever the
  // switches of the real product kernels say.  Real handles: always 0 (they have both operators anyway).
  int zop_flags = 0;
  int64_t zop_top_max;  // what top_max is for a real handle in the environment this handle was created under
  int cd_dbg;        // development aid (HIFIR_AMD_CD_DBG): phases of k_band_cd switched off for timing experiments
  // Column-sliced component bands (kernels.hip.hpp k_band_cs): a component band of at most cs_max_wgs workgroups is cut
  // into 16-column slices (the heaviest component of a narrow band then runs on four compute units); a batch of fewer
  // than 49 columns runs EVERY component band sliced and launches only the slices it has.  HIFIR_AMD_CS=0: off.
  int cs_mode;
  // Two launches for a component band whose slowest wave would walk many entries: the entries of ALL its rows that refer
  // to rows outside their component go to a chip-wide prefix pass (every wave of the chip takes rows, perfectly balanced),
  // and the band kernel is left with right-hand sides -> inverse product -> stores.  One launch more (~ 8 us) against the
  // serial walk of the band's longest chunk at ~ 120 ns per entry.  HIFIR_AMD_CD_SPLIT_MIN: entries of the
  // longest chunk from which a band is split (0 = never); HIFIR_AMD_CD_SPLIT_WGS: only bands of at most this many components
  int cd_split_min, cd_split_wgs;
  int narrow_spmm;   // HIFIR_AMD_NARROW_SPMM=0: batches of <= 32 columns keep the 64-lane Schur product kernel
  int cs_sparse;     // HIFIR_AMD_CS_SPARSE=1: sparse-own bands (level 0) in column slices at full width too
  int device_inverses;  // HIFIR_AMD_DEVICE_INVERSES=0: the block inverses of finalize are formed by the host threads and uploaded
  int cs_max_wgs;    // HIFIR_AMD_CS_MAX_WGS (full batches: measured equal to k_band_cd at every band width)
  int ct_wide_wgs; // HIFIR_AMD_CT_WIDE: a component band with more workgroups than this takes two column tiles per workgroup
  int ct_wide4_wgs;  // HIFIR_AMD_CT_WIDE4: ... and with more than this all four (one workgroup per component)
  int us_mode;  // HIFIR_AMD_US=0: sparse-own U bands keep every row of a component in LDS (k_band_cd)
  int ls_mode;  // HIFIR_AMD_LS=0: sparse-own L bands keep every row of a component in LDS (k_band_cd; the same bits)
  int ls_chunk;  // HIFIR_AMD_LS_CHUNK=32/48/64: rows of k_band_ls's source chunk (0: the largest that fits 80 KB of LDS)
  int narrow_tiles;  // HIFIR_AMD_NARROW_TILES=0: the tiled Schur products always multiply all four column tiles
  int skip_rows;  // HIFIR_AMD_SKIP_ROWS: bit 0 L rows / bit 1 U rows a level's first solve does not store (build_row_flags); 0: every row
  int ct_mode_real;  // HIFIR_AMD_CT_REAL=0: real handles keep the entry walk while HIFIR_AMD_CT_Z stays as set (tests)
  int ct_mode_z;     // HIFIR_AMD_CT_Z=1: complex component bands on coefficient tiles too (k_band_ct_z; measured SLOWER than the
                     // entry walk at every width on BASELINE config 5: 7.17 vs 7.00 ms at 16, 17.9 vs 16.1 ms at 64 columns)
  int ct_mode;       // HIFIR_AMD_CT=0: dense-own component bands walk their entries one by one (k_band_cd / k_band_cs) instead of
                     // multiplying 16 x 4 coefficient tiles on the matrix cores (k_band_ct)
  int xcd_remap;     // HIFIR_AMD_XCD=0: workgroups numbered as the hardware deals them (one device-wide word, set by the last finalize)
  int band_pipe;     // 1: k_trsv_band_p (next row's head behind the last gathers), 0: k_trsv_band at R = 64 too
  BandOptions band;  // how triangles are cut into bands (host.hpp)
  // how resid_dev forms r = b - A x: 0 working precision (k_crs_spmm), 1 compensated (k_crs_resid_dd); from the
  // environment at creation (import.hpp resid_mode_from_env), hifamd_set_residual_precision later
  int resid_mode;

  static EngineOptions from_env(bool is_complex);
};

// One variable: its name, its default for real and for complex handles, and where its value goes.  A variable that only
// one kind of handle reads has an empty `set` for the other kind.  The two floating-point rows carry their member and
// default in `fp` / `fp_dflt` and are parsed with atof; every other row is parsed with atoi.
struct OptionRow {
  const char *name;
  int dflt, dflt_z;
  void (*set)(EngineOptions &o, int v, bool is_complex);
  double EngineOptions::*fp;
  double fp_dflt;
};

#define HIFAMD_ROW(name, dflt, member, value) \
  {name, dflt, dflt, [](EngineOptions &o, int v, bool) { o.member = (value); }, nullptr, 0.0}
// ... read by real handles / by complex handles only
#define HIFAMD_ROW_D(name, dflt, member, value) \
  {name, dflt, dflt, [](EngineOptions &o, int v, bool z) { if (!z) o.member = (value); }, nullptr, 0.0}
#define HIFAMD_ROW_Z(name, dflt, member, value) \
  {name, dflt, dflt, [](EngineOptions &o, int v, bool z) { if (z) o.member = (value); }, nullptr, 0.0}
#define HIFAMD_ROW_FP(name, dflt, member) {name, 0, 0, nullptr, &EngineOptions::member, dflt}

static const OptionRow kOptionRows[] = {
    HIFAMD_ROW("HIFIR_AMD_NO_GRAPH", 0, use_graph, v == 0),
    HIFAMD_ROW("HIFIR_AMD_MIN_LOGR", 6, min_logR, std::min(6, std::max(0, v))),
    HIFAMD_ROW("HIFIR_AMD_GEMM_WAVES", 16, gemm_waves, v),
    HIFAMD_ROW("HIFIR_AMD_BAND_PIPE", 1, band_pipe, v),
    HIFAMD_ROW("HIFIR_AMD_CD_DBG", 0, cd_dbg, v),
    HIFAMD_ROW("HIFIR_AMD_CS", 1, cs_mode, v),
    HIFAMD_ROW("HIFIR_AMD_CS_MAX_WGS", 0, cs_max_wgs, v),
    HIFAMD_ROW("HIFIR_AMD_CT", 1, ct_mode, v),
    HIFAMD_ROW("HIFIR_AMD_CT_Z", 0, ct_mode_z, v),
    HIFAMD_ROW("HIFIR_AMD_CT_REAL", 1, ct_mode_real, v),
    HIFAMD_ROW("HIFIR_AMD_SKIP_ROWS", 3, skip_rows, v),
    HIFAMD_ROW("HIFIR_AMD_NARROW_TILES", 1, narrow_tiles, v),
    HIFAMD_ROW("HIFIR_AMD_US", 1, us_mode, v),
    HIFAMD_ROW("HIFIR_AMD_LS", 1, ls_mode, v),
    HIFAMD_ROW("HIFIR_AMD_LS_CHUNK", 0, ls_chunk, v),
    HIFAMD_ROW("HIFIR_AMD_TOP_LAST", 0, top_last_arriver, v),
    HIFAMD_ROW("HIFIR_AMD_LIST_EARLY", 0, list_early, v),
    HIFAMD_ROW("HIFIR_AMD_SPMM_RB", 1, spmm_rb, v == 2 ? 2 : 1),
    HIFAMD_ROW("HIFIR_AMD_SPMM_TILES_Z", 1, spmm_tiles_z, v),
    HIFAMD_ROW("HIFIR_AMD_SPMM_SPLIT_BLOCKS", 4096, spmm_split_blocks, v),
    HIFAMD_ROW("HIFIR_AMD_CT_WIDE", 128, ct_wide_wgs, v),
    HIFAMD_ROW("HIFIR_AMD_CT_WIDE4", 1 << 30, ct_wide4_wgs, v),
    HIFAMD_ROW("HIFIR_AMD_CS_SPARSE", 0, cs_sparse, v),
    HIFAMD_ROW("HIFIR_AMD_DEVICE_INVERSES", 1, device_inverses, v),
    HIFAMD_ROW("HIFIR_AMD_NARROW_SPMM", 1, narrow_spmm, v),
    HIFAMD_ROW("HIFIR_AMD_CD_SPLIT_MIN", 0, cd_split_min, v),
    HIFAMD_ROW("HIFIR_AMD_CD_SPLIT_WGS", 600, cd_split_wgs, v),
    HIFAMD_ROW("HIFIR_AMD_TOP_GEMM", 4, top_gemm, v),
    HIFAMD_ROW("HIFIR_AMD_FUSE_F", 1, fuse_f, v != 0),
    HIFAMD_ROW("HIFIR_AMD_CARRY_WGS", 512, carry_wgs, std::max(1, v)),
    HIFAMD_ROW("HIFIR_AMD_SPMM_SPLIT", 1, spmm_split, v != 0),
    HIFAMD_ROW("HIFIR_AMD_FUSE_S7", 1, fuse_out, v != 0),
    HIFAMD_ROW("HIFIR_AMD_TAIL_ROWS", 4096, tail_rows, v),
    HIFAMD_ROW_FP("HIFIR_AMD_TAIL_PROBE_TOL", 1e-11, tail_probe_tol),
    HIFAMD_ROW_FP("HIFIR_AMD_TAIL_GROWTH", 1e8, tail_max_growth),
    HIFAMD_ROW("HIFIR_AMD_FUSE_S1", 1, fuse_gather, v != 0),
    HIFAMD_ROW("HIFIR_AMD_SPMM_TILES", 1, spmm_tiles, v != 0),
    HIFAMD_ROW("HIFIR_AMD_TWIN", 1, use_twin, v),
    HIFAMD_ROW("HIFIR_AMD_XCD", 1, xcd_remap, v),
    HIFAMD_ROW("HIFIR_AMD_THIN_ROWS", 96, band.thin_rows, v),
    HIFAMD_ROW("HIFIR_AMD_BAND_DEPTH", 32, band.band_depth, v),
    HIFAMD_ROW("HIFIR_AMD_BAND_WGS", 1024, band.max_wgs, v),
    HIFAMD_ROW("HIFIR_AMD_BAND_WEIGHT", 1024, band.max_comp_weight, v),
    HIFAMD_ROW("HIFIR_AMD_DENSE_BLOCK", 2048, band.dense_block, v),  // 0: exact sequential thin bands
    // carried prefixes (host.hpp finish_band_plan): real data only -- measured on the complex 1M-row case (one
    // workgroup per compute unit, rows of 1 KB) they lose at every threshold (18.8 ms without, 19.7 ... 20.6 ms with)
    {"HIFIR_AMD_BAND_FUSE", 1, 0, [](EngineOptions &o, int v, bool) { o.band.fuse = v != 0; }, nullptr, 0.0},
    HIFAMD_ROW("HIFIR_AMD_BAND_FUSE_WGS", 512, band.fuse_max_wgs, v),
    HIFAMD_ROW("HIFIR_AMD_CD_FUSE_WGS", 600, band.cd_fuse_max_wgs, v),  // (4.26 -> 4.18 ms: the 1,216-workgroup last U band of level 1 gathers its own old sources)
    // component-dense bands (host.hpp plan_bands_cd), fast mode only (from_env); HIFIR_AMD_CD_ROWS=0 keeps the depth-cut bands
    HIFAMD_ROW_D("HIFIR_AMD_CD_ROWS", 128, band.cd_rows, v),
    // complex handles: the same plan with 1 KB rows (k_band_cd_z keeps a component as two real planes: 96 rows = 96 KB)
    HIFAMD_ROW_Z("HIFIR_AMD_CD_ROWS_Z", 96, band.cd_rows, std::min(144, v)),
    HIFAMD_ROW_D("HIFIR_AMD_CD_NNZ", 4000, band.cd_max_nnz, v),  // (a band lasts as long as its heaviest component: 4.53 -> 4.44 ms)
    HIFAMD_ROW_Z("HIFIR_AMD_CD_NNZ_Z", 0, band.cd_max_nnz, v),
    HIFAMD_ROW_D("HIFIR_AMD_CD_SPARSE_ROWS", 192, band.cd_sparse_rows, std::min(240, v)),  // 0: thin triangles keep the flag bands
    // complex handles: sparse-own components for shallow thin triangles since round 4 (HIFIR_AMD_CD_SPARSE_ROWS_Z=0:
    // those triangles keep the round-1 flag bands)
    HIFAMD_ROW_Z("HIFIR_AMD_CD_SPARSE_ROWS_Z", 192, band.cd_sparse_rows, std::min(240, v)),
    HIFAMD_ROW("HIFIR_AMD_TOP_ROWS", 4096, band.top_max, v),  // combined top operator (host.hpp choose_top); 0 = off
    HIFAMD_ROW("HIFIR_AMD_TOP_WGS", 96, band.top_few_wgs, v),
    HIFAMD_ROW("HIFIR_AMD_CD_SPARSE_MIN_ROWS", 4096, band.cd_sparse_min_rows, v),
};
#undef HIFAMD_ROW
#undef HIFAMD_ROW_D
#undef HIFAMD_ROW_Z
#undef HIFAMD_ROW_FP

inline EngineOptions EngineOptions::from_env(bool is_complex) {
  EngineOptions o{};
  for (const OptionRow &r : kOptionRows) {
    const char *e = std::getenv(r.name);
    if (r.fp)
      o.*r.fp = e ? std::atof(e) : r.fp_dflt;
    else
      r.set(o, e ? std::atoi(e) : is_complex ? r.dflt_z : r.dflt, is_complex);
  }
  o.resid_mode = resid_mode_from_env();
  o.band.max_wg_rows = kMaxWgRows;
  o.band.fuse_reorder = o.band.dense_block > 0;  // exact mode keeps the reference's order
  if (o.band.dense_block <= 0) o.band.cd_rows = 0;
  // complex handles: no combined top unless the handle asks for it (set_complex_operators)
  o.zop_top_max = o.band.top_max;
  if (is_complex) o.band.top_max = 0;
  if (o.band.cd_rows > 240) o.band.cd_rows = 240;  // (local row ids are bytes; 120 KB of the CU's 160 KB LDS)
  return o;
}

}  // namespace hifamd
