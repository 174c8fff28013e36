// Dynamic-LDS layouts of the component-band kernels (kernels.hip.hpp), stated ONCE: a kernel takes every LDS pointer from
// its struct, the host (engine.hip, and the k_band_ls planner in host.hpp) every byte count.  Plain C++17, no HIP include:
// kernels.hip.hpp, host.hpp and host tests built with g++ (tests/cpp/band_lds_test.cpp) all read this file.
//
// Every member is the BYTE offset of one array from the start of the kernel's `extern __shared__` block (8-byte aligned),
// in the order the arrays lie in; bytes() is what the launch asks for.  A struct is built from the run-time sizes its
// kernel receives anyway.  The slack some layouts keep behind their last array is part of bytes(): k_band_us and k_band_ls
// are sized so that two workgroups share a compute unit, and the instances that need more than 64 KB get their limit raised
// from these numbers (engine.hip band_lds_table).  Offsets are int32: LDS addresses are 32 bits wide, and the sizes are
// bounded by the planner's options (at most 256 rows, kCdOwnCap own entries).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define HIFAMD_HD __host__ __device__
#else
#define HIFAMD_HD
#endif

namespace hifamd {

// element counts the kernels use that no run-time size gives
constexpr int32_t kLdsRptrSlots = 260;  // uint16 row offsets of a sparse-own component (rows + 1 <= 256)
constexpr int32_t kLdsLvlSlots = 264;   // uint8 depth-level offsets of a sparse-own component (levels + 1 <= 256)
constexpr int32_t kLdsUsRows = 256;     // k_band_us: per-row arrays of a component (<= 255 rows)
constexpr int32_t kLdsSptrSlots = 32;   // k_band_ct / k_band_ct_z: strip -> tile offsets (17 in use: at most 16 strips)

// k_top_gemm / k_top_gemm_z: two chunks of 64 panel rows at stride 80 doubles (80 KB); reused for the reduction
constexpr size_t kTopGemmLds = 2 * 64 * 80 * sizeof(double);

namespace lds {
constexpr int32_t F64 = 8, I32 = 4, U16 = 2;  // element sizes
HIFAMD_HD constexpr int32_t even(int32_t n) { return (n + 1) & ~1; }
}  // namespace lds

// k_band_cd<*, SPARSE>: right-hand sides [rows][64] | row ids | SPARSE: own values, own local sources, row offsets, depth
// levels | fused S7 (LastU): output scale and output row of every row.
// (dense-own plans: rows is a multiple of 32 -- the inverse product reads whole operand sets)
struct BandCdLds {
  int32_t tb = 0, rowid, ow_val, ow_src, ow_rptr, ow_lvl, ot, oi, end;
  HIFAMD_HD BandCdLds(int32_t rows, bool sparse, int32_t own_cap) {
    using namespace lds;
    rowid = rows * 64 * F64;
    ow_val = rowid + even(rows) * I32;
    ow_src = ow_val + own_cap * F64;
    ow_rptr = ow_src + own_cap;
    ow_lvl = ow_rptr + kLdsRptrSlots * U16;
    ot = sparse ? ow_lvl + kLdsLvlSlots : ow_val;
    oi = ot + rows * F64;
    end = oi + rows * I32;
  }
  HIFAMD_HD size_t bytes() const { return (size_t)end + 8; }
};

// k_band_cs<*, SPARSE> (one 16-column slice of a component): right-hand sides [rows][16] | per row: pivot / scale, output
// scale | SPARSE: own values | per row: row id, input row, output row | SPARSE: row offsets, own local sources, depth levels
struct BandCsLds {
  int32_t tb = 0, hd, ot, ow_val, rowid, hp, oi, ow_rptr, ow_src, ow_lvl, end;
  HIFAMD_HD BandCsLds(int32_t rows, bool sparse, int32_t own_cap) {
    using namespace lds;
    hd = rows * 16 * F64;
    ot = hd + rows * F64;
    ow_val = ot + rows * F64;
    rowid = ow_val + (sparse ? own_cap : 0) * F64;
    hp = rowid + rows * I32;
    oi = hp + rows * I32;
    ow_rptr = oi + rows * I32;
    ow_src = ow_rptr + kLdsRptrSlots * U16;
    ow_lvl = ow_src + own_cap;
    end = sparse ? ow_lvl + kLdsLvlSlots : ow_rptr;
  }
  HIFAMD_HD size_t bytes() const { return (size_t)end + 16; }
};

// k_band_ct<*, NCT, *> (NCT column tiles of 16): right-hand sides [rows][16 NCT] | per row: pivot / scale, output scale |
// per row: row id, input row, output row | strip -> tile offsets
struct BandCtLds {
  int32_t tb = 0, hd, ot, rowid, hp, oi, sptr, end;
  HIFAMD_HD BandCtLds(int32_t rows, int nct) {
    using namespace lds;
    hd = rows * 16 * nct * F64;
    ot = hd + rows * F64;
    rowid = ot + rows * F64;
    hp = rowid + rows * I32;
    oi = hp + rows * I32;
    sptr = oi + rows * I32;
    end = sptr + kLdsSptrSlots * I32;
  }
  HIFAMD_HD size_t bytes() const { return (size_t)end; }
};

// k_band_us: black rows [lds_black][64] | own values | S7 scales | row ids | S7 rows | row offsets | own sources | levels
struct BandUsLds {
  int32_t tb = 0, ow_val, ot, rowid, oi, ow_rptr, ow_src, ow_lvl, end;
  HIFAMD_HD BandUsLds(int32_t lds_black, int32_t own_cap) {
    using namespace lds;
    ow_val = lds_black * 64 * F64;
    ot = ow_val + own_cap * F64;
    rowid = ot + kLdsUsRows * F64;
    oi = rowid + kLdsUsRows * I32;
    ow_rptr = oi + kLdsUsRows * I32;
    ow_src = ow_rptr + kLdsRptrSlots * U16;
    ow_lvl = ow_src + own_cap;
    end = ow_lvl + kLdsLvlSlots;
  }
  HIFAMD_HD size_t bytes() const { return (size_t)end; }
};

// k_band_ls<CW, *> (chunk_rows = 16 CW): dependent rows [lds_dep][64] | chunk [chunk_rows][64] | own values | dependent
// row ids | row offsets (rptr_cap of them) | own sources | levels
struct BandLsLds {
  int32_t tb = 0, chunk, ow_val, rowid, ow_rptr, ow_src, ow_lvl, end;
  HIFAMD_HD BandLsLds(int32_t lds_dep, int32_t chunk_rows, int32_t own_cap, int32_t rptr_cap) {
    using namespace lds;
    chunk = lds_dep * 64 * F64;
    ow_val = chunk + chunk_rows * 64 * F64;
    rowid = ow_val + own_cap * F64;
    ow_rptr = rowid + even(lds_dep) * I32;
    ow_src = ow_rptr + rptr_cap * U16;
    ow_lvl = ow_src + own_cap;
    end = ow_lvl + kLdsLvlSlots;
  }
  HIFAMD_HD size_t bytes() const { return (size_t)end; }
};

// k_band_cs_z<*, SPARSE> (one slice of 16 complex columns): two real planes [rows][16] | per row: pivot / scale (re, im) |
// per row: row id, input row | SPARSE: own values (re, im) | row offsets | SPARSE: own local sources, depth levels |
// fused S7 (LastU): output scale and output row of every row.
// The layout is built for an EVEN row count (`rows` below, rounded up: behind an odd number of int32 the own values would
// start at 4 mod 8); own_cap is a multiple of 64.  The kernel gets `rows` as its lds_rows and derives its pointers itself
// (kernels.hip.hpp k_band_cs_z; tests/cpp/band_lds_test.cpp restates that derivation and compares).
struct BandCszLds {
  int32_t rows, t_re = 0, t_im, hdx, hdy, rowid, hp, ow_re, ow_im, ow_rptr, ow_src, ow_lvl, ot, oi, end, slack;
  HIFAMD_HD BandCszLds(int32_t nrows, bool sparse, int32_t own_cap) : rows(lds::even(nrows)) {
    using namespace lds;
    const int32_t own = sparse ? own_cap : 0;
    t_im = rows * 16 * F64;
    hdx = t_im + rows * 16 * F64;
    hdy = hdx + rows * F64;
    rowid = hdy + rows * F64;
    hp = rowid + rows * I32;
    ow_re = hp + rows * I32;
    ow_im = ow_re + own * F64;
    ow_rptr = ow_im + own * F64;
    ow_src = ow_rptr + kLdsRptrSlots * U16;
    ow_lvl = ow_src + own;
    ot = ow_lvl + (sparse ? kLdsLvlSlots : 0) + 8;
    oi = ot + rows * F64;
    end = oi + rows * I32;
    // the margin the launches have always had: the level array counted in either variant, a byte per own entry, 40 bytes
    slack = (sparse ? 0 : kLdsLvlSlots) + own + 40;
  }
  HIFAMD_HD size_t bytes() const { return (size_t)end + (size_t)slack; }
};

// k_band_ct_z (one slice of 16 complex columns): two real planes [rows][16] | per row: pivot / scale (re, im), output
// scale | per row: row id, input row, output row | strip -> tile offsets
struct BandCtzLds {
  int32_t t_re = 0, t_im, hdx, hdy, ot, rowid, hp, oi, sptr, end;
  HIFAMD_HD explicit BandCtzLds(int32_t rows) {
    using namespace lds;
    t_im = rows * 16 * F64;
    hdx = t_im + rows * 16 * F64;
    hdy = hdx + rows * F64;
    ot = hdy + rows * F64;
    rowid = ot + rows * F64;
    hp = rowid + rows * I32;
    oi = hp + rows * I32;
    sptr = oi + rows * I32;
    end = sptr + kLdsSptrSlots * I32;
  }
  HIFAMD_HD size_t bytes() const { return (size_t)end; }
};

// k_band_cd_z: the component's right-hand sides as two real planes [rows][64] | row ids
// (the kernel derives its two pointers itself; tests/cpp/band_lds_test.cpp compares)
struct BandCdzLds {
  int32_t t_re = 0, t_im, rowid, end;
  HIFAMD_HD explicit BandCdzLds(int32_t rows) {
    using namespace lds;
    t_im = rows * 64 * F64;
    rowid = t_im + rows * 64 * F64;
    end = rowid + even(rows) * I32;
  }
  HIFAMD_HD size_t bytes() const { return (size_t)end; }
};

}  // namespace hifamd
