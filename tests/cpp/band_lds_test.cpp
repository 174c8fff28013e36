// CPU test of the dynamic-LDS layouts of the component-band kernels (hifir_amd/csrc/band_lds.hpp): the one statement of
// each layout that the kernels take their pointers from and the host its byte counts.  Over a grid of the sizes the engine
// can pass, for every layout:
//   * the arrays lie in ascending order and do not overlap, with the element counts the kernel uses;
//   * every array is aligned to its element type, and starts a whole number of elements of the array in front of it
//     behind that array (the kernels step from one array to the next in elements of the former: lds_next);
//   * the last array ends at or before bytes().
// bytes() at the default sizes is pinned to literals: the sizes the launches have always asked for.
// k_band_cs_z and k_band_cd_z derive their pointers in their own text (their code generation did not survive any other
// way to write it): that text is restated here on a real buffer and must give the struct's offsets.
// Built and run by tests/test_band_lds_host.py (g++; no GPU).
#include "host.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace hifamd;

static long g_bad = 0, g_sets = 0;
#define EXPECT(c, ...)                     \
  if (!(c)) {                              \
    if (g_bad < 20) {                      \
      std::printf("FAILED (line %d): ", __LINE__); \
      std::printf(__VA_ARGS__);            \
      std::printf("\n");                   \
    }                                      \
    ++g_bad;                               \
  }

struct Arr {
  const char *name;
  int32_t off, elem, count;  // byte offset, element size, elements the kernel uses
};

static void check(const char *layout, const std::vector<Arr> &a, size_t bytes, int p0, int p1, int p2, int p3) {
  ++g_sets;
  int32_t prev_end = 0;
  for (size_t k = 0; k < a.size(); ++k) {
    const Arr &x = a[k];
    EXPECT(x.off >= 0 && x.count >= 0, "%s(%d,%d,%d,%d): %s at %d", layout, p0, p1, p2, p3, x.name, x.off);
    EXPECT(x.off % x.elem == 0, "%s(%d,%d,%d,%d): %s at %d is not aligned to %d", layout, p0, p1, p2, p3, x.name, x.off, x.elem);
    EXPECT(x.off >= prev_end, "%s(%d,%d,%d,%d): %s at %d overlaps the array in front of it (ends at %d)", layout, p0, p1, p2,
           p3, x.name, x.off, prev_end);
    if (k > 0) {
      EXPECT(x.off >= a[k - 1].off, "%s(%d,%d,%d,%d): %s lies in front of %s", layout, p0, p1, p2, p3, x.name, a[k - 1].name);
      EXPECT((x.off - a[k - 1].off) % a[k - 1].elem == 0, "%s(%d,%d,%d,%d): %s is no whole number of elements behind %s", layout,
             p0, p1, p2, p3, x.name, a[k - 1].name);
    }
    prev_end = x.off + x.elem * x.count;
  }
  EXPECT((size_t)prev_end <= bytes, "%s(%d,%d,%d,%d): the last array ends at %d, bytes() = %zu", layout, p0, p1, p2, p3, prev_end,
         bytes);
}

// the arrays of each layout in the order they lie in, with the most elements the kernel touches for these sizes
// (a component of `rows` rows has rows + 1 row offsets and at most rows + 1 level offsets)
static void cd(int rows, bool sparse, int own) {
  const BandCdLds l(rows, sparse, own);
  std::vector<Arr> a = {{"tb", l.tb, 8, rows * 64}, {"rowid", l.rowid, 4, rows}};
  if (sparse)
    a.insert(a.end(), {{"ow_val", l.ow_val, 8, own}, {"ow_src", l.ow_src, 1, own}, {"ow_rptr", l.ow_rptr, 2, rows + 1}, {"ow_lvl", l.ow_lvl, 1, rows + 1}});
  a.insert(a.end(), {{"ot", l.ot, 8, rows}, {"oi", l.oi, 4, rows}});
  check("cd", a, l.bytes(), rows, sparse, own, 0);
}
static void cs(int rows, bool sparse, int own) {
  const BandCsLds l(rows, sparse, own);
  std::vector<Arr> a = {{"tb", l.tb, 8, rows * 16}, {"hd", l.hd, 8, rows}, {"ot", l.ot, 8, rows}, {"ow_val", l.ow_val, 8, sparse ? own : 0},
                        {"rowid", l.rowid, 4, rows}, {"hp", l.hp, 4, rows}, {"oi", l.oi, 4, rows}};
  if (sparse) a.insert(a.end(), {{"ow_rptr", l.ow_rptr, 2, rows + 1}, {"ow_src", l.ow_src, 1, own}, {"ow_lvl", l.ow_lvl, 1, rows + 1}});
  check("cs", a, l.bytes(), rows, sparse, own, 0);
}
static void ct(int rows, int nct) {
  const BandCtLds l(rows, nct);
  check("ct", {{"tb", l.tb, 8, rows * 16 * nct}, {"hd", l.hd, 8, rows}, {"ot", l.ot, 8, rows}, {"rowid", l.rowid, 4, rows},
               {"hp", l.hp, 4, rows}, {"oi", l.oi, 4, rows}, {"sptr", l.sptr, 4, 17}},
        l.bytes(), rows, nct, 0, 0);
}
static void us(int black, int own) {  // (a component of at most 255 rows)
  const BandUsLds l(black, own);
  check("us", {{"tb", l.tb, 8, black * 64}, {"ow_val", l.ow_val, 8, own}, {"ot", l.ot, 8, 255}, {"rowid", l.rowid, 4, 255},
               {"oi", l.oi, 4, 255}, {"ow_rptr", l.ow_rptr, 2, 256}, {"ow_src", l.ow_src, 1, own}, {"ow_lvl", l.ow_lvl, 1, 256}},
        l.bytes(), black, own, 0, 0);
}
static void ls(int dep, int cw, int own, int rptr) {  // (a component of at most 255 rows)
  const BandLsLds l(dep, 16 * cw, own, rptr);
  check("ls", {{"tb", l.tb, 8, dep * 64}, {"chunk", l.chunk, 8, 16 * cw * 64}, {"ow_val", l.ow_val, 8, own}, {"rowid", l.rowid, 4, dep},
               {"ow_rptr", l.ow_rptr, 2, rptr}, {"ow_src", l.ow_src, 1, own}, {"ow_lvl", l.ow_lvl, 1, 256}},
        l.bytes(), dep, cw, own, rptr);
  EXPECT(l.bytes() == ls_lds_bytes(dep, 16 * cw, own, rptr), "ls(%d,%d,%d,%d): the planner's size differs", dep, cw, own, rptr);
}
// kernels.hip.hpp k_band_cs_z, the lines that carve cs_buf (lds_rows = the layout's even row count), as offsets
template <bool SPARSE>
static void csz_kernel_text(double *cs_buf, int32_t lds_rows, int32_t own_cap, int32_t *off) {
  double *t_re = cs_buf, *t_im = cs_buf + (size_t)lds_rows * 16;
  double *s_hdx = t_im + (size_t)lds_rows * 16, *s_hdy = s_hdx + lds_rows;
  int32_t *s_rowid = reinterpret_cast<int32_t *>(s_hdy + lds_rows);
  int32_t *s_hp = s_rowid + lds_rows;
  double *ow_re = reinterpret_cast<double *>(s_hp + ((lds_rows + 1) & ~1));
  double *ow_im = ow_re + (SPARSE ? own_cap : 0);
  uint16_t *ow_rptr = reinterpret_cast<uint16_t *>(ow_im + (SPARSE ? own_cap : 0));
  uint8_t *ow_src = reinterpret_cast<uint8_t *>(ow_rptr + 260);
  uint8_t *ow_lvl = ow_src + (SPARSE ? own_cap : 0);
  double *s_ot = reinterpret_cast<double *>(ow_lvl + (SPARSE ? 264 : 0) + 8);
  s_ot = reinterpret_cast<double *>((reinterpret_cast<uintptr_t>(s_ot) + 7) & ~(uintptr_t)7);
  int32_t *s_oi = reinterpret_cast<int32_t *>(s_ot + lds_rows);
  const void *p[13] = {t_re, t_im, s_hdx, s_hdy, s_rowid, s_hp, ow_re, ow_im, ow_rptr, ow_src, ow_lvl, s_ot, s_oi};
  for (int k = 0; k < 13; ++k) off[k] = (int32_t)(reinterpret_cast<const char *>(p[k]) - reinterpret_cast<const char *>(cs_buf));
}
alignas(8) static double g_block[160 * 1024 / 8 + 8192];  // (addresses only: nothing is read or written)

static void csz(int rows, bool sparse, int own) {
  const BandCszLds l(rows, sparse, own);
  EXPECT(l.rows >= rows && l.rows <= rows + 1 && l.rows % 2 == 0, "csz(%d): layout rows %d", rows, l.rows);
  int32_t k_off[13];
  if (sparse) csz_kernel_text<true>(g_block, l.rows, own, k_off);
  else csz_kernel_text<false>(g_block, l.rows, own, k_off);
  const int32_t s_off[13] = {l.t_re, l.t_im, l.hdx, l.hdy, l.rowid, l.hp, l.ow_re, l.ow_im, l.ow_rptr, l.ow_src, l.ow_lvl, l.ot, l.oi};
  EXPECT(std::memcmp(k_off, s_off, sizeof k_off) == 0, "csz(%d,%d,%d): the kernel's text gives other offsets", rows, sparse, own);
  std::vector<Arr> a = {{"t_re", l.t_re, 8, rows * 16}, {"t_im", l.t_im, 8, rows * 16}, {"hdx", l.hdx, 8, rows}, {"hdy", l.hdy, 8, rows},
                        {"rowid", l.rowid, 4, rows}, {"hp", l.hp, 4, rows}};
  if (sparse)
    a.insert(a.end(), {{"ow_re", l.ow_re, 8, own}, {"ow_im", l.ow_im, 8, own}, {"ow_rptr", l.ow_rptr, 2, rows + 1}, {"ow_src", l.ow_src, 1, own},
                       {"ow_lvl", l.ow_lvl, 1, rows + 1}});
  a.insert(a.end(), {{"ot", l.ot, 8, rows}, {"oi", l.oi, 4, rows}});
  check("csz", a, l.bytes(), rows, sparse, own, 0);
}
static void ctz(int rows) {
  const BandCtzLds l(rows);
  check("ctz", {{"t_re", l.t_re, 8, rows * 16}, {"t_im", l.t_im, 8, rows * 16}, {"hdx", l.hdx, 8, rows}, {"hdy", l.hdy, 8, rows},
                {"ot", l.ot, 8, rows}, {"rowid", l.rowid, 4, rows}, {"hp", l.hp, 4, rows}, {"oi", l.oi, 4, rows}, {"sptr", l.sptr, 4, 17}},
        l.bytes(), rows, 0, 0, 0);
}
static void cdz(int rows) {
  const BandCdzLds l(rows);
  {  // kernels.hip.hpp k_band_cd_z, the lines that carve cd_tbuf
    double *cd_tbuf = g_block;
    const int32_t lds_rows = rows;
    double *t_re = cd_tbuf, *t_im = cd_tbuf + (size_t)lds_rows * 64;
    int32_t *cd_rowid = reinterpret_cast<int32_t *>(cd_tbuf + (size_t)lds_rows * 128);
    EXPECT((char *)t_re - (char *)cd_tbuf == l.t_re && (char *)t_im - (char *)cd_tbuf == l.t_im && (char *)cd_rowid - (char *)cd_tbuf == l.rowid,
           "cdz(%d): the kernel's text gives other offsets", rows);
  }
  check("cdz", {{"t_re", l.t_re, 8, rows * 64}, {"t_im", l.t_im, 8, rows * 64}, {"rowid", l.rowid, 4, rows}}, l.bytes(), rows, 0, 0, 0);
}

int main() {
  // ---- the grid: dense rows 32 ... 256 by 32, sparse rows 1 ... 240, own_cap in multiples of 64 up to kCdOwnCap, NCT 1 / 2 / 4,
  // CW 2 ... 4 (its NCH does not enter the layout but bounds rptr_cap), rptr_cap in multiples of 4
  for (int rows = 32; rows <= 256; rows += 32) {
    cd(rows, false, 0), cd(rows, false, kCdOwnCap), cs(rows, false, 0), cs(rows, false, kCdOwnCap), csz(rows, false, 0), ctz(rows);
    for (int nct : {1, 2, 4}) ct(rows, nct);
  }
  for (int rows = 1; rows <= 256; ++rows) cdz(rows);
  for (int own = 64; own <= kCdOwnCap; own += 64) {
    for (int rows = 1; rows <= 240; ++rows) cd(rows, true, own), cs(rows, true, own), csz(rows, true, own);
    for (int black = 1; black <= 255; ++black) us(black, own);
  }
  // (k_band_ls: every multiple of 4 up to the row offsets of the most chunks the instance allows, (NCH + 1) dep + 1)
  for (int dep = 1; dep <= 255; ++dep)
    for (int cw = 2; cw <= 4; ++cw)
      for (int own = 64; own <= kCdOwnCap; own += 64)
        for (int rptr = 4; rptr <= (((ls_max_chunks(cw) + 1) * dep + 1 + 3) & ~3); rptr += 4) ls(dep, cw, own, rptr);
  // ---- bytes() at the default sizes (HIFIR_AMD_CD_ROWS 128, _CD_SPARSE_ROWS 192, _CD_ROWS_Z 96, kCdOwnCap own entries)
  EXPECT(kCdOwnCap == 4096, "kCdOwnCap");
  EXPECT(BandCdLds(128, false, kCdOwnCap).bytes() == 67592, "cd dense");
  EXPECT(BandCdLds(192, true, kCdOwnCap).bytes() == 139032, "cd sparse");
  EXPECT(BandCsLds(128, false, kCdOwnCap).bytes() == 19984, "cs dense");
  EXPECT(BandCsLds(192, true, kCdOwnCap).bytes() == 67616, "cs sparse");
  EXPECT(BandCtLds(128, 1).bytes() == 20096, "ct1");
  EXPECT(BandCtLds(128, 2).bytes() == 36480, "ct2");
  EXPECT(BandCtLds(128, 4).bytes() == 69248, "ct4");
  EXPECT(BandCtLds(256, 2).bytes() == 72832, "ct2 at 256 rows");  // (HIFIR_AMD_CD_ROWS = 240: more than 64 KB)
  EXPECT(BandUsLds(192, kCdOwnCap).bytes() == 140048, "us");
  EXPECT(BandLsLds(128, 48, 1024, 388).bytes() == 100880, "ls");
  EXPECT(BandCszLds(192, true, kCdOwnCap).bytes() == 130624, "csz sparse");
  EXPECT(BandCszLds(96, false, 0).bytes() == 28864, "csz dense");
  EXPECT(BandCtzLds(96).bytes() == 28160, "ctz");
  EXPECT(BandCdzLds(96).bytes() == 98688, "cdz");
  EXPECT(kTopGemmLds == 81920 && kLsLdsMax == 81920, "fixed sizes");
  std::printf("argument sets %ld, failures %ld\n", g_sets, g_bad);
  std::printf(g_bad ? "FAILED\n" : "OK\n");
  return g_bad ? 1 : 0;
}
