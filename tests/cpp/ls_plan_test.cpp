// CPU test of the streamed-source plan of sparse-own L bands (hifir_amd/csrc/host.hpp ls_reorder_own / build_ls_plan /
// check_ls_plan; kernel k_band_ls).  For synthetic sparse-own triangles and for every hierarchy file given on the command
// line (written by hifamd_save) it
//   * reorders the own lists, builds and checks the plan, without and with the level's F entries;
//   * EMULATES the kernel's three phases in plain C++, reading the plan arrays the way the kernel does (16 waves, register
//     slots, chunk buffer, segment offsets, levels), and compares the result BITWISE with a row-by-row substitution over the
//     reordered lists (what k_band_cd / k_band_cs compute) and to 1e-13 with a plain triangular solve;
//   * damages plans by hand and expects check_ls_plan to refuse them;
//   * prints, per qualifying L band, the table of rows / sources / dependent rows / own entries / depth levels.
// Built and run by tests/test_ls_plan_host.py (g++ -ffp-contract=off, -fsanitize=address,undefined; no GPU).
#include "import.hpp"
#include "options.hpp"  // env_int; the planner options below stay this program's own list
#include <random>
using namespace hifamd;

static int g_bad = 0;
static long g_bands = 0, g_comps = 0, g_multi_chunk = 0;
#define EXPECT(c, what)                                              \
  if (!(c)) {                                                        \
    if (g_bad < 20) std::printf("FAILED: %s (line %d)\n", what, __LINE__); \
    ++g_bad;                                                         \
  }

// the row-by-row reference over the plan's lists: slot after slot (a valid execution order), every row of a qualifying
// band as  rhs, outside entries [ptr, csplit) in plan order, F entries, own entries in the order of the own lists;
// every other row in its CSR order.  lists == false: every row in CSR order (the plain triangular solve).
static void solve_rows(const BandPlan &P, const Csr<double> &A, const Csr<double> *F, int64_t src_row0, const std::vector<uint8_t> &band_ok,
                       const std::vector<double> &b, std::vector<double> &x, bool lists) {
  const int64_t m = A.nrows;
  std::vector<int32_t> comp_of((size_t)m, -1);
  for (int64_t bd = 0; bd < P.nbands(); ++bd) {
    if (!band_ok[(size_t)bd]) continue;
    for (int32_t c = P.wg_grp_ptr[(size_t)P.band_wg_ptr[(size_t)bd]]; c < P.wg_grp_ptr[(size_t)P.band_wg_ptr[(size_t)bd + 1]]; ++c)
      for (int32_t sl = P.grp_slot_ptr[(size_t)c]; sl < P.grp_slot_ptr[(size_t)c + 1]; ++sl) comp_of[(size_t)sl] = c;
  }
  for (int64_t sl = 0; sl < m; ++sl) {
    const int32_t i = A.rowid[(size_t)sl];
    double acc = b[(size_t)i];
    const int32_t c = comp_of[(size_t)sl];
    const int32_t kend = (c >= 0 && lists) ? P.csplit[(size_t)sl] : A.ptr[(size_t)sl + 1];
    for (int32_t k = A.ptr[(size_t)sl]; k < kend; ++k) acc = acc - A.val[(size_t)k] * x[(size_t)A.col[(size_t)k]];
    if (c >= 0 && lists) {
      if (F)
        for (int32_t k = F->ptr[(size_t)i]; k < F->ptr[(size_t)i + 1]; ++k) acc = acc - F->val[(size_t)k] * x[(size_t)(src_row0 + F->col[(size_t)k])];
      const int32_t *dsc = &P.cd_desc[(size_t)c * kCdDescWords];
      const int32_t s0 = dsc[0], own0 = dsc[20], orp0 = dsc[22], r = (int32_t)sl - s0;
      for (int32_t e = own0 + P.own_rptr[(size_t)orp0 + (size_t)r]; e < own0 + P.own_rptr[(size_t)orp0 + (size_t)r + 1]; ++e)
        acc = acc - A.val[(size_t)P.own_k[(size_t)e]] * x[(size_t)A.rowid[(size_t)(s0 + P.own_lsrc[(size_t)e])]];
    } else if (F) {
      for (int32_t k = F->ptr[(size_t)i]; k < F->ptr[(size_t)i + 1]; ++k) acc = acc - F->val[(size_t)k] * x[(size_t)(src_row0 + F->col[(size_t)k])];
    }
    x[(size_t)i] = acc;
  }
}

// k_band_ls for one component, one column: the plan arrays are read exactly as the kernel reads them
static void emulate_component(const LsPlan<double> &S, const LsStream<double> &E, int32_t c, int cw, const std::vector<double> &b,
                              std::vector<double> &x) {
  const int32_t C = 16 * cw;
  const int32_t *dsc = &S.desc[(size_t)c * kLsDescWords];
  const int32_t s0 = dsc[0], nb = dsc[1], nd = dsc[2], own0 = dsc[3], orp0 = dsc[4], lvl0 = dsc[5], nlvl = dsc[6], nch = dsc[7];
  const double *ow_val = S.own_val.data() + own0;
  const uint8_t *ow_src = S.own_src.data() + own0;
  const uint16_t *ow_rptr = S.own_rptr.data() + orp0;
  const uint8_t *ow_lvl = S.own_lvl.data() + lvl0;
  std::vector<double> dep((size_t)std::max(1, nd), 0.0), chunk((size_t)C, 0.0);
  std::vector<std::vector<double>> slot(16, std::vector<double>((size_t)kLsMaxSlots, 0.0));
  const int32_t e0 = E.base[(size_t)c];
  const uint16_t *wp = &E.wptr[(size_t)c * 33];
  // phase 1
  for (int w = 0; w < 16; ++w) {
    for (int32_t r = w; r < nd; r += 16) dep[(size_t)r] = b[(size_t)S.rowid[(size_t)(s0 + r)]];
    for (int32_t e = e0 + wp[2 * w]; e < e0 + wp[2 * w + 1]; ++e)
      dep[(size_t)E.tag[(size_t)e]] = dep[(size_t)E.tag[(size_t)e]] - E.val[(size_t)e] * x[(size_t)E.col[(size_t)e]];
    for (int q = 0; q < kLsMaxSlots; ++q) {
      const int32_t r = std::min(nd + w + 16 * q, nb - 1);  // (the kernel's clamped load)
      slot[(size_t)w][(size_t)q] = b[(size_t)S.rowid[(size_t)(s0 + r)]];
    }
    for (int32_t e = e0 + wp[2 * w + 1]; e < e0 + wp[2 * w + 2]; ++e)
      slot[(size_t)w][(size_t)E.tag[(size_t)e]] = slot[(size_t)w][(size_t)E.tag[(size_t)e]] - E.val[(size_t)e] * x[(size_t)E.col[(size_t)e]];
    for (int q = 0; q < kLsMaxSlots; ++q)
      if (nd + w + 16 * q < nb) x[(size_t)S.rowid[(size_t)(s0 + nd + w + 16 * q)]] = slot[(size_t)w][(size_t)q];
  }
  // phase 2
  for (int32_t k = 0; k < nch; ++k) {
    for (int w = 0; w < 16; ++w)
      for (int j = 0; j < cw; ++j) chunk[(size_t)(w + 16 * j)] = k * cw + j < kLsMaxSlots ? slot[(size_t)w][(size_t)(k * cw + j)] : 0.0;
    for (int32_t r = 0; r < nd; ++r) {
      const int32_t eb = ow_rptr[k * nd + r], ee = ow_rptr[k * nd + r + 1];
      double a2 = dep[(size_t)r];
      for (int32_t e = eb; e < ee; ++e) a2 = a2 - ow_val[e] * chunk[(size_t)ow_src[e]];
      dep[(size_t)r] = a2;
    }
  }
  // phase 3
  const uint16_t *rp3 = ow_rptr + nch * nd;
  for (int32_t lv = 0; lv < nlvl; ++lv)
    for (int32_t r = ow_lvl[lv]; r < ow_lvl[lv + 1]; ++r) {
      double a2 = dep[(size_t)r];
      for (int32_t e = rp3[r]; e < rp3[r + 1]; ++e) a2 = a2 - ow_val[e] * dep[(size_t)ow_src[e]];
      dep[(size_t)r] = a2;
      x[(size_t)S.rowid[(size_t)(s0 + r)]] = a2;
    }
}

static void emulate(const BandPlan &P, const Csr<double> &A, const Csr<double> *F, int64_t src_row0, const LsPlan<double> &S, bool fused,
                    const std::vector<double> &b, std::vector<double> &x) {
  // rows outside the plan's bands: the reference's row loop; the plan's bands: the kernel, component after component
  const int64_t m = A.nrows;
  std::vector<int32_t> band_of((size_t)m, -1);
  for (int64_t bd = 0; bd < P.nbands(); ++bd)
    for (int32_t c = P.wg_grp_ptr[(size_t)P.band_wg_ptr[(size_t)bd]]; c < P.wg_grp_ptr[(size_t)P.band_wg_ptr[(size_t)bd + 1]]; ++c)
      for (int32_t sl = P.grp_slot_ptr[(size_t)c]; sl < P.grp_slot_ptr[(size_t)c + 1]; ++sl) band_of[(size_t)sl] = (int32_t)bd;
  for (int64_t bd = 0; bd < P.nbands(); ++bd) {
    const int32_t c0 = P.wg_grp_ptr[(size_t)P.band_wg_ptr[(size_t)bd]], c1 = P.wg_grp_ptr[(size_t)P.band_wg_ptr[(size_t)bd + 1]];
    if (S.band_ok[(size_t)bd]) {
      for (int32_t c = c0; c < c1; ++c) emulate_component(S, fused ? S.fused : S.plain, c, S.band_cw[(size_t)bd], b, x);
      continue;
    }
    for (int32_t sl = P.grp_slot_ptr[(size_t)c0]; sl < P.grp_slot_ptr[(size_t)c1]; ++sl) {
      const int32_t i = A.rowid[(size_t)sl];
      double acc = b[(size_t)i];
      for (int32_t k = A.ptr[(size_t)sl]; k < A.ptr[(size_t)sl + 1]; ++k) acc = acc - A.val[(size_t)k] * x[(size_t)A.col[(size_t)k]];
      if (fused)
        for (int32_t k = F->ptr[(size_t)i]; k < F->ptr[(size_t)i + 1]; ++k) acc = acc - F->val[(size_t)k] * x[(size_t)(src_row0 + F->col[(size_t)k])];
      x[(size_t)i] = acc;
    }
  }
  (void)band_of;
}

template <class Fn>
static bool refused(Fn fn, const char *needle) {
  try {
    fn();
  } catch (const std::exception &e) {
    if (std::strstr(e.what(), needle)) return true;
    std::printf("refused with another message: %s (wanted: %s)\n", e.what(), needle);
    return false;
  }
  return false;
}

// one L triangle in slot order with its finished plan (build_cd_streams done); F: the level's F rows (by row id) or nullptr
static void test_triangle(const char *label, BandPlan P, const Csr<double> &A, const Csr<double> *F, int64_t n_total, bool table) {
  if (!P.cd_sparse) return;
  const int64_t m = A.nrows, src_row0 = n_total + m, nsrc = 2 * n_total;
  const BandPlan P0 = P;
  const int64_t changed = ls_reorder_own(P);
  for (int64_t bd = 0; bd < P.nbands(); ++bd)  // (a qualifying band touches its rows first: nothing in front of split)
    for (int32_t sl = P.grp_slot_ptr[(size_t)P.wg_grp_ptr[(size_t)P.band_wg_ptr[(size_t)bd]]];
         ls_band_qualifies(P, bd) && sl < P.grp_slot_ptr[(size_t)P.wg_grp_ptr[(size_t)P.band_wg_ptr[(size_t)bd + 1]]]; ++sl)
      EXPECT(P.split[(size_t)sl] == A.ptr[(size_t)sl], "a qualifying band has no prefix");
  {  // idempotent, and a permutation of every row's list
    BandPlan P2 = P;
    EXPECT(ls_reorder_own(P2) == 0 && P2.own_k == P.own_k && P2.own_lsrc == P.own_lsrc, "the reordering is idempotent");
    EXPECT(P.own_rptr == P0.own_rptr && P.own_lvl == P0.own_lvl, "the reordering keeps offsets and levels");
    std::vector<int32_t> a = P0.own_k, c = P.own_k;
    std::sort(a.begin(), a.end()), std::sort(c.begin(), c.end());
    EXPECT(a == c, "the reordering permutes the entries");
  }
  for (int chunk_req : {0, 32, 48}) {
    LsPlan<double> S;
    build_ls_plan(P, A, F, src_row0, chunk_req, S);
    if (!S.any) {
      if (chunk_req == 0) std::printf("%s: no qualifying L band\n", label);
      continue;
    }
    check_ls_plan(P, A, S, nsrc);
    EXPECT(!F || S.fused.on, "the fused streams were built");
    std::mt19937_64 g(1234 + (uint64_t)m);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    std::vector<double> b((size_t)n_total);
    for (auto &v : b) v = u(g);
    for (int fused = 0; fused < (F ? 2 : 1); ++fused) {
      std::vector<double> x0((size_t)nsrc, 0.0);
      for (int64_t k = src_row0; k < nsrc; ++k) x0[(size_t)k] = u(g);  // the child's solution, where the F entries read
      std::vector<double> xe = x0, xr = x0, xp = x0;
      emulate(P, A, fused ? F : nullptr, src_row0, S, fused != 0, b, xe);
      solve_rows(P, A, fused ? F : nullptr, src_row0, S.band_ok, b, xr, true);
      solve_rows(P, A, fused ? F : nullptr, src_row0, S.band_ok, b, xp, false);
      double scale = 0.0, diff = 0.0;
      int64_t nbits = 0;
      for (int64_t i = 0; i < m; ++i) {
        const size_t r = (size_t)A.rowid[(size_t)i];
        if (std::memcmp(&xe[r], &xr[r], sizeof(double)) != 0) ++nbits;
        scale = std::max(scale, std::fabs(xp[r])), diff = std::max(diff, std::fabs(xe[r] - xp[r]));
      }
      EXPECT(nbits == 0, "the emulated kernel equals the row-by-row substitution over the reordered lists bitwise");
      EXPECT(diff <= 1e-13 * scale, "the emulated kernel agrees with the plain triangular solve to 1e-13");
      if (chunk_req == 0)
        std::printf("%s%s: %ld rows, %ld row lists reordered, chunk %ld rows, %ld streamed sources, %ld rows in LDS, bitwise differences %ld, "
                    "vs plain solve %.2e\n", label, fused ? " (with F)" : "", (long)m, (long)changed, (long)S.chunk_rows, (long)S.sources,
                    (long)S.deps, (long)nbits, scale > 0 ? diff / scale : 0.0);
    }
    if (chunk_req != 0) continue;
    // ---- the table, and what the hand-damaged plans need
    int32_t vict_c = -1, vict_src_e = -1, vict_dep_e = -1, vict_dep_r = -1;
    for (int64_t bd = 0; bd < P.nbands(); ++bd) {
      if (!S.band_ok[(size_t)bd]) continue;
      ++g_bands;
      const int32_t c0 = P.wg_grp_ptr[(size_t)P.band_wg_ptr[(size_t)bd]], c1 = P.wg_grp_ptr[(size_t)P.band_wg_ptr[(size_t)bd + 1]];
      long rows = 0, srcs = 0, iso = 0, deps = 0, dep_read = 0, own = 0, own_src = 0, dep_first = 0;
      int mx_rows = 0, mx_src = 0, mx_dep = 0, mx_own = 0, mx_lvl = 0;
      long hist[16] = {0};
      for (int32_t c = c0; c < c1; ++c, ++g_comps) {
        const int32_t *dsc = &S.desc[(size_t)c * kLsDescWords];
        const int32_t s0 = dsc[0], nb = dsc[1], nd = dsc[2], own0 = dsc[3], orp0 = dsc[4], nch = dsc[7];
        if (nch > 1) ++g_multi_chunk;
        std::vector<uint8_t> read((size_t)nb, 0);
        const int32_t *cdd = &P0.cd_desc[(size_t)c * kCdDescWords];
        for (int32_t r = 0; r < nb; ++r) {
          bool seen_dep = false, counted = false;
          for (int32_t e = cdd[20] + P0.own_rptr[(size_t)cdd[22] + (size_t)r]; e < cdd[20] + P0.own_rptr[(size_t)cdd[22] + (size_t)r + 1]; ++e) {
            const int32_t q = P0.own_lsrc[(size_t)e];
            read[(size_t)q] = 1;
            const bool qdep = P0.own_rptr[(size_t)cdd[22] + (size_t)q + 1] > P0.own_rptr[(size_t)cdd[22] + (size_t)q];
            if (qdep) seen_dep = true;
            else if (seen_dep && !counted) ++dep_first, counted = true;  // (a dependent entry in front of a source entry, CSR order)
          }
        }
        int32_t sread = 0, dread = 0;
        for (int32_t r = 0; r < nb; ++r) {
          const bool isdep = P0.own_rptr[(size_t)cdd[22] + (size_t)r + 1] > P0.own_rptr[(size_t)cdd[22] + (size_t)r];
          if (isdep) dread += read[(size_t)r];
          else sread += read[(size_t)r];
        }
        const uint16_t *rp = &S.own_rptr[(size_t)orp0];
        const int32_t nown = rp[(size_t)(nch + 1) * (size_t)nd], nsrc_e = rp[(size_t)nch * (size_t)nd];
        rows += nb, srcs += sread, iso += (nb - nd) - sread, deps += nd, dep_read += dread, own += nown, own_src += nsrc_e;
        mx_rows = std::max(mx_rows, nb), mx_src = std::max(mx_src, nb - nd), mx_dep = std::max(mx_dep, nd), mx_own = std::max(mx_own, nown);
        mx_lvl = std::max(mx_lvl, dsc[6]);
        ++hist[std::min(15, nd / 16)];
        if (vict_c < 0 && nch >= 1 && nsrc_e > 0 && nown > nsrc_e) {
          vict_c = c, vict_src_e = own0;
          for (int32_t r = 0; r < nd; ++r)
            if (rp[(size_t)nch * (size_t)nd + (size_t)r + 1] > rp[(size_t)nch * (size_t)nd + (size_t)r]) {
              vict_dep_r = r, vict_dep_e = own0 + rp[(size_t)nch * (size_t)nd + (size_t)r];
              break;
            }
        }
      }
      if (table) {
        const double nc = (double)(c1 - c0);
        std::printf("%s L band %ld: %d components, chunk %d rows, at most %d chunks\n", label, (long)bd, c1 - c0, 16 * S.band_cw[(size_t)bd],
                    S.band_nch[(size_t)bd]);
        std::printf("  rows              mean %7.1f  max %4d  total %ld\n", rows / nc, mx_rows, rows);
        std::printf("  pure sources      mean %7.1f  max %4d  total %ld   (rows without entries that nobody reads: %ld)\n", srcs / nc, mx_src, srcs, iso);
        std::printf("  dependent rows    mean %7.1f  max %4d  total %ld   (read by others %ld, read by nobody %ld)\n", deps / nc, mx_dep, deps, dep_read,
                    deps - dep_read);
        std::printf("  own entries       mean %7.1f  max %4d  total %ld   (to pure sources %ld, to dependent rows %ld)\n", own / nc, mx_own, own, own_src,
                    own - own_src);
        std::printf("  depth levels      max %d;  rows with a dependent entry before a source entry: %ld\n", mx_lvl, dep_first);
        std::printf("  dependent rows per component:");
        for (int h = 0; h < 16; ++h)
          if (hist[h]) std::printf("  %d-%d: %ld", 16 * h, 16 * h + 15, hist[h]);
        std::printf("\n");
      }
    }
    // ---- hand-damaged plans must be refused
    if (vict_c >= 0) {
      const int32_t *dsc = &S.desc[(size_t)vict_c * kLsDescWords];
      {
        LsPlan<double> D = S;  // a dependent row declared a source
        D.desc[(size_t)vict_c * kLsDescWords + 2] -= 1;
        EXPECT(refused([&] { check_ls_plan(P, A, D, nsrc); }, "a source has an own entry"), "refuses a source with an own entry");
      }
      {
        LsPlan<double> D = S;  // an entry that points behind its chunk
        D.own_src[(size_t)vict_src_e] = 255;
        EXPECT(refused([&] { check_ls_plan(P, A, D, nsrc); }, "wrong chunk"), "refuses an entry filed under the wrong chunk");
      }
      if (vict_dep_e >= 0) {
        LsPlan<double> D = S;  // a dependent row that reads itself
        D.own_src[(size_t)vict_dep_e] = (uint8_t)vict_dep_r;
        EXPECT(refused([&] { check_ls_plan(P, A, D, nsrc); }, "own or a later level"), "refuses a level violation");
      }
      if (!S.plain.col.empty()) {
        LsPlan<double> D = S;
        D.plain.col[0] = (int32_t)nsrc;
        EXPECT(refused([&] { check_ls_plan(P, A, D, nsrc); }, "outside-entry source"), "refuses an outside entry out of range");
      }
      {
        LsPlan<double> D = S;
        D.oslot[(size_t)dsc[0]] = (int32_t)m;
        EXPECT(refused([&] { check_ls_plan(P, A, D, nsrc); }, "slot permutation"), "refuses a slot out of range");
      }
      {
        LsPlan<double> D = S;
        D.desc[(size_t)vict_c * kLsDescWords + 3] = (int32_t)S.own_val.size();
        EXPECT(refused([&] { check_ls_plan(P, A, D, nsrc); }, "own entries"), "refuses own entries out of range");
      }
      {
        LsPlan<double> D = S;
        D.plain.wptr[(size_t)vict_c * 33 + 32] = 65535;
        bool thrown = false;
        try {
          check_ls_plan(P, A, D, nsrc);
        } catch (const std::exception &) {
          thrown = true;
        }
        EXPECT(thrown, "refuses an outside-entry run out of range");
      }
    }
  }
}

// ---- synthetic sparse-own triangles: trees of chains, so that components hold many rows without entries -------------
static Csr<double> make_forest(int64_t m, int leaves, uint64_t seed) {
  // blocks of (leaves + spine) rows: `leaves` rows without entries, then a spine whose rows read 2-3 leaves and 0-2
  // earlier spine rows of the block, and now and then a row of an EARLIER block (an outside entry)
  std::mt19937_64 g(seed);
  std::uniform_real_distribution<double> u(-0.5, 0.5);
  Ccs<double> A;
  A.nrows = A.ncols = m;
  std::vector<std::vector<std::pair<int32_t, double>>> cols((size_t)m);
  const int64_t spine = std::max<int64_t>(4, leaves / 2), blk = leaves + spine;
  for (int64_t b0 = 0; b0 < m; b0 += blk) {
    const int64_t nl = std::min<int64_t>(leaves, m - b0);
    for (int64_t i = b0 + nl; i < std::min(m, b0 + blk); ++i) {
      std::vector<int64_t> srcs;
      const int cnt = 2 + (int)(g() % 2);
      for (int k = 0; k < cnt; ++k) srcs.push_back(b0 + (int64_t)(g() % (uint64_t)nl));
      const int cnt2 = (int)(g() % 3);
      for (int k = 0; k < cnt2 && i > b0 + nl; ++k) srcs.push_back(b0 + nl + (int64_t)(g() % (uint64_t)(i - b0 - nl)));
      if (b0 > 0 && g() % 5 == 0) srcs.push_back((int64_t)(g() % (uint64_t)b0));
      std::sort(srcs.begin(), srcs.end());
      srcs.erase(std::unique(srcs.begin(), srcs.end()), srcs.end());
      for (int64_t j : srcs) cols[(size_t)j].push_back({(int32_t)i, u(g)});
    }
  }
  A.colptr.assign(1, 0);
  for (int64_t j = 0; j < m; ++j) {
    std::sort(cols[(size_t)j].begin(), cols[(size_t)j].end());
    for (auto &e : cols[(size_t)j]) A.rowind.push_back(e.first), A.vals.push_back(e.second);
    A.colptr.push_back((int64_t)A.rowind.size());
  }
  return ccs_to_csr(A, false);
}

static void run_synthetic(int64_t m, int leaves, int64_t cd_rows) {
  BandOptions opt;
  opt.cd_rows = cd_rows;
  opt.cd_sparse_rows = cd_rows;
  opt.dense_block = 2048;
  opt.max_wg_rows = 16384;
  Csr<double> R = make_forest(m, leaves, 7 + (uint64_t)m + (uint64_t)leaves);
  Schedule Sc = level_schedule(R, true);
  BandPlan P = plan_bands_cd(R, Sc, true, opt, nullptr, true);
  Csr<double> Rs = permute_rows(R, P.order);
  finish_band_plan(P, Rs, opt);
  (void)plan_dense_blocks<double>(P, opt);
  build_cd_streams(P, Rs.ptr);
  // F: 0-3 entries per row into 41 columns of the child's solution
  Csr<double> F;
  F.nrows = m, F.ncols = 41;
  F.ptr.assign((size_t)m + 1, 0);
  std::mt19937_64 gf(99 + (uint64_t)m);
  for (int64_t i = 0; i < m; ++i) {
    const int cnt = (int)(gf() % 4);
    for (int k = 0; k < cnt; ++k) F.col.push_back((int32_t)(gf() % 41)), F.val.push_back(0.25 * (double)(1 + gf() % 7));
    F.ptr[(size_t)i + 1] = (int32_t)F.col.size();
  }
  char label[96];
  std::snprintf(label, sizeof label, "synthetic m=%ld leaves=%d cd_rows=%ld", (long)m, leaves, (long)cd_rows);
  test_triangle(label, P, Rs, &F, m + 41, true);
}

struct Sink {
  BandOptions opt;
  int64_t parent_nm = -1;
  size_t level_no = 0;
  const char *path = "";
  void add_level(int64_t m, int64_t n, const int64_t *Lcp, const int32_t *Lri, const double *Lv, const int64_t *Ucp,
                 const int32_t *Uri, const double *Uv, const int64_t *Ecp, const int32_t *Eri, const double *Ev, int64_t fn,
                 const int64_t *Fcp, const int32_t *Fri, const double *Fv, const double *d, const double *s, const double *t,
                 const int32_t *p, const int32_t *p_inv, const int32_t *q, const int32_t *q_inv) {
    HostLevel<double> H = import_level<double>(parent_nm, m, n, Lcp, Lri, Lv, Ucp, Uri, Uv, Ecp, Eri, Ev, fn, Fcp, Fri, Fv, d, s, t, p,
                                               p_inv, q, q_inv);
    parent_nm = n - m;
    analyze_level(H, opt, false, level_no);
    char label[512];
    std::snprintf(label, sizeof label, "%s level %zu", path, level_no);
    const bool with_f = H.F_ncols > 0 && H.m > 0 && (int64_t)H.Fr.ptr.size() == H.m + 1;
    test_triangle(label, H.Lp, H.Lr, with_f ? &H.Fr : nullptr, H.n, true);
    ++level_no;
  }
  void set_dense(int64_t, const double *, double) {}
  void set_dense_symm(int64_t, const double *, int) {}
  void set_dense_lup(int64_t, const double *) {}
};

int main(int argc, char **argv) {
  try {
    run_synthetic(6000, 120, 192);   // components of ~180 rows, ~120 sources: three chunks of 48
    run_synthetic(3000, 40, 96);     // one or two chunks
    run_synthetic(2500, 150, 240);   // more sources than nine register slots of a 32-row chunk hold: larger chunks or no plan
    run_synthetic(500, 6, 32);       // tiny components (bags): nothing qualifies or one chunk
    EXPECT(g_multi_chunk > 0, "a synthetic triangle has components that exceed one chunk");
    for (int a = 1; a < argc; ++a) {
      std::FILE *f = std::fopen(argv[a], "rb");
      char magic[8];
      int64_t vt = -1;
      if (!f || std::fread(magic, 8, 1, f) != 1 || std::fread(&vt, 8, 1, f) != 1) {
        std::printf("cannot read %s\n", argv[a]);
        return 2;
      }
      if (vt != 0) {  // (complex hierarchies have no streamed-source plan)
        std::fclose(f);
        continue;
      }
      Sink S;
      S.path = argv[a];
      BandOptions &o = S.opt;
      o.max_wg_rows = 16384;
      o.dense_block = env_int("HIFIR_AMD_DENSE_BLOCK", 2048);
      o.fuse_reorder = o.dense_block > 0;
      o.fuse_max_wgs = env_int("HIFIR_AMD_BAND_FUSE_WGS", 512);
      o.cd_fuse_max_wgs = env_int("HIFIR_AMD_CD_FUSE_WGS", 600);
      o.cd_rows = env_int("HIFIR_AMD_CD_ROWS", 128);
      o.cd_max_nnz = env_int("HIFIR_AMD_CD_NNZ", 4000);
      o.cd_sparse_rows = env_int("HIFIR_AMD_CD_SPARSE_ROWS", 192);
      o.cd_sparse_min_rows = env_int("HIFIR_AMD_CD_SPARSE_MIN_ROWS", 4096);
      o.top_max = env_int("HIFIR_AMD_TOP_ROWS", 4096);
      o.top_few_wgs = env_int("HIFIR_AMD_TOP_WGS", 96);
      const long before = g_bands;
      load_hierarchy<double>(f, S);
      std::fclose(f);
      std::printf("%s: %ld qualifying L bands\n", argv[a], g_bands - before);
    }
  } catch (const std::exception &e) {
    std::printf("error: %s\n", e.what());
    return 1;
  }
  std::printf("%ld bands, %ld components (%ld with more than one chunk), failures %d\n", g_bands, g_comps, g_multi_chunk, g_bad);
  std::printf(g_bad ? "FAILED\n" : "OK\n");
  return g_bad ? 1 : 0;
}
