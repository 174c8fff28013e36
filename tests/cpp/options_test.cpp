// CPU test of hifir_amd/csrc/options.hpp: EngineOptions::from_env against the values the engine's constructor computed
// when it still read the environment itself, one env_int line per switch.  Every expected value here is a literal taken
// from that constructor (and, for the BandOptions members no variable reaches, from host.hpp), never computed through
// options.hpp:
//   * nothing set: every field, for real and for complex handles;
//   * every row of the table set alone to a value that is not its default: exactly the expected fields move;
//   * the edges of the derived rules, one assertion each;
//   * the table: no name twice, every row has a case here, and rows + the names engine.hip reads where they take effect
//     = the 61 distinct names engine.hip read before the table existed.
// Built and run by tests/test_options_host.py (g++ -Wall -Werror -fsanitize=undefined; no GPU).
#include "options.hpp"

#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>
using namespace hifamd;

extern char **environ;

static int g_bad = 0, g_checks = 0;
#define EXPECT(c, ...)                                 \
  do {                                                 \
    ++g_checks;                                        \
    if (!(c)) {                                        \
      std::printf("FAILED (line %d): ", __LINE__);     \
      std::printf(__VA_ARGS__);                        \
      std::printf("\n");                               \
      ++g_bad;                                         \
    }                                                  \
  } while (0)

typedef std::map<std::string, double> Fields;

static Fields fields_of(const EngineOptions &o) {
  Fields m;
#define F(x) m[#x] = (double)o.x;
  F(use_twin) F(list_early) F(use_graph) F(min_logR) F(gemm_waves) F(spmm_tiles) F(fuse_gather) F(tail_rows)
  F(tail_probe_tol) F(tail_max_growth) F(fuse_out) F(spmm_tiles_z) F(spmm_rb) F(spmm_split_blocks) F(spmm_split)
  F(carry_wgs) F(fuse_f) F(top_gemm) F(top_last_arriver) F(zop_flags) F(zop_top_max) F(cd_dbg) F(cs_mode)
  F(cd_split_min) F(cd_split_wgs) F(narrow_spmm) F(cs_sparse) F(device_inverses) F(cs_max_wgs) F(ct_wide_wgs)
  F(ct_wide4_wgs) F(us_mode) F(ls_mode) F(ls_chunk) F(narrow_tiles) F(skip_rows) F(ct_mode_real) F(ct_mode_z) F(ct_mode)
  F(xcd_remap) F(band_pipe) F(resid_mode)
  F(band.thin_rows) F(band.band_depth) F(band.max_comp_weight) F(band.max_wg_rows) F(band.max_wgs) F(band.dense_block)
  F(band.fuse) F(band.fuse_reorder) F(band.fuse_max_wgs) F(band.dense_min_rows) F(band.cd_rows) F(band.cd_min_row_nnz)
  F(band.cd_fuse_max_wgs) F(band.cd_max_nnz) F(band.cd_sparse_max_depth) F(band.cd_sparse_min_rows)
  F(band.cd_sparse_rows) F(band.top_max) F(band.top_few_wgs) F(band.dense_max_growth)
#undef F
  return m;
}

// what a handle created with nothing set has always run with
static Fields defaults(bool z) {
  Fields m = {
      {"use_twin", 1}, {"list_early", 0}, {"use_graph", 1}, {"min_logR", 6}, {"gemm_waves", 16}, {"spmm_tiles", 1},
      {"fuse_gather", 1}, {"tail_rows", 4096}, {"tail_probe_tol", 1e-11}, {"tail_max_growth", 1e8}, {"fuse_out", 1},
      {"spmm_tiles_z", 1}, {"spmm_rb", 1}, {"spmm_split_blocks", 4096}, {"spmm_split", 1}, {"carry_wgs", 512},
      {"fuse_f", 1}, {"top_gemm", 4}, {"top_last_arriver", 0}, {"zop_flags", 0}, {"zop_top_max", 4096}, {"cd_dbg", 0},
      {"cs_mode", 1}, {"cd_split_min", 0}, {"cd_split_wgs", 600}, {"narrow_spmm", 1}, {"cs_sparse", 0},
      {"device_inverses", 1}, {"cs_max_wgs", 0}, {"ct_wide_wgs", 128}, {"ct_wide4_wgs", 1073741824}, {"us_mode", 1},
      {"ls_mode", 1}, {"ls_chunk", 0}, {"narrow_tiles", 1}, {"skip_rows", 3}, {"ct_mode_real", 1}, {"ct_mode_z", 0},
      {"ct_mode", 1}, {"xcd_remap", 1}, {"band_pipe", 1}, {"resid_mode", 0},
      {"band.thin_rows", 96}, {"band.band_depth", 32}, {"band.max_comp_weight", 1024}, {"band.max_wg_rows", 16384},
      {"band.max_wgs", 1024}, {"band.dense_block", 2048}, {"band.fuse", 1}, {"band.fuse_reorder", 1},
      {"band.fuse_max_wgs", 512}, {"band.dense_min_rows", 96}, {"band.cd_rows", 128}, {"band.cd_min_row_nnz", 4.0},
      {"band.cd_fuse_max_wgs", 600}, {"band.cd_max_nnz", 4000}, {"band.cd_sparse_max_depth", 64},
      {"band.cd_sparse_min_rows", 4096}, {"band.cd_sparse_rows", 192}, {"band.top_max", 4096}, {"band.top_few_wgs", 96},
      {"band.dense_max_growth", 1e4},
  };
  if (z) m["band.fuse"] = 0, m["band.cd_rows"] = 96, m["band.cd_max_nnz"] = 0, m["band.top_max"] = 0;
  return m;
}

static const std::string kPfx = "HIFIR_AMD_";

static void clear_env() {
  std::vector<std::string> names;
  for (char **e = environ; *e; ++e)
    if (!std::strncmp(*e, kPfx.c_str(), kPfx.size())) names.push_back(std::string(*e, std::strcspn(*e, "=")));
  for (const auto &n : names) unsetenv(n.c_str());
}

// from_env(z) with the one variable `name` (without its prefix) set to `value`
static EngineOptions with(const char *name, const char *value, bool z) {
  clear_env();
  setenv((kPfx + name).c_str(), value, 1);
  const EngineOptions o = EngineOptions::from_env(z);
  clear_env();
  return o;
}

static void expect_fields(const char *what, bool z, const EngineOptions &o, Fields want) {
  const Fields got = fields_of(o);
  EXPECT(got.size() == want.size(), "%s (%s): %zu fields dumped, %zu expected", what, z ? "complex" : "real", got.size(), want.size());
  for (const auto &kv : want) {
    const auto it = got.find(kv.first);
    EXPECT(it != got.end() && it->second == kv.second, "%s (%s): %s is %.17g, expected %.17g", what, z ? "complex" : "real",
           kv.first.c_str(), it == got.end() ? -1.0 : it->second, kv.second);
  }
}

// one variable set alone: the fields that move, on a real handle and on a complex one
struct Case {
  const char *name, *value;
  Fields real, cplx;
  Case(const char *n, const char *v, Fields both) : name(n), value(v), real(both), cplx(both) {}
  Case(const char *n, const char *v, Fields d, Fields z) : name(n), value(v), real(d), cplx(z) {}
};

int main() {
  clear_env();
  // ---- nothing set
  expect_fields("nothing set", false, EngineOptions::from_env(false), defaults(false));
  expect_fields("nothing set", true, EngineOptions::from_env(true), defaults(true));

  // ---- every row alone
  const std::vector<Case> cases = {
      {"NO_GRAPH", "1", {{"use_graph", 0}}},
      {"MIN_LOGR", "4", {{"min_logR", 4}}},
      {"GEMM_WAVES", "8", {{"gemm_waves", 8}}},
      {"BAND_PIPE", "0", {{"band_pipe", 0}}},
      {"CD_DBG", "2048", {{"cd_dbg", 2048}}},
      {"CS", "0", {{"cs_mode", 0}}},
      {"CS_MAX_WGS", "64", {{"cs_max_wgs", 64}}},
      {"CT", "0", {{"ct_mode", 0}}},
      {"CT_Z", "1", {{"ct_mode_z", 1}}},
      {"CT_REAL", "0", {{"ct_mode_real", 0}}},
      {"SKIP_ROWS", "1", {{"skip_rows", 1}}},
      {"NARROW_TILES", "0", {{"narrow_tiles", 0}}},
      {"US", "0", {{"us_mode", 0}}},
      {"LS", "0", {{"ls_mode", 0}}},
      {"LS_CHUNK", "48", {{"ls_chunk", 48}}},
      {"TOP_LAST", "1", {{"top_last_arriver", 1}}},
      {"LIST_EARLY", "1", {{"list_early", 1}}},
      {"SPMM_RB", "2", {{"spmm_rb", 2}}},
      {"SPMM_TILES_Z", "0", {{"spmm_tiles_z", 0}}},
      {"SPMM_SPLIT_BLOCKS", "100", {{"spmm_split_blocks", 100}}},
      {"CT_WIDE", "7", {{"ct_wide_wgs", 7}}},
      {"CT_WIDE4", "9", {{"ct_wide4_wgs", 9}}},
      {"CS_SPARSE", "1", {{"cs_sparse", 1}}},
      {"DEVICE_INVERSES", "0", {{"device_inverses", 0}}},
      {"NARROW_SPMM", "0", {{"narrow_spmm", 0}}},
      {"CD_SPLIT_MIN", "500", {{"cd_split_min", 500}}},
      {"CD_SPLIT_WGS", "100", {{"cd_split_wgs", 100}}},
      {"TOP_GEMM", "2", {{"top_gemm", 2}}},
      {"FUSE_F", "0", {{"fuse_f", 0}}},
      {"CARRY_WGS", "64", {{"carry_wgs", 64}}},
      {"SPMM_SPLIT", "0", {{"spmm_split", 0}}},
      {"FUSE_S7", "0", {{"fuse_out", 0}}},
      {"TAIL_ROWS", "1000", {{"tail_rows", 1000}}},
      {"TAIL_PROBE_TOL", "1e-9", {{"tail_probe_tol", 1e-9}}},
      {"TAIL_GROWTH", "10", {{"tail_max_growth", 10.0}}},
      {"FUSE_S1", "0", {{"fuse_gather", 0}}},
      {"SPMM_TILES", "0", {{"spmm_tiles", 0}}},
      {"TWIN", "0", {{"use_twin", 0}}},
      {"XCD", "0", {{"xcd_remap", 0}}},
      {"THIN_ROWS", "50", {{"band.thin_rows", 50}}},
      {"BAND_DEPTH", "8", {{"band.band_depth", 8}}},
      {"BAND_WGS", "1", {{"band.max_wgs", 1}}},
      {"BAND_WEIGHT", "99", {{"band.max_comp_weight", 99}}},
      {"DENSE_BLOCK", "512", {{"band.dense_block", 512}}},
      {"BAND_FUSE", "0", {{"band.fuse", 0}}, {}},
      {"BAND_FUSE", "1", {}, {{"band.fuse", 1}}},
      {"BAND_FUSE_WGS", "96", {{"band.fuse_max_wgs", 96}}},
      {"CD_FUSE_WGS", "0", {{"band.cd_fuse_max_wgs", 0}}},
      {"CD_ROWS", "64", {{"band.cd_rows", 64}}, {}},
      {"CD_ROWS_Z", "64", {}, {{"band.cd_rows", 64}}},
      {"CD_NNZ", "200", {{"band.cd_max_nnz", 200}}, {}},
      {"CD_NNZ_Z", "200", {}, {{"band.cd_max_nnz", 200}}},
      {"CD_SPARSE_ROWS", "100", {{"band.cd_sparse_rows", 100}}, {}},
      {"CD_SPARSE_ROWS_Z", "100", {}, {{"band.cd_sparse_rows", 100}}},
      {"TOP_ROWS", "777", {{"band.top_max", 777}, {"zop_top_max", 777}}, {{"zop_top_max", 777}}},
      {"TOP_WGS", "10", {{"band.top_few_wgs", 10}}},
      {"CD_SPARSE_MIN_ROWS", "10", {{"band.cd_sparse_min_rows", 10}}},
  };
  for (const Case &c : cases)
    for (int z = 0; z < 2; ++z) {
      Fields want = defaults(z != 0);
      for (const auto &kv : (z ? c.cplx : c.real)) {
        EXPECT(want.count(kv.first) && want[kv.first] != kv.second, "%s=%s is no change of %s", c.name, c.value, kv.first.c_str());
        want[kv.first] = kv.second;
      }
      expect_fields((std::string(c.name) + "=" + c.value).c_str(), z != 0, with(c.name, c.value, z != 0), want);
    }

  // ---- the edges of the derived rules
  for (int z = 0; z < 2; ++z) {
    EXPECT(with("MIN_LOGR", "-3", z).min_logR == 0, "MIN_LOGR=-3");
    EXPECT(with("MIN_LOGR", "9", z).min_logR == 6, "MIN_LOGR=9");
    EXPECT(with("SPMM_RB", "3", z).spmm_rb == 1, "SPMM_RB=3");
    EXPECT(with("CARRY_WGS", "0", z).carry_wgs == 1, "CARRY_WGS=0");
    const EngineOptions exact = with("DENSE_BLOCK", "0", z);
    EXPECT(exact.band.dense_block == 0 && exact.band.cd_rows == 0, "DENSE_BLOCK=0: cd_rows %ld", (long)exact.band.cd_rows);
    EXPECT(exact.band.fuse_reorder == false, "DENSE_BLOCK=0: fuse_reorder");
    EXPECT(with("CD_SPARSE_ROWS", "999", z).band.cd_sparse_rows == (z ? 192 : 240), "CD_SPARSE_ROWS=999");
    EXPECT(with("CD_SPARSE_ROWS_Z", "999", z).band.cd_sparse_rows == (z ? 240 : 192), "CD_SPARSE_ROWS_Z=999");
    EXPECT(with("NO_GRAPH", "0", z).use_graph == true, "NO_GRAPH=0");
    EXPECT(with("FUSE_F", "-1", z).fuse_f == true, "FUSE_F=-1 is not 0");
  }
  EXPECT(with("CD_ROWS", "500", false).band.cd_rows == 240, "CD_ROWS=500");
  EXPECT(with("CD_ROWS", "500", true).band.cd_rows == 96, "CD_ROWS=500, complex");
  EXPECT(with("CD_ROWS_Z", "500", true).band.cd_rows == 144, "CD_ROWS_Z=500");
  EXPECT(with("CD_ROWS_Z", "500", false).band.cd_rows == 128, "CD_ROWS_Z=500, real");
  {
    const EngineOptions o = with("TOP_ROWS", "777", true);
    EXPECT(o.band.top_max == 0 && o.zop_top_max == 777, "TOP_ROWS=777, complex: top_max %ld zop_top_max %ld", (long)o.band.top_max,
           (long)o.zop_top_max);
  }
  EXPECT(with("CD_NNZ", "200", true).band.cd_max_nnz == 0, "CD_NNZ=200, complex");
  EXPECT(with("CD_NNZ_Z", "200", false).band.cd_max_nnz == 4000, "CD_NNZ_Z=200, real");
  EXPECT(EngineOptions::from_env(false).band.fuse == true, "BAND_FUSE unset, real");
  EXPECT(EngineOptions::from_env(true).band.fuse == false, "BAND_FUSE unset, complex");
  EXPECT(with("TAIL_PROBE_TOL", "1e-9", false).tail_probe_tol == 1e-9, "TAIL_PROBE_TOL=1e-9");
  EXPECT(with("TAIL_GROWTH", "10", true).tail_max_growth == 10.0, "TAIL_GROWTH=10");
  EXPECT(with("TAIL_GROWTH", "2.5e3", false).tail_max_growth == 2500.0, "TAIL_GROWTH=2.5e3");
  // the residual mode (import.hpp resid_mode_from_env: compensated when the variable's leading integer is 1)
  const std::pair<const char *, int> resid[] = {{"1", 1}, {"0", 0}, {"2", 0}, {"", 0}, {"01", 1}, {" 1", 1}, {"1x", 1}, {"yes", 0}, {"-1", 0}};
  for (const auto &r : resid)
    for (int z = 0; z < 2; ++z) {
      Fields want = defaults(z != 0);
      want["resid_mode"] = r.second;
      expect_fields((std::string("RESIDUAL=") + r.first).c_str(), z != 0, with("RESIDUAL", r.first, z != 0), want);
    }

  // ---- the table itself
  std::set<std::string> rows, tested;
  for (const OptionRow &r : kOptionRows) {
    EXPECT(!std::strncmp(r.name, kPfx.c_str(), kPfx.size()), "row %s lacks the prefix", r.name);
    EXPECT(rows.insert(r.name).second, "row %s twice", r.name);
  }
  for (const Case &c : cases) tested.insert(kPfx + c.name);
  EXPECT(rows == tested, "the table has %zu rows, %zu of them have a case here", rows.size(), tested.size());
  // engine.hip reads these five where they take effect (the comment at the top of options.hpp); with them the table
  // accounts for every distinct name engine.hip read when the engine's constructor was the reader
  const char *at_use[] = {"PLAN_DUMP", "FINALIZE_DUMP", "PROBE_OUT", "CSPROBE_OUT", "LOAD_ANALYSIS"};
  for (const char *n : at_use) EXPECT(!rows.count(kPfx + n), "%s is read where it takes effect, not by the table", n);
  EXPECT(rows.size() + 5 == 61, "%zu rows + 5 names read at use != 61", rows.size());

  std::printf("rows %zu, cases %zu, checks %d, failures %d\n", rows.size(), cases.size(), g_checks, g_bad);
  std::printf(g_bad ? "FAILED\n" : "OK\n");
  return g_bad ? 1 : 0;
}
