// tests/cpp/facade_bgcr_test.cpp -- TEST (compiled and run on the GPU box by tests/test_gpu_blockgcr.py; needs no reference
// headers: the hierarchy is a stand-in with the precs() interface that hifamd::HIF::attach reads).
//
// Restarted block GCR through the header-only facade include/hifir_amd.hpp: one bgcr call on a nonsymmetric tridiagonal
// matrix (-1.5, 2, -0.5; n = 40) with M = I as a one-level diagonal hierarchy, four columns of which the last repeats the
// first, restart 20 (one cycle: a restart of 8 does not reach 1e-10 in 200 steps on this matrix).  Exit code 0 = every check holds.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <tuple>
#include <vector>

#include "hifir_amd.hpp"

namespace {

template <class I, class T>
struct Compressed {  // the accessors of hif::CCS / hif::CRS that the facade reads
  std::vector<I> start;
  std::vector<int> ind;
  std::vector<T> v;
  std::size_t nr, nc;
  const std::vector<I> &col_start() const { return start; }
  const std::vector<I> &row_start() const { return start; }
  const std::vector<int> &row_ind() const { return ind; }
  const std::vector<int> &col_ind() const { return ind; }
  const std::vector<T> &vals() const { return v; }
  std::size_t nrows() const { return nr; }
  std::size_t ncols() const { return nc; }
};
typedef Compressed<std::ptrdiff_t, double> ccs_t;

struct DenseBlock {
  std::vector<double> mat;
  std::size_t n;
  bool empty() const { return n == 0; }
  const DenseBlock &mat_backup() const { return *this; }
  const char *method() const { return "QRCP"; }
  std::size_t nrows() const { return n; }
  const double *data() const { return mat.data(); }
};

struct Level {
  std::size_t m, n;
  ccs_t L_B, U_B, E, F;
  std::vector<double> d_B, s, t;
  std::vector<int> p, p_inv, q, q_inv;
  DenseBlock dense_solver, symm_dense_solver;
};

struct Hierarchy {
  std::vector<Level> lv;
  const std::vector<Level> &precs() const { return lv; }
};

ccs_t empty_ccs(std::size_t nr, std::size_t nc) {
  ccs_t C;
  C.start.assign(nc + 1, 0);
  C.ind.reserve(1), C.v.reserve(1);
  C.nr = nr, C.nc = nc;
  return C;
}

int failures = 0;
void check(const char *what, bool ok) {
  std::printf("%-72s %s\n", what, ok ? "ok" : "FAIL");
  if (!ok) ++failures;
}

}  // namespace

int main() {
  const std::size_t n = 40;
  const int nrhs = 4;
  Hierarchy H;  // M^{-1} = I: every row in the sparse block, d = 1, nothing else
  H.lv.resize(1);
  Level &L = H.lv[0];
  L.m = n, L.n = n;
  L.L_B = empty_ccs(n, n), L.U_B = empty_ccs(n, n), L.E = empty_ccs(0, n), L.F = empty_ccs(n, 0);
  L.d_B.assign(n, 1.0), L.s.assign(n, 1.0), L.t.assign(n, 1.0);
  for (std::size_t i = 0; i < n; ++i) L.p.push_back((int)i);
  L.p_inv = L.q = L.q_inv = L.p;
  L.dense_solver.n = 0, L.symm_dense_solver.n = 0;

  Compressed<std::ptrdiff_t, double> crs;  // tridiag(-1.5, 2, -0.5)
  crs.nr = crs.nc = n;
  crs.start.push_back(0);
  for (std::size_t i = 0; i < n; ++i) {
    if (i > 0) crs.ind.push_back((int)i - 1), crs.v.push_back(-1.5);
    crs.ind.push_back((int)i), crs.v.push_back(2.0);
    if (i + 1 < n) crs.ind.push_back((int)i + 1), crs.v.push_back(-0.5);
    crs.start.push_back((std::ptrdiff_t)crs.ind.size());
  }
  std::vector<double> B(n * nrhs);  // [n][nrhs]
  for (std::size_t i = 0; i < n; ++i) {
    B[i * nrhs + 0] = 1.0;
    B[i * nrhs + 1] = std::sin(0.7 * (double)(i + 1));
    B[i * nrhs + 2] = (double)((7 * i) % 5) - 2.0;
    B[i * nrhs + 3] = 1.0;
  }

  try {
    hifamd::HIF<double> G;
    G.attach(H, 8);
    std::vector<double> X;
    std::vector<int> flags, iters, ranks;
    const double rtol = 1e-10;
    std::tie(X, flags, iters, ranks) = G.bgcr(crs, B, nrhs, 4, 20, rtol, 200);
    bool conv = flags.size() == 4 && iters.size() == 4, same = true;
    for (int c = 0; conv && c < nrhs; ++c) conv = flags[c] == 0 && iters[c] == iters[0] && iters[c] >= 1;
    check("four columns: flag 0, one step count", conv);
    check("ranks: the duplicate column is deflated at the start", ranks.size() == 2 && ranks[0] == 3 && ranks[1] >= 1 && ranks[1] <= 3);
    double worst = 0.0;
    for (int c = 0; c < nrhs; ++c) {
      double r2 = 0.0, b2 = 0.0;
      for (std::size_t i = 0; i < n; ++i) {
        double ax = 2.0 * X[i * nrhs + c];
        if (i > 0) ax -= 1.5 * X[(i - 1) * nrhs + c];
        if (i + 1 < n) ax -= 0.5 * X[(i + 1) * nrhs + c];
        r2 += (ax - B[i * nrhs + c]) * (ax - B[i * nrhs + c]);
        b2 += B[i * nrhs + c] * B[i * nrhs + c];
      }
      worst = std::fmax(worst, std::sqrt(r2 / b2));
    }
    for (std::size_t i = 0; i < n; ++i) same = same && std::fabs(X[i * nrhs] - X[i * nrhs + 3]) <= 1e-9 * std::fabs(X[i * nrhs]);
    std::printf("  (%d steps, ranks %d %d, worst true residual %.3e)\n", iters.empty() ? -1 : iters[0], ranks[0], ranks[1], worst);
    check("true residuals <= 2 rtol", worst <= 2 * rtol);
    check("the duplicate column gets its original's solution", same);
    bool refused = false;
    try {
      G.bgcr(crs, B, nrhs, 65, 8, rtol, 200);
    } catch (const std::runtime_error &) {
      refused = true;
    }
    check("block = 65 is refused", refused);
    refused = false;
    try {
      G.bgcr(crs, B, nrhs, 4, HIFAMD_BGCR_MAX_RESTART + 1, rtol, 200);
    } catch (const std::runtime_error &) {
      refused = true;
    }
    check("restart = HIFAMD_BGCR_MAX_RESTART + 1 is refused", refused);
  } catch (const std::exception &e) {
    std::printf("exception: %s\n", e.what());
    return 2;
  }
  if (failures) return 1;
  std::printf("FACADE BGCR TEST OK\n");
  return 0;
}
