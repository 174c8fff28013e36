// tests/cpp/facade_xp_test.cpp -- TEST (compiled and run on the GPU box by tests/test_gpu_xp_facade.py; needs no reference
// headers: the hierarchy is a stand-in with the precs() interface that hifamd::HIF::attach reads).
//
// The extra-precise residual through the header-only facade include/hifir_amd.hpp: set_residual_precision / residual /
// hifir under the mode / gmres_ir on the 8 x 8 Hilbert matrix rounded to float32 (condition number 1.5e10) with M = A as a
// one-level hierarchy and b = A xt for integer xt, exact in double.  Exit code 0 = every check holds.
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
  std::vector<double> mat;  // column-major
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
  const std::size_t n = 8;
  const double eps = std::ldexp(1.0, -53);
  std::vector<double> A(n * n), xt(n), b(n);  // A row-major
  for (std::size_t i = 0; i < n; ++i)
    for (std::size_t j = 0; j < n; ++j) A[i * n + j] = (double)(float)(1.0 / (double)(i + j + 1));
  for (std::size_t i = 0; i < n; ++i) xt[i] = (i % 2 ? -1.0 : 1.0) * (double)(1 + (3 * i) % 8);
  for (std::size_t i = 0; i < n; ++i) {  // 24-bit entries in [1/15, 1] times integers up to 8: every partial sum is exact
    double sum = 0.0;
    for (std::size_t j = 0; j < n; ++j) sum += A[i * n + j] * xt[j];
    b[i] = sum;
  }

  Hierarchy H;
  H.lv.resize(1);
  Level &L = H.lv[0];
  L.m = 0, L.n = n;
  L.L_B = empty_ccs(0, 0), L.U_B = empty_ccs(0, 0), L.E = empty_ccs(n, 0), L.F = empty_ccs(0, n);
  L.d_B.reserve(1);
  L.s.assign(n, 1.0), L.t.assign(n, 1.0);
  for (std::size_t i = 0; i < n; ++i) L.p.push_back((int)i);
  L.p_inv = L.q = L.q_inv = L.p;
  L.dense_solver.n = n;
  L.dense_solver.mat.resize(n * n);
  for (std::size_t i = 0; i < n; ++i)
    for (std::size_t j = 0; j < n; ++j) L.dense_solver.mat[j * n + i] = A[i * n + j];
  L.symm_dense_solver.n = 0;

  Compressed<std::ptrdiff_t, double> crs;
  crs.nr = crs.nc = n;
  crs.start.push_back(0);
  for (std::size_t i = 0; i < n; ++i) {
    for (std::size_t j = 0; j < n; ++j) crs.ind.push_back((int)j), crs.v.push_back(A[i * n + j]);
    crs.start.push_back((std::ptrdiff_t)crs.ind.size());
  }

  try {
    hifamd::HIF<double> G;
    G.attach(H, 8);
    G.set_matrix(crs);
    check("the handle starts in working precision", G.residual_precision() == HIFAMD_RESID_WORKING);

    // an iterate seven digits away: the residual is all cancellation
    std::vector<double> x(n), r0(n), r1(n), rh(n);
    for (std::size_t i = 0; i < n; ++i) x[i] = xt[i] + 1e-7 / (double)(3 + i);  // (a full mantissa: no product is exact in double)
    G.residual(crs, b, x, r0, false, HIFAMD_RESID_WORKING);
    G.residual(crs, b, x, r1, false, HIFAMD_RESID_COMPENSATED);
    bool dd_ok = true, differ = false;
    for (std::size_t i = 0; i < n; ++i) {
      __float128 ex = b[i];
      for (std::size_t j = 0; j < n; ++j) ex -= (__float128)A[i * n + j] * (__float128)x[j];  // 24 + 53 bits: exact products
      const double want = (double)ex;
      if (std::fabs(r1[i] - want) > 2.0 * eps * std::fabs(want)) dd_ok = false;
      if (r0[i] != r1[i]) differ = true;
    }
    check("residual(HIFAMD_RESID_COMPENSATED) is the rounded exact residual", dd_ok);
    check("residual(HIFAMD_RESID_WORKING) differs from it", differ);

    G.set_residual_precision(HIFAMD_RESID_COMPENSATED);
    check("set_residual_precision is read back", G.residual_precision() == HIFAMD_RESID_COMPENSATED);
    G.residual(crs, b, x, rh);  // mode -1: the handle's
    bool same = true;
    for (std::size_t i = 0; i < n; ++i) same = same && rh[i] == r1[i];
    check("residual() follows the handle's mode", same);

    std::vector<double> y(n);
    G.hifir(crs, b, 8, y);
    bool fwd = true;
    for (std::size_t i = 0; i < n; ++i) fwd = fwd && std::fabs(y[i] - xt[i]) <= 2.0 * eps * std::fabs(xt[i]);
    check("hifir under the compensated residual: |x - xt| <= 2 eps |xt|", fwd);

    G.set_residual_precision(HIFAMD_RESID_WORKING);
    G.hifir(crs, b, 8, y);
    double worst = 0.0;
    for (std::size_t i = 0; i < n; ++i) worst = std::fmax(worst, std::fabs(y[i] - xt[i]) / std::fabs(xt[i]));
    std::printf("  (working precision: forward error %.3e)\n", worst);
    check("hifir in working precision stays above 1e-10", worst > 1e-10);

    std::vector<double> z;
    int flag = -1, outer = -1, iters = -1;
    double relres = 1.0;
    std::tie(z, flag, outer, iters, relres) = G.gmres_ir(crs, b, 30, 1e-27, 1e-6, 10, 500, true);
    fwd = true;
    for (std::size_t i = 0; i < n; ++i) fwd = fwd && std::fabs(z[i] - xt[i]) <= 2.0 * eps * std::fabs(xt[i]);
    std::printf("  (gmres_ir: flag %d, %d corrections, %d inner iterations, relres %.3e)\n", flag, outer, iters, relres);
    check("gmres_ir: flag 0, at most 4 corrections, relres <= 1e-14", flag == 0 && outer <= 4 && relres <= 1e-14);
    check("gmres_ir: |x - xt| <= 2 eps |xt|", fwd);

    bool refused = false;
    try {
      G.set_residual_precision(2);
    } catch (const std::runtime_error &) {
      refused = true;
    }
    check("set_residual_precision(2) is refused", refused);
  } catch (const std::exception &e) {
    std::printf("exception: %s\n", e.what());
    return 2;
  }
  if (failures) return 1;
  std::printf("FACADE XP TEST OK\n");
  return 0;
}
