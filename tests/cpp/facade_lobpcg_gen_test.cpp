// tests/cpp/facade_lobpcg_gen_test.cpp -- TEST (compiled and run on the GPU box by tests/test_gpu_lobpcg_gen.py; needs no
// reference headers: the hierarchy is a stand-in with the precs() interface that hifamd::HIF::attach reads).
//
// Generalized LOBPCG through the header-only facade include/hifir_amd.hpp: the two smallest eigenpairs of K x = lambda M x with
// the 1D stiffness matrix K = tridiag(-1, 2, -1) and the 1D mass matrix M = tridiag(1, 4, 1) / 6 (n = 40; with
// c_j = cos(j pi / 41), lambda_j = (2 - 2 c_j) / ((4 + 2 c_j) / 6)), preconditioner I as a one-level diagonal hierarchy, a
// block of four generated candidates, then the same from a caller's start block.  Exit code 0 = every check holds.
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
  const int k = 4, nev = 2;
  Hierarchy H;  // M^{-1} = I: every row in the sparse block, d = 1, nothing else
  H.lv.resize(1);
  Level &L = H.lv[0];
  L.m = n, L.n = n;
  L.L_B = empty_ccs(n, n), L.U_B = empty_ccs(n, n), L.E = empty_ccs(0, n), L.F = empty_ccs(n, 0);
  L.d_B.assign(n, 1.0), L.s.assign(n, 1.0), L.t.assign(n, 1.0);
  for (std::size_t i = 0; i < n; ++i) L.p.push_back((int)i);
  L.p_inv = L.q = L.q_inv = L.p;
  L.dense_solver.n = 0, L.symm_dense_solver.n = 0;

  Compressed<std::ptrdiff_t, double> stiff, mass;  // tridiag(-1, 2, -1) and tridiag(1, 4, 1) / 6
  stiff.nr = stiff.nc = mass.nr = mass.nc = n;
  stiff.start.push_back(0), mass.start.push_back(0);
  for (std::size_t i = 0; i < n; ++i) {
    if (i > 0) stiff.ind.push_back((int)i - 1), stiff.v.push_back(-1.0), mass.ind.push_back((int)i - 1), mass.v.push_back(1.0 / 6.0);
    stiff.ind.push_back((int)i), stiff.v.push_back(2.0), mass.ind.push_back((int)i), mass.v.push_back(4.0 / 6.0);
    if (i + 1 < n) stiff.ind.push_back((int)i + 1), stiff.v.push_back(-1.0), mass.ind.push_back((int)i + 1), mass.v.push_back(1.0 / 6.0);
    stiff.start.push_back((std::ptrdiff_t)stiff.ind.size()), mass.start.push_back((std::ptrdiff_t)mass.ind.size());
  }
  // y = T x for a tridiagonal T with constant diagonals (off, dia, off)
  auto tri = [n](const std::vector<double> &X, int k, int c, std::size_t i, double off, double dia) {
    double y = dia * X[i * k + c];
    if (i > 0) y += off * X[(i - 1) * k + c];
    if (i + 1 < n) y += off * X[(i + 1) * k + c];
    return y;
  };
  try {
    hifamd::HIF<double> G;
    G.attach(H, 8);
    check("the diagonal hierarchy is Hermitian", G.is_hermitian());
    std::vector<double> lam, X, res;
    std::vector<int> flags;
    int steps = 0;
    const double tol = 1e-9, anorm = 4.0, bnorm = 1.0, pi = 3.14159265358979323846;
    std::tie(lam, X, res, flags, steps) = G.lobpcg_gen(stiff, mass, k, nev, std::vector<double>(), tol, 2000, 7);
    bool conv = flags.size() == 4 && lam.size() == 4 && res.size() == 4 && X.size() == n * k && steps >= 1;
    for (int c = 0; conv && c < nev; ++c) conv = flags[c] == 0 && res[c] <= tol;
    check("the first nev columns: flag 0, res <= tol", conv);
    double worst_l = 0.0, worst_r = 0.0, worst_o = 0.0;
    for (int c = 0; c < nev; ++c) {
      const double cj = std::cos((c + 1) * pi / 41.0);
      worst_l = std::fmax(worst_l, std::fabs(lam[c] - (2.0 - 2.0 * cj) / ((4.0 + 2.0 * cj) / 6.0)));
      double r2 = 0.0, x2 = 0.0;
      for (std::size_t i = 0; i < n; ++i) {
        const double r = tri(X, k, c, i, -1.0, 2.0) - lam[c] * tri(X, k, c, i, 1.0 / 6.0, 4.0 / 6.0);
        r2 += r * r, x2 += X[i * k + c] * X[i * k + c];
      }
      worst_r = std::fmax(worst_r, std::sqrt(r2) / ((anorm + std::fabs(lam[c]) * bnorm) * std::sqrt(x2)));
    }
    for (int a = 0; a < k; ++a)
      for (int b = 0; b < k; ++b) {
        double dot = 0.0;
        for (std::size_t i = 0; i < n; ++i) dot += X[i * k + a] * tri(X, k, b, i, 1.0 / 6.0, 4.0 / 6.0);
        worst_o = std::fmax(worst_o, std::fabs(dot - (a == b ? 1.0 : 0.0)));
      }
    std::printf("  (%d steps, eigenvalue error %.3e, true backward error %.3e, B-orthonormality %.3e)\n", steps, worst_l, worst_r, worst_o);
    check("eigenvalues within tol ||A||_inf of the pencil's", worst_l <= tol * anorm);
    check("true backward errors <= 2 tol", worst_r <= 2 * tol);
    check("X^H B X = I to 1e-12", worst_o <= 1e-12);
    // the result as a start block: converged at once
    std::vector<double> lam2, X2, res2;
    std::vector<int> flags2;
    int steps2 = -1;
    std::tie(lam2, X2, res2, flags2, steps2) = G.lobpcg_gen(stiff, mass, k, nev, X, 2 * tol, 50);
    check("started from its own result: 0 steps, flag 0", steps2 == 0 && flags2[0] == 0 && flags2[1] == 0);
    // the standard driver on the same object is untouched by the mass matrix: the 1D Laplacian's own eigenvalue
    std::vector<double> lam3, X3, res3;
    std::vector<int> flags3;
    int steps3 = -1;
    std::tie(lam3, X3, res3, flags3, steps3) = G.lobpcg(stiff, k, nev, std::vector<double>(), tol, 2000, 7);
    check("lobpcg on the same object: the matrix's own smallest eigenvalue",
          flags3[0] == 0 && std::fabs(lam3[0] - (2.0 - 2.0 * std::cos(pi / 41.0))) <= tol * anorm);
    bool refused = false;
    try {
      G.lobpcg_gen(stiff, mass, 17, 2, std::vector<double>(), tol, 50);
    } catch (const std::runtime_error &) {
      refused = true;
    }
    check("k = 17 is refused", refused);
    refused = false;
    try {
      G.set_nsp_const();
      G.lobpcg_gen(stiff, mass, k, nev, std::vector<double>(), tol, 50);
    } catch (const std::runtime_error &) {
      refused = true;
    }
    check("a null-space filter is refused", refused);
  } catch (const std::exception &e) {
    std::printf("exception: %s\n", e.what());
    return 2;
  }
  if (failures) return 1;
  std::printf("FACADE LOBPCG GEN TEST OK\n");
  return 0;
}
