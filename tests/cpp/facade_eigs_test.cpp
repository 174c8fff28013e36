// tests/cpp/facade_eigs_test.cpp -- TEST (compiled and run on the GPU box by tests/test_gpu_eigs.py; needs no reference
// headers: the hierarchy is a stand-in with the precs() interface that hifamd::HIF::attach reads).
//
// The locked LOBPCG sweeps and the B-orthogonal projector through the header-only facade include/hifir_amd.hpp: the six
// smallest eigenpairs of K x = lambda x and of K x = lambda M x with the 1D stiffness matrix K = tridiag(-1, 2, -1) and the 1D
// mass matrix M = tridiag(1, 4, 1) / 6 (n = 40; with c_j = cos(j pi / 41), lambda_j = 2 - 2 c_j and
// (2 - 2 c_j) / ((4 + 2 c_j) / 6)), preconditioner I as a one-level diagonal hierarchy, blocks of k = 4 candidates with one
// guard column (two sweeps of three), then the next three from the first six as constraints.  Exit code 0 = every check holds.
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
  const int k = 4, guard = 1, nev = 6;
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
    const double tol = 1e-9, anorm = 4.0, pi = 3.14159265358979323846;
    const std::vector<double> none;
    for (int gen = 0; gen < 2; ++gen) {
      std::vector<double> lam, X, res;
      std::vector<int> flags, info;
      if (gen)
        std::tie(lam, X, res, flags, info) = G.eigsh(stiff, mass, nev, k, guard, none, 0, none, tol, 4000, 7);
      else
        std::tie(lam, X, res, flags, info) = G.eigsh(stiff, nev, k, guard, none, 0, none, tol, 4000, 7);
      bool conv = flags.size() == 6 && lam.size() == 6 && res.size() == 6 && X.size() == n * nev && info.size() == 4;
      for (int c = 0; conv && c < nev; ++c) conv = flags[c] == 0 && res[c] <= tol;
      check(gen ? "pencil: six columns locked, res <= tol" : "matrix: six columns locked, res <= tol", conv);
      check("info4: at least two sweeps, six locked", conv && info[1] >= 2 && info[2] == 6 && info[0] >= 2);
      double worst_l = 0.0, worst_o = 0.0;
      for (int c = 0; c < nev; ++c) {
        const double cj = std::cos((c + 1) * pi / 41.0);
        worst_l = std::fmax(worst_l, std::fabs(lam[c] - (2.0 - 2.0 * cj) / (gen ? (4.0 + 2.0 * cj) / 6.0 : 1.0)));
      }
      for (int a = 0; a < nev; ++a)
        for (int b = 0; b < nev; ++b) {
          double dot = 0.0;
          for (std::size_t i = 0; i < n; ++i) dot += X[i * nev + a] * (gen ? tri(X, nev, b, i, 1.0 / 6.0, 4.0 / 6.0) : X[i * nev + b]);
          worst_o = std::fmax(worst_o, std::fabs(dot - (a == b ? 1.0 : 0.0)));
        }
      std::printf("  (%d steps in %d sweeps, eigenvalue error %.3e, B-orthonormality %.3e)\n", info[0], info[1], worst_l, worst_o);
      check("eigenvalues within tol ||A||_inf", worst_l <= tol * anorm);
      check("X^H B X = I to 1e-12", worst_o <= 1e-12);
      // the six as constraints: the next three eigenvalues, B-orthogonal to them
      std::vector<double> lam2, X2, res2;
      std::vector<int> flags2, info2;
      if (gen)
        std::tie(lam2, X2, res2, flags2, info2) = G.eigsh(stiff, mass, 3, k, guard, X, nev, none, tol, 4000, 9);
      else
        std::tie(lam2, X2, res2, flags2, info2) = G.eigsh(stiff, 3, k, guard, X, nev, none, tol, 4000, 9);
      double worst2 = 0.0, cross = 0.0;
      for (int c = 0; c < 3; ++c) {
        const double cj = std::cos((c + 7) * pi / 41.0);
        worst2 = std::fmax(worst2, std::fabs(lam2[c] - (2.0 - 2.0 * cj) / (gen ? (4.0 + 2.0 * cj) / 6.0 : 1.0)));
      }
      for (int a = 0; a < nev; ++a)
        for (int b = 0; b < 3; ++b) {
          double dot = 0.0;
          for (std::size_t i = 0; i < n; ++i) dot += X[i * nev + a] * (gen ? tri(X2, 3, b, i, 1.0 / 6.0, 4.0 / 6.0) : X2[i * 3 + b]);
          cross = std::fmax(cross, std::fabs(dot));
        }
      check("behind six constraints: eigenvalues 7 .. 9, flags 0", flags2[0] == 0 && flags2[1] == 0 && flags2[2] == 0 && worst2 <= tol * anorm);
      check("Y^H B X = 0 to 1e-12", cross <= 1e-12);
      // the projector alone: W <- W - Y (B Y)^H W is B-orthogonal to Y, and projecting again changes nothing much
      std::vector<double> W(n * 2);
      for (std::size_t i = 0; i < n * 2; ++i) W[i] = std::sin(0.37 * (double)(i + 1));
      G.b_project(W, 2, X, nev, gen != 0);
      double off = 0.0;
      for (int a = 0; a < nev; ++a)
        for (int b = 0; b < 2; ++b) {
          double dot = 0.0;
          for (std::size_t i = 0; i < n; ++i) dot += X[i * nev + a] * (gen ? tri(W, 2, b, i, 1.0 / 6.0, 4.0 / 6.0) : W[i * 2 + b]);
          off = std::fmax(off, std::fabs(dot));
        }
      check("b_project: (B Y)^H W = 0 to 1e-12", off <= 1e-12);
    }
    bool refused = false;
    try {
      G.eigsh(stiff, 125, k, guard, std::vector<double>(n * 4, 0.0), 4, none, tol, 50);
    } catch (const std::runtime_error &) {
      refused = true;
    }
    check("m0 + nev = 129 is refused", refused);
    refused = false;
    try {
      G.eigsh(stiff, nev, k, k, none, 0, none, tol, 50);
    } catch (const std::runtime_error &) {
      refused = true;
    }
    check("guard = k is refused", refused);
  } catch (const std::exception &e) {
    std::printf("exception: %s\n", e.what());
    return 2;
  }
  if (failures) return 1;
  std::printf("FACADE EIGS TEST OK\n");
  return 0;
}
