// Host side of the null-space search (hifir_amd/csrc/import.hpp nsp_find_rotation, nsp_chol_inverse, nsp_probe_fill --
// the very code engine.hip compiles for hifamd_nsp_find), driven directly so that it runs under
// -fsanitize=address,undefined:
//   * a block V = U diag(s) W^H with singular values graded 1 ... 1e-8 (Gram spectrum 1 ... 1e-16): the rotation
//     returns the eigenvalues descending, and after the rotation and two Cholesky steps the leading columns (those
//     above the rounding of the Gram matrix) are orthonormal to 1e-12;
//   * the Cholesky step preserves the order: its matrix is upper triangular, V R^{-1} is orthonormal to 1e-12 for a
//     well-conditioned block;
//   * a rank-deficient block (exactly zero columns from index 5 on): the Cholesky step keeps exactly 5 columns and
//     zeroes the others, the rotation keeps at least 5 and returns finite numbers; a zero and a NaN Gram matrix keep
//     nothing -- no crash, no non-finite output;
//   * real and complex; the Gram matrix is handed over with the device's layout and row stride (64).
// With a file name as its argument it also writes the probe blocks of a few seeds (nsp_probe_fill) for the numpy
// restatement of the header's formula in tests/test_nsp_find_host.py.
// Build: g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -I hifir_amd/csrc tests/cpp/nsp_find_test.cpp
// Exit code 0 = clean; every failure is printed.
#include "import.hpp"

#include <cstdio>
#include <random>

using namespace hifamd;

static int g_fail = 0;
#define EXPECT(cond, ...)                  \
  do {                                     \
    if (!(cond)) {                         \
      ++g_fail;                            \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);   \
      std::fprintf(stderr, "\n");          \
    }                                      \
  } while (0)

static const int64_t K = 16, LDG = 64;

static void fill(double &v, std::mt19937_64 &g) { v = std::uniform_real_distribution<double>(-1, 1)(g); }
static void fill(zdouble &v, std::mt19937_64 &g) {
  std::uniform_real_distribution<double> u(-1, 1);
  v = zdouble(u(g), u(g));
}

// [rows][16] with orthonormal columns
template <class T>
static std::vector<T> random_orthonormal(int64_t rows, unsigned seed) {
  std::mt19937_64 g(seed);
  std::vector<T> V((size_t)(rows * K));
  for (auto &v : V) fill(v, g);
  return nsp_orthonormalize<T>(rows, K, V.data(), K, K);
}

// the Gram matrix as the device leaves it: G[j * 64 + c] = v_j^H v_c, the other entries poisoned
template <class T>
static std::vector<T> gram(int64_t n, const std::vector<T> &V) {
  std::vector<T> G((size_t)(K * LDG), T(777.0));
  for (int64_t j = 0; j < K; ++j)
    for (int64_t c = 0; c < K; ++c) {
      T h = T(0);
      for (int64_t i = 0; i < n; ++i) h += conj_(V[(size_t)(i * K + j)]) * V[(size_t)(i * K + c)];
      G[(size_t)(j * LDG + c)] = h;
    }
  return G;
}

// V <- V M, M row-major 16 x 16 (what k_blk_rmul does)
template <class T>
static void rmul(int64_t n, std::vector<T> &V, const std::vector<T> &M) {
  std::vector<T> row((size_t)K);
  for (int64_t i = 0; i < n; ++i) {
    for (int64_t c = 0; c < K; ++c) {
      T a = T(0);
      for (int64_t j = 0; j < K; ++j) a += V[(size_t)(i * K + j)] * M[(size_t)(j * K + c)];
      row[(size_t)c] = a;
    }
    std::copy(row.begin(), row.end(), V.begin() + i * K);
  }
}

template <class T>
static double orth_defect(int64_t n, const std::vector<T> &V, int64_t lead) {
  const std::vector<T> G = gram<T>(n, V);
  double worst = 0.0;
  for (int64_t j = 0; j < lead; ++j)
    for (int64_t c = 0; c < lead; ++c) worst = std::max(worst, abs_(G[(size_t)(j * LDG + c)] - T(j == c ? 1.0 : 0.0)));
  return worst;
}

template <class T>
static bool all_finite(const std::vector<T> &M) {
  for (const T &v : M)
    if (!std::isfinite(abs1_(v))) return false;
  return true;
}

template <class T>
static void check_graded(const char *what) {
  const int64_t n = 200;
  const std::vector<T> U = random_orthonormal<T>(n, 3), W = random_orthonormal<T>(K, 4);
  std::vector<T> V((size_t)(n * K), T(0));
  for (int64_t i = 0; i < n; ++i)
    for (int64_t c = 0; c < K; ++c) {
      T a = T(0);
      for (int64_t l = 0; l < K; ++l) a += U[(size_t)(i * K + l)] * std::pow(10.0, -8.0 * (double)l / 15.0) * conj_(W[(size_t)(c * K + l)]);
      V[(size_t)(i * K + c)] = a;
    }
  std::vector<T> M((size_t)(K * K));
  std::vector<double> w((size_t)K);
  const int kept = nsp_find_rotation<T>(gram<T>(n, V).data(), LDG, M.data(), w.data());
  EXPECT(kept >= 8 && kept <= 16, "%s graded: kept %d", what, kept);
  for (int64_t c = 1; c < K; ++c) EXPECT(w[(size_t)c] <= w[(size_t)c - 1], "%s graded: eigenvalue %lld not descending", what, (long long)c);
  EXPECT(std::fabs(w[0] - 1.0) <= 1e-12, "%s graded: largest eigenvalue %.17g", what, w[0]);
  for (int64_t c = 0; c < 8; ++c) {
    const double want = std::pow(10.0, -16.0 * (double)c / 15.0);
    EXPECT(std::fabs(w[(size_t)c] - want) <= 1e-6 * want, "%s graded: eigenvalue %lld = %.6e, expected %.6e", what, (long long)c, w[(size_t)c], want);
  }
  EXPECT(all_finite(M), "%s graded: rotation not finite", what);
  rmul<T>(n, V, M);
  for (int pass = 0; pass < 2; ++pass) {
    const int kc = nsp_chol_inverse<T>(gram<T>(n, V).data(), LDG, M.data());
    EXPECT(kc >= 8, "%s graded: Cholesky pass %d kept %d", what, pass, kc);
    EXPECT(all_finite(M), "%s graded: Cholesky inverse not finite", what);
    rmul<T>(n, V, M);
  }
  const double d = orth_defect<T>(n, V, 8);
  EXPECT(d <= 1e-12, "%s graded: leading columns |Q^H Q - I| = %.3e", what, d);
  // the leading columns span the leading left singular vectors, in order: q_c is +-u_c up to the gaps' rounding
  for (int64_t c = 0; c < 4; ++c) {
    T h = T(0);
    for (int64_t i = 0; i < n; ++i) h += conj_(U[(size_t)(i * K + c)]) * V[(size_t)(i * K + c)];
    EXPECT(std::fabs(abs_(h) - 1.0) <= 1e-6, "%s graded: column %lld is not the singular vector (|u^H q| = %.9f)", what, (long long)c, abs_(h));
  }
}

template <class T>
static void check_cholesky(const char *what) {
  const int64_t n = 333;
  std::mt19937_64 g(11);
  std::vector<T> V((size_t)(n * K));
  for (auto &v : V) fill(v, g);
  const std::vector<T> V0 = V;
  std::vector<T> M((size_t)(K * K));
  for (int pass = 0; pass < 2; ++pass) {
    const int kc = nsp_chol_inverse<T>(gram<T>(n, V).data(), LDG, M.data());
    EXPECT(kc == 16, "%s cholesky: kept %d", what, kc);
    for (int64_t j = 0; j < K; ++j)
      for (int64_t c = 0; c < j; ++c) EXPECT(M[(size_t)(j * K + c)] == T(0), "%s cholesky: R^{-1} not upper triangular", what);
    rmul<T>(n, V, M);
  }
  const double d = orth_defect<T>(n, V, K);
  EXPECT(d <= 1e-12, "%s cholesky: |Q^H Q - I| = %.3e", what, d);
  // order preserved: q_0 is v_0 normalized
  double n0 = 0.0, d0 = 0.0;
  for (int64_t i = 0; i < n; ++i) n0 += real_(conj_(V0[(size_t)(i * K)]) * V0[(size_t)(i * K)]);
  n0 = std::sqrt(n0);
  for (int64_t i = 0; i < n; ++i) d0 = std::max(d0, abs_(V[(size_t)(i * K)] - V0[(size_t)(i * K)] / n0));
  EXPECT(d0 <= 1e-14, "%s cholesky: q_0 is not v_0 / |v_0| (%.3e)", what, d0);
}

template <class T>
static void check_dropped(const char *what) {
  const int64_t n = 97;
  std::mt19937_64 g(21);
  std::vector<T> V((size_t)(n * K), T(0));
  for (int64_t i = 0; i < n; ++i)
    for (int64_t c = 0; c < 5; ++c) fill(V[(size_t)(i * K + c)], g);
  std::vector<T> M((size_t)(K * K));
  std::vector<double> w((size_t)K);
  const std::vector<T> G = gram<T>(n, V);
  int kept = nsp_chol_inverse<T>(G.data(), LDG, M.data());
  EXPECT(kept == 5, "%s rank-deficient: Cholesky kept %d, expected 5", what, kept);
  EXPECT(all_finite(M), "%s rank-deficient: Cholesky inverse not finite", what);
  for (int64_t j = 0; j < K; ++j)
    for (int64_t c = 5; c < K; ++c) EXPECT(M[(size_t)(j * K + c)] == T(0), "%s rank-deficient: a dropped column is not zero", what);
  kept = nsp_find_rotation<T>(G.data(), LDG, M.data(), w.data());
  EXPECT(kept >= 5 && kept <= 16, "%s rank-deficient: rotation kept %d", what, kept);
  EXPECT(all_finite(M), "%s rank-deficient: rotation not finite", what);
  for (int64_t c = 0; c < 5; ++c) EXPECT(w[(size_t)c] > 1.0, "%s rank-deficient: eigenvalue %lld = %.3e", what, (long long)c, w[(size_t)c]);
  for (int64_t c = kept; c < K; ++c)
    for (int64_t j = 0; j < K; ++j) EXPECT(M[(size_t)(j * K + c)] == T(0), "%s rank-deficient: a dropped rotation column is not zero", what);
  // nothing at all, and not a number
  std::vector<T> Z((size_t)(K * LDG), T(0));
  EXPECT(nsp_find_rotation<T>(Z.data(), LDG, M.data(), w.data()) == 0, "%s zero: rotation kept something", what);
  EXPECT(nsp_chol_inverse<T>(Z.data(), LDG, M.data()) == 0, "%s zero: Cholesky kept something", what);
  std::vector<T> N = G;
  N[(size_t)(3 * LDG + 2)] = T(std::numeric_limits<double>::quiet_NaN());
  EXPECT(!nsp_gram_finite<T>(N.data(), LDG), "%s NaN: reported finite", what);
  EXPECT(nsp_find_rotation<T>(N.data(), LDG, M.data(), w.data()) == 0, "%s NaN: rotation kept something", what);
  EXPECT(all_finite(M), "%s NaN: rotation output not finite", what);
  EXPECT(nsp_chol_inverse<T>(N.data(), LDG, M.data()) == 0, "%s NaN: Cholesky kept something", what);
  EXPECT(all_finite(M), "%s NaN: Cholesky output not finite", what);
  N = G;
  N[0] = T(std::numeric_limits<double>::infinity());
  EXPECT(nsp_find_rotation<T>(N.data(), LDG, M.data(), w.data()) == 0, "%s Inf: rotation kept something", what);
  EXPECT(nsp_chol_inverse<T>(N.data(), LDG, M.data()) == 0, "%s Inf: Cholesky kept something", what);
  // a negative diagonal entry behind two good columns: Cholesky keeps the two
  N = gram<T>(n, random_orthonormal<T>(n, 31));
  N[(size_t)(2 * LDG + 2)] = T(-1.0);
  EXPECT(nsp_chol_inverse<T>(N.data(), LDG, M.data()) == 2, "%s negative pivot: not dropped from column 2 on", what);
}

// probe blocks for the numpy restatement: per seed int64 n, then the real block [n][16] and the complex block [n][16]
static const uint64_t kSeeds[] = {0ull, 1ull, 0x123456789ABCDEFull, 0xFFFFFFFFFFFFFFFFull};
static int write_probes(const char *path) {
  std::FILE *f = std::fopen(path, "wb");
  if (!f) return 1;
  const int64_t n = 1000, ld = 19;
  for (uint64_t seed : kSeeds) {
    std::vector<double> R((size_t)(n * ld), 777.0);
    std::vector<zdouble> Z((size_t)(n * ld), zdouble(777.0));
    nsp_probe_fill<double>(n, seed, R.data(), ld);
    nsp_probe_fill<zdouble>(n, seed, Z.data(), ld);
    std::fwrite(&n, sizeof(n), 1, f);
    for (int64_t i = 0; i < n; ++i) std::fwrite(&R[(size_t)(i * ld)], sizeof(double), (size_t)K, f);
    for (int64_t i = 0; i < n; ++i) std::fwrite(&Z[(size_t)(i * ld)], sizeof(zdouble), (size_t)K, f);
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j = K; j < ld; ++j)
        EXPECT(R[(size_t)(i * ld + j)] == 777.0 && Z[(size_t)(i * ld + j)] == zdouble(777.0), "probe fill wrote into the stride gap");
  }
  std::fclose(f);
  return 0;
}

int main(int argc, char **argv) {
  check_graded<double>("real");
  check_graded<zdouble>("complex");
  check_cholesky<double>("real");
  check_cholesky<zdouble>("complex");
  check_dropped<double>("real");
  check_dropped<zdouble>("complex");
  for (uint64_t c = 1; c < 100000; c += 7) {
    const double v = nsp_probe_value(42, c);
    if (!(v >= -1.0 && v < 1.0)) EXPECT(false, "probe value %.17g out of [-1, 1)", v);
  }
  if (argc > 1 && write_probes(argv[1])) EXPECT(false, "cannot write %s", argv[1]);
  if (g_fail) {
    std::fprintf(stderr, "%d failure(s)\n", g_fail);
    return 1;
  }
  std::fprintf(stderr, "nsp_find_test -> ok\n");
  return 0;
}
