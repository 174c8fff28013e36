// Host orthonormalization of the basis null-space filter (hifir_amd/csrc/import.hpp nsp_orthonormalize -- the very
// code engine.hip compiles for hifamd_set_nsp_basis), driven directly so that it runs under -fsanitize=address,undefined:
//   * Q^H Q = I to 1e-12 for k = 1, 3, 16, real and complex, row strides ldv > k, padded sizes included;
//   * span(Q) = span(V): V - Q (Q^H V) vanishes to 1e-12 of |V|, and Q has k orthonormal columns;
//   * the padding columns are exactly zero;
//   * a duplicated vector, a zero vector, a NaN and an Inf are refused with kBadPrec, the message naming the index;
//   * k = 0, k = 17, ldv < k and a NULL array are refused with kMismatchedSizes.
// Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I hifir_amd/csrc tests/cpp/nsp_basis_test.cpp
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

static void fill(double &v, std::mt19937_64 &g) { v = std::uniform_real_distribution<double>(-1, 1)(g); }
static void fill(zdouble &v, std::mt19937_64 &g) {
  std::uniform_real_distribution<double> u(-1, 1);
  v = zdouble(u(g), u(g));
}

template <class T>
static std::vector<T> random_block(int64_t n, int64_t k, int64_t ldv, unsigned seed) {
  std::mt19937_64 g(seed);
  std::vector<T> V((size_t)(n * ldv), T(777.0));  // (the stride gap holds a value that must never be read as data)
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < k; ++j) fill(V[(size_t)(i * ldv + j)], g);
  return V;
}

template <class T>
static void check_orthonormal(int64_t n, int64_t k, int64_t ldv, const char *what) {
  const std::vector<T> V = random_block<T>(n, k, ldv, (unsigned)(17 * k + ldv));
  const int64_t kp = nsp_padded(k);
  EXPECT(kp >= k && kp <= 16 && (kp & (kp - 1)) == 0, "%s: padded size %lld", what, (long long)kp);
  const std::vector<T> Q = nsp_orthonormalize<T>(n, k, V.data(), ldv, kp);
  EXPECT((int64_t)Q.size() == n * kp, "%s: size", what);
  double worst = 0.0;
  for (int64_t a = 0; a < kp; ++a)
    for (int64_t b = 0; b < kp; ++b) {
      T h = T(0);
      for (int64_t i = 0; i < n; ++i) h += conj_(Q[(size_t)(i * kp + a)]) * Q[(size_t)(i * kp + b)];
      const double want = (a == b && a < k) ? 1.0 : 0.0;
      worst = std::max(worst, abs_(h - T(want)));
    }
  EXPECT(worst <= 1e-12, "%s k=%lld: |Q^H Q - I| = %.3e", what, (long long)k, worst);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = k; j < kp; ++j) EXPECT(Q[(size_t)(i * kp + j)] == T(0), "%s: padding column not zero", what);
  // span(V) inside span(Q): the residual of every v_j after the projection
  double res = 0.0, vmax = 0.0;
  for (int64_t j = 0; j < k; ++j) {
    std::vector<T> r((size_t)n);
    for (int64_t i = 0; i < n; ++i) r[(size_t)i] = V[(size_t)(i * ldv + j)];
    for (int64_t a = 0; a < k; ++a) {
      T h = T(0);
      for (int64_t i = 0; i < n; ++i) h += conj_(Q[(size_t)(i * kp + a)]) * V[(size_t)(i * ldv + j)];
      for (int64_t i = 0; i < n; ++i) r[(size_t)i] -= h * Q[(size_t)(i * kp + a)];
    }
    for (int64_t i = 0; i < n; ++i) {
      res = std::max(res, abs_(r[(size_t)i]));
      vmax = std::max(vmax, abs_(V[(size_t)(i * ldv + j)]));
    }
  }
  EXPECT(res <= 1e-12 * vmax, "%s k=%lld: |V - Q Q^H V| = %.3e", what, (long long)k, res / vmax);
  // the caller's order: q_0 is v_0 normalized
  double n0 = 0.0;
  for (int64_t i = 0; i < n; ++i) n0 += real_(conj_(V[(size_t)(i * ldv)]) * V[(size_t)(i * ldv)]);
  n0 = std::sqrt(n0);
  double d0 = 0.0;
  for (int64_t i = 0; i < n; ++i) d0 = std::max(d0, abs_(Q[(size_t)(i * kp)] - V[(size_t)(i * ldv)] / n0));
  EXPECT(d0 <= 1e-14, "%s: q_0 is not v_0 / |v_0| (%.3e)", what, d0);
}

template <class T, class F>
static void expect_refused(int code, const char *needle, const char *what, F &&f) {
  try {
    f();
    EXPECT(false, "%s: accepted", what);
  } catch (const Error &e) {
    EXPECT(e.code == code, "%s: code %d, expected %d (%s)", what, e.code, code, e.what());
    EXPECT(std::string(e.what()).find(needle) != std::string::npos, "%s: message '%s' does not name '%s'", what, e.what(), needle);
  }
}

template <class T>
static void check_refusals(const char *what) {
  const int64_t n = 101, k = 5, ldv = 7;
  const std::vector<T> V0 = random_block<T>(n, k, ldv, 99);
  {  // vector 3 := vector 1 (a duplicate), then := v_0 + 2 v_2 (a combination)
    std::vector<T> V = V0;
    for (int64_t i = 0; i < n; ++i) V[(size_t)(i * ldv + 3)] = V[(size_t)(i * ldv + 1)];
    expect_refused<T>(kBadPrec, "vector 3", what, [&] { nsp_orthonormalize<T>(n, k, V.data(), ldv, 8); });
    for (int64_t i = 0; i < n; ++i) V[(size_t)(i * ldv + 3)] = V[(size_t)(i * ldv)] + T(2.0) * V[(size_t)(i * ldv + 2)];
    expect_refused<T>(kBadPrec, "vector 3", what, [&] { nsp_orthonormalize<T>(n, k, V.data(), ldv, 8); });
  }
  {  // a zero vector
    std::vector<T> V = V0;
    for (int64_t i = 0; i < n; ++i) V[(size_t)(i * ldv + 2)] = T(0);
    expect_refused<T>(kBadPrec, "vector 2", what, [&] { nsp_orthonormalize<T>(n, k, V.data(), ldv, 8); });
  }
  {  // not finite
    std::vector<T> V = V0;
    V[(size_t)(40 * ldv + 4)] = T(std::numeric_limits<double>::quiet_NaN());
    expect_refused<T>(kBadPrec, "vector 4", what, [&] { nsp_orthonormalize<T>(n, k, V.data(), ldv, 8); });
    V = V0;
    V[(size_t)(7 * ldv + 0)] = T(std::numeric_limits<double>::infinity());
    expect_refused<T>(kBadPrec, "vector 0", what, [&] { nsp_orthonormalize<T>(n, k, V.data(), ldv, 8); });
  }
  // a nearly dependent vector ABOVE the threshold eps^(2/3) ~ 3.7e-11 is accepted: v_1 = v_0 + 1e-8 w
  {
    std::vector<T> V = V0;
    for (int64_t i = 0; i < n; ++i) V[(size_t)(i * ldv + 1)] = V[(size_t)(i * ldv)] + T(1e-8) * V0[(size_t)(i * ldv + 1)];
    try {
      nsp_orthonormalize<T>(n, 2, V.data(), ldv, 2);
    } catch (const Error &e) {
      EXPECT(false, "%s: a vector at 1e-8 from dependence was refused: %s", what, e.what());
    }
    for (int64_t i = 0; i < n; ++i) V[(size_t)(i * ldv + 1)] = V[(size_t)(i * ldv)] + T(1e-13) * V0[(size_t)(i * ldv + 1)];
    expect_refused<T>(kBadPrec, "vector 1", what, [&] { nsp_orthonormalize<T>(n, 2, V.data(), ldv, 2); });
  }
  expect_refused<T>(kMismatchedSizes, "", what, [&] { nsp_orthonormalize<T>(n, 0, V0.data(), ldv, 1); });
  expect_refused<T>(kMismatchedSizes, "", what, [&] { nsp_orthonormalize<T>(n, 17, V0.data(), 17, 32); });
  expect_refused<T>(kMismatchedSizes, "", what, [&] { nsp_orthonormalize<T>(n, k, V0.data(), k - 1, 8); });
  expect_refused<T>(kMismatchedSizes, "", what, [&] { nsp_orthonormalize<T>(n, k, (const T *)nullptr, ldv, 8); });
}

int main() {
  for (int64_t k : {1, 3, 16}) {
    check_orthonormal<double>(257, k, k + 3, "real");
    check_orthonormal<zdouble>(257, k, k + 2, "complex");
    check_orthonormal<double>(1000, k, k + 1, "real");
  }
  check_orthonormal<double>(16, 16, 17, "real square");  // k = n: Q is unitary
  check_refusals<double>("real");
  check_refusals<zdouble>("complex");
  if (g_fail) {
    std::fprintf(stderr, "%d failure(s)\n", g_fail);
    return 1;
  }
  std::fprintf(stderr, "nsp_basis_test -> ok\n");
  return 0;
}
