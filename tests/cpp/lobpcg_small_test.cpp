// Host driver of hifir_amd/csrc/lobpcg_small.hpp, the small-matrix arithmetic k_lob_small runs in one workgroup: built with
// g++ and the address / undefined sanitizers by tests/test_lobpcg_small_host.py, which writes the cases and compares what
// this program prints with numpy.
//
//   lobpcg_small_test CASES
// CASES (text), four kinds of case, every value as `re im`, matrices row by row:
//   eig name r complex          then r * r values: a Hermitian matrix H.  Prints
//       eig name sweeps | theta (r, ascending) | V (r x r, columns in the order of theta)
//   rr name s k deftol complex  then s * s values of GB and s * s values of GA.  Prints
//       rr name r bad sweeps | piv ... | lam (k) | C (s x k) | Cp (s x k)
//   start name k deftol complex then k * k values of GB = X0^H X0.  Prints (lob::start_factor)
//       start name running verdict | E (k x k)
//   test name k nev step maxit tol anorm nb   then nb * 16 partial sums of |r_j|^2.  Prints (lob::residual_test, from a
//       running tile whose columns are all active)
//       test name running | res (k) | active (k) | flag (k) | iter (k)
// The team is the team of one: what the kernel must reproduce bit for bit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "lobpcg_small.hpp"

namespace bcg = hifamd::bcg;
namespace lob = hifamd::lob;
struct Z {
  double x, y;
};
// (the dynamic LDS of k_lob_small, real and complex: two matrices, jac.s, d | dsc | jac.c, piv | taken | perm | mate, count)
static_assert(lob::RitzScratch<double>::bytes() == 2 * 32768 + 512 + 3 * 512 + 4 * 256 + 16, "k_lob_small's LDS, real");
static_assert(lob::RitzScratch<Z>::bytes() == 2 * 65536 + 1024 + 3 * 512 + 4 * 256 + 16, "k_lob_small's LDS, complex");
static void put(double a) { std::printf(" %.17g 0", a); }
static void put(const Z &a) { std::printf(" %.17g %.17g", a.x, a.y); }
static void make(double &a, double re, double) { a = re; }
static void make(Z &a, double re, double im) { a = Z{re, im}; }

template <class T>
static bool read_matrix(std::FILE *f, int m, std::vector<T> &M) {
  const int L = bcg::kLd;
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) {
      char sre[64], sim[64];
      if (std::fscanf(f, "%63s %63s", sre, sim) != 2) return false;
      make(M[i * L + j], std::strtod(sre, nullptr), std::strtod(sim, nullptr));
    }
  return true;
}

template <class T>
struct Work {
  static constexpr int L = bcg::kLd;
  std::vector<T> W1, W2, X1, X2, X3, s;
  std::vector<double> d, dsc, c;
  std::vector<int> piv, taken, perm, mate, count;
  Work() : W1(L * L), W2(L * L), X1(L * L), X2(L * L), X3(L * L), s(L), d(L), dsc(L), c(L), piv(L, -1), taken(L), perm(L), mate(L), count(1) {}
  lob::JacobiScratch<T> jac() { return lob::JacobiScratch<T>{mate.data(), c.data(), s.data(), count.data()}; }
  lob::RitzScratch<T> ritz() {
    return lob::RitzScratch<T>{W1.data(), W2.data(), X1.data(), X2.data(), X3.data(), d.data(), dsc.data(), piv.data(), taken.data(), perm.data(), jac()};
  }
};

template <class T>
static int eig_case(const std::string &name, int r, std::FILE *f) {
  const int L = bcg::kLd;
  std::vector<T> H(L * L), V(L * L);
  if (!read_matrix(f, r, H)) return 1;
  Work<T> w;
  const bcg::Serial tm;
  lob::identity(V.data(), r, tm);
  const int sweeps = lob::jacobi(H.data(), V.data(), r, w.jac(), tm);
  for (int i = 0; i < r; ++i) w.d[i] = bcg::re(H[i * L + i]);
  lob::order_ascending(w.d.data(), r, w.perm.data(), tm);
  std::printf("eig %s %d |", name.c_str(), sweeps);
  for (int j = 0; j < r; ++j) std::printf(" %.17g", w.d[w.perm[j]]);
  std::printf(" |");
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < r; ++j) put(V[i * L + w.perm[j]]);
  std::printf("\n");
  return 0;
}

template <class T>
static int rr_case(const std::string &name, int s, int k, double deftol, std::FILE *f) {
  const int L = bcg::kLd;
  std::vector<T> GB(L * L), GA(L * L), CC(L * L);
  std::vector<double> lam(L, 0.0);
  if (!read_matrix(f, s, GB) || !read_matrix(f, s, GA)) return 1;
  Work<T> w;
  const bcg::Serial tm;
  const lob::Ritz out = lob::rayleigh_ritz(GB.data(), GA.data(), s, k, deftol, true, w.ritz(), CC.data(), lam.data(), tm);
  std::printf("rr %s %d %d %d |", name.c_str(), out.r, out.bad ? 1 : 0, out.sweeps);
  for (int i = 0; i < out.f.r; ++i) std::printf(" %d", w.piv[i]);
  std::printf(" |");
  if (!out.bad)
    for (int j = 0; j < k; ++j) std::printf(" %.17g", lam[j]);
  for (int part = 0; part < 2; ++part) {
    std::printf(" |");
    if (!out.bad)
      for (int i = 0; i < s; ++i)
        for (int j = 0; j < k; ++j) put(CC[i * L + lob::kMaxK * part + j]);
  }
  std::printf("\n");
  return 0;
}

template <class T>
struct Tile {  // a tile's state on the host
  static constexpr int L = bcg::kLd;
  std::vector<T> GB, GA, CC;
  std::vector<double> lam, res;
  std::vector<int> flag, iter, active, ctl;
  Tile() : GB(L * L), GA(L * L), CC(L * L), lam(L), res(L), flag(L, -1), iter(L, -1), active(L, 1), ctl(4, 0) {}
  lob::Small<T> small(int k, int nev, double tol, double deftol, double anorm, int maxit) {
    return lob::Small<T>{GB.data(), GA.data(), CC.data(), lam.data(), res.data(), flag.data(), iter.data(), active.data(), ctl.data(),
                         tol, deftol, anorm, maxit, k, nev};
  }
};

template <class T>
static int start_case(const std::string &name, int k, double deftol, std::FILE *f) {
  const int L = bcg::kLd;
  Tile<T> t;
  if (!read_matrix(f, k, t.GB)) return 1;
  Work<T> w;
  lob::start_factor(t.small(k, k, 1e-8, deftol, 1.0, 10), w.ritz(), bcg::Serial());
  std::printf("start %s %d %d |", name.c_str(), t.ctl[0], t.ctl[3]);
  if (t.ctl[0])
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j) put(t.CC[i * L + j]);
  std::printf("\n");
  return 0;
}

static int test_case(const std::string &name, std::FILE *f) {
  int k, nev, step, maxit, nb;
  double tol, anorm;
  if (std::fscanf(f, "%d %d %d %d %lf %lf %d", &k, &nev, &step, &maxit, &tol, &anorm, &nb) != 7 || k < 1 || k > lob::kMaxK || nb < 1) return 1;
  std::vector<double> partial((size_t)nb * lob::kMaxK);
  for (double &v : partial) {
    char word[64];
    if (std::fscanf(f, "%63s", word) != 1) return 1;
    v = std::strtod(word, nullptr);
  }
  Tile<double> t;
  t.ctl[0] = 1;
  lob::residual_test(t.small(k, nev, tol, 1e-12, anorm, maxit), partial.data(), nb, step, bcg::Serial());
  std::printf("test %s %d |", name.c_str(), t.ctl[0]);
  for (int c = 0; c < k; ++c) std::printf(" %.17g", t.res[c]);
  for (const std::vector<int> *v : {&t.active, &t.flag, &t.iter}) {
    std::printf(" |");
    for (int c = 0; c < k; ++c) std::printf(" %d", (*v)[c]);
  }
  std::printf("\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char kind[16], name[64];
  int cases = 0;
  while (std::fscanf(f, "%15s %63s", kind, name) == 2) {
    int s, k = 0, cplx;
    double deftol = 0.0;
    if (std::string(kind) == "eig") {
      if (std::fscanf(f, "%d %d", &s, &cplx) != 2 || s < 1 || s > lob::kMaxS) return 3;
      if (cplx ? eig_case<Z>(name, s, f) : eig_case<double>(name, s, f)) return 4;
    } else if (std::string(kind) == "rr") {
      if (std::fscanf(f, "%d %d %lf %d", &s, &k, &deftol, &cplx) != 4 || s < 1 || s > lob::kMaxS || k < 1 || k > lob::kMaxK) return 3;
      if (cplx ? rr_case<Z>(name, s, k, deftol, f) : rr_case<double>(name, s, k, deftol, f)) return 4;
    } else if (std::string(kind) == "start") {
      if (std::fscanf(f, "%d %lf %d", &k, &deftol, &cplx) != 3 || k < 1 || k > lob::kMaxK) return 3;
      if (cplx ? start_case<Z>(name, k, deftol, f) : start_case<double>(name, k, deftol, f)) return 4;
    } else if (std::string(kind) == "test") {
      if (test_case(name, f)) return 4;
    } else {
      return 3;
    }
    ++cases;
  }
  std::fclose(f);
  std::printf("cases %d OK\n", cases);
  return 0;
}
