// Host driver of hifir_amd/csrc/blockcg_small.hpp, the small-matrix arithmetic k_bcg_small runs in one workgroup: built with
// g++ and the address / undefined sanitizers by tests/test_blockcg_small_host.py, which writes the cases and compares what
// this program prints with numpy.
//
//   blockcg_small_test CASES
// CASES (text): per case a line `name m deftol pivoted complex nb`, then nb * m * m values (re im) row by row: the nb
// partial matrices of an m x m Gram.  Per case the program sums the partials in order, makes the sum Hermitian, factors it and
// prints
//   case name r bad kept dropped | piv ... | S (r x m, re im) ... | rec inv sel quad
// rec = max |G[i][j] - (S^H S)[i][j]| over the pivot rows and columns, inv = max |S[:, piv] Ti - I|, sel = max |S E - I| with
// E = I[:, piv] Ti (through select_rows and matmul), quad = max_j |sqrt(c_j^H G c_j) - |S c_j|| for the columns c_j of
// E (through quad_forms, adjoint and matmul); 0 where r = 0 or the factorization broke down.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "blockcg_small.hpp"

namespace bcg = hifamd::bcg;
struct Z {
  double x, y;
};
static double mag(double a) { return std::fabs(a); }
static double mag(const Z &a) { return std::hypot(a.x, a.y); }
static void put(double a) { std::printf(" %.17g 0", a); }
static void put(const Z &a) { std::printf(" %.17g %.17g", a.x, a.y); }
static void make(double &a, double re, double) { a = re; }
static void make(Z &a, double re, double im) { a = Z{re, im}; }

template <class T>
static int run_case(const std::string &name, int m, double deftol, bool pivoted, int nb, std::FILE *f) {
  const int L = bcg::kLd;
  std::vector<T> part((size_t)nb * L * L), G(L * L), H(L * L), S(L * L), Ti(L * L), E(L * L), W(L * L), Wh(L * L);
  for (int b = 0; b < nb; ++b)
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) {
        char sre[64], sim[64];
        if (std::fscanf(f, "%63s %63s", sre, sim) != 2) return 1;
        make(part[(size_t)b * L * L + i * L + j], std::strtod(sre, nullptr), std::strtod(sim, nullptr));
      }
  const bcg::Serial tm;
  std::vector<double> d(L), q(L);
  std::vector<int> piv(L, -1), taken(L);
  bcg::sum_partials(part.data(), nb, m, G.data(), tm);
  bcg::hermitize(G.data(), H.data(), m, tm);
  const bcg::Chol c = bcg::chol(G.data(), m, deftol, pivoted, S.data(), piv.data(), d.data(), taken.data(), tm);
  std::printf("case %s %d %d %.17g %.17g |", name.c_str(), c.r, c.bad ? 1 : 0, c.kept, c.dropped);
  for (int k = 0; k < c.r; ++k) std::printf(" %d", piv[k]);
  std::printf(" |");
  for (int k = 0; k < c.r; ++k)
    for (int j = 0; j < m; ++j) put(S[k * L + j]);
  double rec = 0, inv = 0, sel = 0, quad = 0;
  if (c.r > 0 && !c.bad) {
    const int r = c.r;
    for (int a = 0; a < r; ++a)
      for (int b = 0; b < r; ++b) {
        T acc;
        bcg::set(acc, 0.0);
        for (int k = 0; k < r; ++k) acc = bcg::add(acc, bcg::mul(bcg::cj(S[k * L + piv[a]]), S[k * L + piv[b]]));
        rec = std::fmax(rec, mag(bcg::sub(G[piv[a] * L + piv[b]], acc)));
      }
    bcg::tri_inv(S.data(), piv.data(), r, Ti.data(), tm);
    for (int a = 0; a < r; ++a)
      for (int b = 0; b < r; ++b) {
        T acc;
        bcg::set(acc, a == b ? -1.0 : 0.0);
        for (int k = 0; k < r; ++k) acc = bcg::add(acc, bcg::mul(S[a * L + piv[k]], Ti[k * L + b]));
        inv = std::fmax(inv, mag(acc));
      }
    bcg::select_rows(Ti.data(), piv.data(), r, m, r, E.data(), tm);
    bcg::matmul(S.data(), E.data(), false, r, m, r, (const double *)nullptr, W.data(), tm);  // S E = I
    for (int a = 0; a < r; ++a)
      for (int b = 0; b < r; ++b) sel = std::fmax(sel, mag(bcg::sub(W[a * L + b], T{a == b ? 1.0 : 0.0})));
    // |S c_j| two ways: the quadratic form of G, and the columns of W = S E through adjoint and matmul (W W^H)
    bcg::quad_forms(G.data(), E.data(), m, r, Wh.data(), q.data(), tm);
    bcg::adjoint(W.data(), r, r, Wh.data(), tm);
    bcg::matmul(Wh.data(), Wh.data(), true, r, r, r, (const double *)nullptr, H.data(), tm);  // (W^H)(W^H)^H = W^H W
    for (int j = 0; j < r; ++j) quad = std::fmax(quad, std::fabs(q[j] - std::sqrt(std::fabs(bcg::re(H[j * L + j])))));
  }
  std::printf(" | %.17g %.17g %.17g %.17g\n", rec, inv, sel, quad);
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char name[64];
  int m, pivoted, cplx, nb, cases = 0;
  double deftol;
  while (std::fscanf(f, "%63s %d %lf %d %d %d", name, &m, &deftol, &pivoted, &cplx, &nb) == 6) {
    if (m < 0 || m > bcg::kLd || nb < 1) return 3;
    if (cplx ? run_case<Z>(name, m, deftol, pivoted != 0, nb, f) : run_case<double>(name, m, deftol, pivoted != 0, nb, f)) return 4;
    ++cases;
  }
  std::fclose(f);
  std::printf("cases %d OK\n", cases);
  return 0;
}
