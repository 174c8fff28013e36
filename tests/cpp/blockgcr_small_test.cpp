// Host driver of hifir_amd/csrc/blockgcr_small.hpp, the decisions and small matrices of the restarted block GCR driver
// (k_bgcr_rho, k_bgcr_small) with a team of one: built with g++ and the address / undefined sanitizers by
// tests/test_blockgcr_small_host.py, which writes the cases and compares what this program prints with numpy.
//
//   blockgcr_small_test CASES
// CASES (text): per case a line `name s complex rtol deftol maxit nops`, a line of s norms ||b|| and s active marks, then
// nops operations `kind a b` followed by their values, replayed on ONE state (C, ranks, mu carry over as in a tile):
//   0 cycle steps : s values ||r||^2                       -> bgcr::cycle_start
//   1 first steps : s x s Gram (re im, row by row)         -> bgcr::cycle_factor
//   2 steps 0     : s x s Gram (zero outside its block)    -> bgcr::step_basis
//   3 0 0         : s x s matrix D                         -> bgcr::step_coeff
//   4 steps last  : s x s Gram                             -> bgcr::step_test
// After each operation it prints
//   op name index ctl0 ctl1 ctl2 ctl3 q mu | flags | iters | tres | relres | E1 | E2 | C | pad
// with the s x s leading blocks of the three matrices (re im) and pad = the largest magnitude outside those blocks.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "blockgcr_small.hpp"

namespace bcg = hifamd::bcg;
namespace bgcr = hifamd::bgcr;
struct Z {
  double x, y;
};
static double mag(double a) { return std::fabs(a); }
static double mag(const Z &a) { return std::hypot(a.x, a.y); }
static void put(double a) { std::printf(" %.17g 0", a); }
static void put(const Z &a) { std::printf(" %.17g %.17g", a.x, a.y); }
static void make(double &a, double re, double) { a = re; }
static void make(Z &a, double re, double im) { a = Z{re, im}; }

static bool number(std::FILE *f, double &v) {
  char s[64];
  if (std::fscanf(f, "%63s", s) != 1) return false;
  v = std::strtod(s, nullptr);  // (inf and nan as text)
  return true;
}

template <class T>
static int run_case(const std::string &name, int s, double rtol, double deftol, int maxit, int nops, std::FILE *f) {
  const int L = bgcr::kLd;
  std::vector<T> C(L * L), E1(L * L), E2(L * L), G(L * L), W1(L * L), W2(L * L);
  std::vector<double> bnorm(L), rho(L), tres(L), relres(L), mu(L), d(L);
  std::vector<int> iter(L), flag(L), active(L), live(L), ctl(4), aux(L), piv(L), taken(L);
  for (int c = 0; c < s; ++c)
    if (!number(f, bnorm[c])) return 1;
  for (int c = 0; c < s; ++c)
    if (std::fscanf(f, "%d", &active[c]) != 1) return 1;
  ctl[0] = 1, ctl[3] = s;  // (what k_bcg_beta leaves)
  const bgcr::Small<T> S{{{bnorm.data(), iter.data(), flag.data(), active.data(), ctl.data(), maxit, rtol},
                          C.data(), E1.data(), E2.data(), G.data(), relres.data(), deftol},
                         rho.data(), tres.data(), mu.data(), live.data(), aux.data()};
  const bcg::Work<T> W{W1.data(), W2.data(), d.data(), piv.data(), taken.data()};
  const bcg::Serial tm;
  for (int op = 0; op < nops; ++op) {
    int kind, a, b;
    if (std::fscanf(f, "%d %d %d", &kind, &a, &b) != 3) return 1;
    if (kind == 0) {
      for (int c = 0; c < s; ++c)
        if (!number(f, rho[c])) return 1;
      bgcr::cycle_start(S, s, a, b, tm);
    } else {
      for (int i = 0; i < s; ++i)
        for (int j = 0; j < s; ++j) {
          double re, im;
          if (!number(f, re) || !number(f, im)) return 1;
          make(G[i * L + j], re, im);
        }
      if (kind == 1) bgcr::cycle_factor(S, W, s, a != 0, b, tm);
      if (kind == 2) bgcr::step_basis(S, W, s, a, tm);
      if (kind == 3) bgcr::step_coeff(S, W, s, tm);
      if (kind == 4) bgcr::step_test(S, W, s, a, b != 0, tm);
    }
    std::printf("op %s %d %d %d %d %d %d %.17g |", name.c_str(), op, ctl[0], ctl[1], ctl[2], ctl[3], aux[0], mu[0]);
    for (int c = 0; c < s; ++c) std::printf(" %d", flag[c]);
    std::printf(" |");
    for (int c = 0; c < s; ++c) std::printf(" %d", iter[c]);
    std::printf(" |");
    for (int c = 0; c < s; ++c) std::printf(" %.17g", tres[c]);
    std::printf(" |");
    for (int c = 0; c < s; ++c) std::printf(" %.17g", relres[c]);
    double pad = 0.0;
    for (const std::vector<T> *M : {&E1, &E2, &C}) {
      std::printf(" |");
      for (int i = 0; i < L; ++i)
        for (int j = 0; j < L; ++j) {
          if (i < s && j < s)
            put((*M)[i * L + j]);
          else
            pad = std::fmax(pad, mag((*M)[i * L + j]));
        }
    }
    std::printf(" | %.17g\n", pad);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char name[64];
  int s, cplx, maxit, nops, cases = 0;
  double rtol, deftol;
  while (std::fscanf(f, "%63s %d %d %lf %lf %d %d", name, &s, &cplx, &rtol, &deftol, &maxit, &nops) == 7) {
    if (s < 1 || s > bgcr::kLd || nops < 0) return 3;
    if (cplx ? run_case<Z>(name, s, rtol, deftol, maxit, nops, f) : run_case<double>(name, s, rtol, deftol, maxit, nops, f)) return 4;
    ++cases;
  }
  std::fclose(f);
  std::printf("cases %d OK\n", cases);
  return 0;
}
