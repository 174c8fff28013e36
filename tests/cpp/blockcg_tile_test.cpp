// Host driver of the decisions of the block CG driver in hifir_amd/csrc/blockcg_small.hpp (what k_bcg_beta and k_bcg_small
// run: bcg::start_columns and the four modes) with a team of one: built with g++ and the address / undefined sanitizers by
// tests/test_blockcg_small_host.py, which writes the cases and compares what this program prints with numpy.
//
//   blockcg_tile_test CASES
// CASES (text): per case a line `name s complex rtol deftol maxit nops`, then nops operations `kind k` followed by their
// values, replayed on ONE state (C, the ranks and the residual ratios carry over as in a tile):
//   0 0 : s values |b_j|^2                          -> bcg::start_columns
//   1 0 : s x s Gram (re im, row by row)            -> bcg::start_factor
//   2 k : s x s Gram (zero outside its block)       -> bcg::step_alpha
//   3 k : s x s Gram                                -> bcg::step_test
//   4 k : s x s Gram                                -> bcg::step_next
// After each operation it prints
//   op name index ctl0 ctl1 ctl2 ctl3 | flags | iters | active | bnorm | relres | E1 | E2 | C | pad
// with the s x s leading blocks of the three matrices (re im) and pad = the largest magnitude outside those blocks.
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

static bool number(std::FILE *f, double &v) {
  char s[64];
  if (std::fscanf(f, "%63s", s) != 1) return false;
  v = std::strtod(s, nullptr);  // (inf and nan as text)
  return true;
}

// (the dynamic LDS of k_bcg_small and k_bgcr_small, real and complex)
static_assert(bcg::Work<double>::bytes() == 66560 && bcg::Work<Z>::bytes() == 132096, "the small kernels' dynamic LDS");

template <class T>
static int run_case(const std::string &name, int s, double rtol, double deftol, int maxit, int nops, std::FILE *f) {
  const int L = bcg::kLd;
  std::vector<T> C(L * L), E1(L * L), E2(L * L), G(L * L);
  std::vector<double> bnorm(L), relres(L), b2(L);
  std::vector<double> lds(bcg::Work<T>::bytes() / sizeof(double));  // carved as the kernels carve their LDS: a step past its end is seen
  std::vector<int> iter(L, -1), flag(L, -1), active(L, -1), ctl(4, 0);
  const bcg::Small<T> S{{bnorm.data(), iter.data(), flag.data(), active.data(), ctl.data(), maxit, rtol},
                        C.data(), E1.data(), E2.data(), G.data(), relres.data(), deftol};
  const bcg::Work<T> W = bcg::Work<T>::carve(lds.data());
  const bcg::Serial tm;
  for (int op = 0; op < nops; ++op) {
    int kind, k;
    if (std::fscanf(f, "%d %d", &kind, &k) != 2) return 1;
    if (kind == 0) {
      for (int c = 0; c < s; ++c)
        if (!number(f, b2[c])) return 1;
      bcg::start_columns(S, s, b2.data(), tm);
    } else {
      for (int i = 0; i < s; ++i)
        for (int j = 0; j < s; ++j) {
          double re, im;
          if (!number(f, re) || !number(f, im)) return 1;
          make(G[i * L + j], re, im);
        }
      if (kind == 1) bcg::start_factor(S, W, s, tm);
      if (kind == 2) bcg::step_alpha(S, W, s, k, tm);
      if (kind == 3) bcg::step_test(S, W, s, k, tm);
      if (kind == 4) bcg::step_next(S, W, s, k, tm);
    }
    std::printf("op %s %d %d %d %d %d |", name.c_str(), op, ctl[0], ctl[1], ctl[2], ctl[3]);
    for (const std::vector<int> *v : {&flag, &iter, &active}) {
      for (int c = 0; c < s; ++c) std::printf(" %d", (*v)[c]);
      std::printf(" |");
    }
    for (int c = 0; c < s; ++c) std::printf(" %.17g", bnorm[c]);
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
    if (s < 1 || s > bcg::kLd || nops < 0) return 3;
    if (cplx ? run_case<Z>(name, s, rtol, deftol, maxit, nops, f) : run_case<double>(name, s, rtol, deftol, maxit, nops, f)) return 4;
    ++cases;
  }
  std::fclose(f);
  std::printf("cases %d OK\n", cases);
  return 0;
}
