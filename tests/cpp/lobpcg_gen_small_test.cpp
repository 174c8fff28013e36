// tests/cpp/lobpcg_gen_small_test.cpp -- TEST (compiled with g++ -fsanitize=address,undefined and run by
// tests/test_lobpcg_gen_host.py; no GPU, no input file).
//
// lob::residual_test_gen of hifir_amd/csrc/lobpcg_small.hpp, the stopping test of the generalized LOBPCG driver, with the team
// of one -- what k_lob_small's mode 2 must reproduce bit for bit -- on hand-made partials [nb][32] (|r_j|^2 at j, |x_j|^2 at 16 + j).
// Every expectation is computed here: res_j = sqrt(sum r) / ((anorm + |lambda_j| bnorm) sqrt(sum x)) with the sums in block
// order, active_j = !(res_j <= tol), and the tile's end (flags 0 / 2, iter = step, ctl[0] = 0) when every j < nev is
// converged or step == maxit.  Exit code 0 and "GEN SMALL TEST OK" = every check holds.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "lobpcg_small.hpp"

namespace bcg = hifamd::bcg;
namespace lob = hifamd::lob;

namespace {

int failures = 0;
void check(const char *name, const char *what, bool ok) {
  if (!ok) std::printf("%s: %s FAIL\n", name, what), ++failures;
}

struct Tile {
  std::vector<double> lam, res;
  std::vector<int> flag, iter, active, ctl;
  Tile() : lam(64, 0.0), res(64, -1.0), flag(64, -1), iter(64, -1), active(64, 1), ctl(4, 0) { ctl[0] = 1; }
  lob::Small<double> small(int k, int nev, double tol, double anorm, double bnorm, int maxit) {
    lob::Small<double> S{nullptr, nullptr, nullptr, lam.data(), res.data(), flag.data(), iter.data(), active.data(), ctl.data(),
                         tol, 1e-12, anorm, maxit, k, nev};
    S.bnorm = bnorm;
    return S;
  }
};

bool same(double a, double b) { return (a != a && b != b) || a == b; }

// runs one case and checks it against the expectation computed here; ends: whether the tile must be over afterwards
void run(const char *name, int k, int nev, int step, int maxit, double tol, double anorm, double bnorm, const std::vector<double> &lam,
         const std::vector<double> &partial, int nb, bool ends) {
  Tile t;
  for (int c = 0; c < k; ++c) t.lam[(size_t)c] = lam[(size_t)c];
  lob::residual_test_gen(t.small(k, nev, tol, anorm, bnorm, maxit), partial.data(), nb, step, bcg::Serial());
  bool all = true;
  std::vector<int> act((size_t)k);
  for (int c = 0; c < k; ++c) {
    double rr = partial[(size_t)c], xx = partial[16 + (size_t)c];
    for (int b = 1; b < nb; ++b) rr += partial[(size_t)(32 * b + c)], xx += partial[(size_t)(32 * b + 16 + c)];
    const double scale = (anorm + std::fabs(lam[(size_t)c]) * bnorm) * std::sqrt(xx);
    double want = scale == 0.0 ? std::sqrt(rr) : std::sqrt(rr) / scale;
    if (scale > std::numeric_limits<double>::max()) want = HUGE_VAL;
    act[(size_t)c] = want <= tol ? 0 : 1;
    if (c < nev) all = all && act[(size_t)c] == 0;
    check(name, "res_j", same(t.res[(size_t)c], want));
    check(name, "active_j", t.active[(size_t)c] == act[(size_t)c]);
  }
  const bool over = all || step >= maxit;
  check(name, "the expected end", over == ends);
  check(name, "ctl[0]", t.ctl[0] == (over ? 0 : 1));
  for (int c = 0; c < k; ++c) {
    check(name, "flag_j", t.flag[(size_t)c] == (over ? (act[(size_t)c] ? 2 : 0) : -1));
    check(name, "iter_j", t.iter[(size_t)c] == (over ? step : -1));
  }
  for (int c = k; c < 64; ++c)
    check(name, "columns >= k untouched", t.res[(size_t)c] == -1.0 && t.flag[(size_t)c] == -1 && t.active[(size_t)c] == 1);
}

// nb blocks of partials: |r_j|^2 = r2[j] and |x_j|^2 = x2[j] in total, dealt unevenly over the blocks
std::vector<double> deal(int nb, int k, const std::vector<double> &r2, const std::vector<double> &x2) {
  std::vector<double> p((size_t)nb * 32, 0.0);
  double wsum = 0.0;
  for (int b = 0; b < nb; ++b) wsum += 1.0 + 0.37 * b;
  for (int b = 0; b < nb; ++b)
    for (int c = 0; c < k; ++c) {
      const double w = (1.0 + 0.37 * b) / wsum;
      p[(size_t)(32 * b + c)] = r2[(size_t)c] * w, p[(size_t)(32 * b + 16 + c)] = x2[(size_t)c] * w;
    }
  return p;
}

}  // namespace

int main() {
  const double tol = 1e-9, anorm = 8.0, bnorm = 0.5;
  const std::vector<double> lam = {0.5, -2.0, 3.0, 4.0, 100.0};
  const std::vector<double> x2 = {4.0, 9.0, 0.25, 1.0, 16.0};
  // scale_j = (8 + |lam_j| / 2) sqrt(x2_j); residuals of 1e-6 are far from converged, of 1e-12 converged
  const std::vector<double> far = {1e-12, 1e-12, 1e-12, 1e-12, 1e-12}, near = {1e-24, 1e-24, 1e-24, 1e-12, 1e-12};
  run("none_converged", 5, 5, 3, 10, tol, anorm, bnorm, lam, deal(7, 5, far, x2), 7, false);
  run("at_maxit", 5, 5, 10, 10, tol, anorm, bnorm, lam, deal(7, 5, far, x2), 7, true);
  run("wanted_converged_guards_not", 5, 3, 4, 10, tol, anorm, bnorm, lam, deal(7, 5, near, x2), 7, true);
  run("a_wanted_column_not_converged", 5, 4, 4, 10, tol, anorm, bnorm, lam, deal(7, 5, near, x2), 7, false);
  run("one_block", 5, 3, 0, 10, tol, anorm, bnorm, lam, deal(1, 5, near, x2), 1, true);
  // the scale follows |lambda| ||B||: the same residual converges under a large |lambda_j| and not under a small one
  {
    const std::vector<double> l2 = {1e-3, 1e6}, r2 = {1e-16, 1e-16}, one = {1.0, 1.0};
    run("scale_follows_lambda", 2, 2, 1, 10, tol, anorm, bnorm, l2, deal(3, 2, r2, one), 3, false);
    Tile t;
    t.lam[0] = l2[0], t.lam[1] = l2[1];
    const std::vector<double> p = deal(3, 2, r2, one);
    lob::residual_test_gen(t.small(2, 2, tol, anorm, bnorm, 10), p.data(), 3, 1, bcg::Serial());
    check("scale_follows_lambda", "column 0 active, column 1 not", t.active[0] == 1 && t.active[1] == 0);
  }
  // a zero ||x_j||: the scale is exactly zero and res_j = ||r_j||; with a zero residual too the column counts as converged
  {
    const std::vector<double> r2 = {1e-30, 0.0, 1e-6}, z2 = {0.0, 0.0, 0.0};
    run("zero_x", 3, 3, 2, 10, tol, anorm, bnorm, lam, deal(4, 3, r2, z2), 4, false);
    run("zero_x_wanted_two", 3, 2, 2, 10, tol, anorm, bnorm, lam, deal(4, 3, r2, z2), 4, true);
    run("both_norms_zero", 2, 2, 0, 10, tol, 0.0, 0.0, lam, deal(2, 2, std::vector<double>{0.0, 1e-30}, std::vector<double>{1.0, 1.0}), 2, true);
  }
  // a partial that is not finite: res_j is NaN (or HUGE_VAL for an infinite scale), the column stays active, flag 2 at maxit
  {
    std::vector<double> p = deal(5, 3, near, x2);
    p[32 * 2 + 1] = std::nan("");
    run("nan_r_partial", 3, 3, 4, 10, tol, anorm, bnorm, lam, p, 5, false);
    run("nan_r_partial_at_maxit", 3, 3, 10, 10, tol, anorm, bnorm, lam, p, 5, true);
    std::vector<double> q = deal(5, 3, near, x2);
    q[32 * 3 + 16 + 0] = std::nan("");
    run("nan_x_partial", 3, 3, 4, 10, tol, anorm, bnorm, lam, q, 5, false);
    std::vector<double> w = deal(5, 3, near, x2);
    w[32 * 1 + 16 + 2] = HUGE_VAL;
    run("inf_x_partial", 3, 3, 4, 10, tol, anorm, bnorm, lam, w, 5, false);
    Tile t;
    for (int c = 0; c < 3; ++c) t.lam[(size_t)c] = lam[(size_t)c];
    lob::residual_test_gen(t.small(3, 3, tol, anorm, bnorm, 10), w.data(), 5, 4, bcg::Serial());
    check("inf_x_partial", "an infinite scale is not convergence", t.active[2] == 1 && t.res[2] == HUGE_VAL);
  }
  // a tile that is over is left alone
  {
    Tile t;
    t.ctl[0] = 0;
    const std::vector<double> p = deal(2, 5, near, x2);
    lob::residual_test_gen(t.small(5, 5, tol, anorm, bnorm, 10), p.data(), 2, 3, bcg::Serial());
    check("over", "nothing written", t.res[0] == -1.0 && t.flag[0] == -1 && t.iter[0] == -1 && t.active[0] == 1 && t.ctl[0] == 0);
  }
  // k = 16: every column of the partial rows
  {
    std::vector<double> l16(16), r16(16), x16(16);
    for (int c = 0; c < 16; ++c) l16[(size_t)c] = 0.25 * c, r16[(size_t)c] = c < 13 ? 1e-26 : 1e-10, x16[(size_t)c] = 1.0 + c;
    run("k16_nev13", 16, 13, 6, 10, tol, anorm, bnorm, l16, deal(9, 16, r16, x16), 9, true);
    run("k16_nev14", 16, 14, 6, 10, tol, anorm, bnorm, l16, deal(9, 16, r16, x16), 9, false);
  }
  if (failures) {
    std::printf("%d checks FAILED\n", failures);
    return 1;
  }
  std::printf("GEN SMALL TEST OK\n");
  return 0;
}
