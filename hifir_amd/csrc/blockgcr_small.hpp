// The small-matrix arithmetic and every decision of the restarted block GCR driver (Engine::bgcr_tile, k_bgcr_rho and
// k_bgcr_small in kernels.hip.hpp): the tests of a cycle's start on the true residuals, the rank-revealing factorization of
// the residual block, the orthonormalization of a new direction block, the coefficients of the update, the recurrence's
// residual test and the re-factorization of the residual.  Plain C++17, no HIP include: the kernels and host programs built
// with g++ (tests/cpp/blockgcr_small_test.cpp) run the same code, on blockcg_small.hpp's functions and with its Team
// convention (a function is called by every thread of the team and ends with a barrier; a team of one gives the same bits).
#pragma once
#include "blockcg_small.hpp"

namespace hifamd {
namespace bgcr {

using bcg::kLd;

// The small state of a tile of s <= 64 columns: block CG's, and what the cycles add.  relres: the recurrence's rel_j.
//   ctl[0]: 0 the tile is over, 1 inside a cycle, 2 the cycle has ended (the next one starts with a true residual)
//   ctl[1]: rank after the start of the first cycle; ctl[2]: rank of the residual block during the last step
//   ctl[3]: current rank r of the residual block; aux[0]: rank q of the step's direction block
template <class T>
struct Small : bcg::Small<T> {
  double *rho, *tres, *mu;  // [64]: ||r|| at the cycle's start, rho / beta (the last true residual's ratio); mu[0]
  int *live, *aux;          // [64]; live: a block column whose residual is not an exact zero
};

// A cycle's start.  rho[c] holds ||r_c||^2 of the true residual; it becomes ||r_c||, tres[c] = ||r_c|| / ||b_c|| (0 for a
// column outside the block).  All tres <= rtol: flags 0, the tile is over.  steps == maxit: flag 0 / 2.  From the second
// cycle on, mu = max tres not below the last cycle's: flag 0 / 1 (stagnated).  Otherwise the cycle runs (ctl[0] = 1).
template <class T, class Team>
HIFAMD_HD inline void cycle_start(const Small<T> &S, int s, int cycle, int steps, const Team &tm) {
  if (S.ctl[0] == 0) return;
  tm.sync();
  for (int c = tm.rank(); c < s; c += tm.size()) {
    const bool in = S.active[c] != 0;
    const double r = in ? std::sqrt(S.rho[c]) : 0.0;
    S.rho[c] = r;
    S.tres[c] = in ? r / S.bnorm[c] : 0.0;
    S.live[c] = (in && r != 0.0) ? 1 : 0;
    S.relres[c] = S.tres[c];
  }
  tm.sync();
  bool all = true;
  double mu = 0.0;
  for (int c = 0; c < s; ++c) {
    const double t = S.tres[c];
    all = all && t <= S.rtol;
    if (mu == mu && (t != t || t > mu)) mu = t;  // (a NaN stays)
  }
  const double mu_prev = S.mu[0];
  tm.sync();
  if (all) return bcg::end_tile(S, S.tres, s, 0, steps, tm);
  if (steps >= S.maxit) return bcg::end_tile(S, S.tres, s, 2, steps, tm);
  if (cycle > 0 && !(mu < mu_prev)) return bcg::end_tile(S, S.tres, s, 1, steps, tm);
  if (tm.rank() == 0) S.mu[0] = mu, S.ctl[0] = 1;
  tm.sync();
}

// Mode 1, after cycle_start: G = Rn^H Rn of the normalized residuals -> S (r x s), rank r; E1 = I[:, piv] inv(S[:, piv])
// (Rh = Rn E1), C = S diag(rho / beta).  r == 0 or a bad Gram: every column not <= rtol gets flag 1, the tile is over.
template <class T, class Team>
HIFAMD_HD inline void cycle_factor(const Small<T> &S, const bcg::Work<T> &W, int s, bool first, int steps, const Team &tm) {
  if (S.ctl[0] != 1) return;
  tm.sync();
  const bcg::Chol f = bcg::factor_basis(S.G, s, S.deftol, W, S.E1, S.E2, tm);
  if (tm.rank() == 0) {
    if (first) S.ctl[1] = S.ctl[2] = f.r;
    S.ctl[3] = f.r;
  }
  tm.sync();
  if (f.bad || f.r == 0) return bcg::end_tile(S, S.tres, s, 1, steps, tm);
  for (int e = tm.rank(); e < kLd * kLd; e += tm.size()) {
    const int i = e / kLd, j = e % kLd;
    T v;
    bcg::set(v, 0.0);
    S.C[e] = (i < f.r && j < s) ? bcg::scale(S.tres[j], W.W2[e]) : v;
  }
  tm.sync();
}

// Mode 2: G = W^H W of the projected direction block (r x r) -> S1, rank q; E1 = I[:, piv] inv(S1[:, piv]) (Q_j = W E1,
// P_j = Z E1).  q == 0: the cycle ends (the coefficients stay zero, so the step's remaining passes change nothing).  A bad
// Gram ends the tile as in mode 1.
template <class T, class Team>
HIFAMD_HD inline void step_basis(const Small<T> &S, const bcg::Work<T> &W, int s, int steps, const Team &tm) {
  if (S.ctl[0] != 1) return;
  const int r = S.ctl[3];
  tm.sync();
  const bcg::Chol f = bcg::factor_basis(S.G, r, S.deftol, W, S.E1, S.E2, tm);
  if (tm.rank() == 0) S.ctl[2] = r, S.aux[0] = f.r;
  tm.sync();
  if (f.bad) return bcg::end_tile(S, S.tres, s, 1, steps, tm);
  if (f.r == 0) bcg::set_state(S, 2, tm);
}

// Mode 3: G = D = Q_j^H Rh (q x r, as it is): E1 = D C diag(beta) (X += P_j E1), E2 = D (Rh -= Q_j E2)
template <class T, class Team>
HIFAMD_HD inline void step_coeff(const Small<T> &S, const bcg::Work<T> &W, int s, const Team &tm) {
  if (S.ctl[0] != 1) return;
  const int r = S.ctl[3], q = S.aux[0];
  tm.sync();
  bcg::clear(S.E1, tm);
  bcg::stage(S.G, W.W1, q, r, tm);
  bcg::stage(W.W1, S.E2, q, r, tm);
  bcg::times_C_beta(W.W1, q, r, s, S, W.W2, W.d, tm);
}

// Mode 4: G = H = Rh^H Rh (r x r): rel_j = sqrt(max(0, c_j^H H c_j)).  All rel <= rtol, steps == maxit or the cycle's last
// step (`last`): the cycle ends, BEFORE H is factored.  Otherwise H -> S (r' x r): r' == 0 ends the cycle, a bad H the tile;
// E1 = I[:, piv] inv(S[:, piv]) (Rh <- Rh E1), C <- S C, r <- r'.
template <class T, class Team>
HIFAMD_HD inline void step_test(const Small<T> &S, const bcg::Work<T> &W, int s, int steps, bool last, const Team &tm) {
  if (S.ctl[0] != 1) return;
  const int r = S.ctl[3];
  tm.sync();
  bcg::clear(S.E1, tm);
  bcg::clear(S.E2, tm);
  bcg::stage(S.G, W.W1, r, r, tm);
  bcg::hermitize(W.W1, W.W2, r, tm);
  bcg::stage(S.C, W.W2, r, s, tm);
  bcg::quad_forms(W.W1, W.W2, r, s, S.G, S.relres, tm);
  bool all = true;
  for (int c = 0; c < s; ++c) all = all && S.relres[c] <= S.rtol;
  tm.sync();
  if (all || steps >= S.maxit || last) return bcg::set_state(S, 2, tm);
  const bcg::Chol f = bcg::factor_staged(W, r, S.deftol, S.E1, tm);
  if (f.bad) return bcg::end_tile(S, S.tres, s, 1, steps, tm);
  if (f.r == 0) return bcg::set_state(S, 2, tm);
  bcg::advance_C(W, f.r, r, s, S.C, S.G, tm);
  if (tm.rank() == 0) S.ctl[3] = f.r;
  tm.sync();
}

}  // namespace bgcr
}  // namespace hifamd
