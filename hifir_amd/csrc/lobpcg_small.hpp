// The small-matrix arithmetic of the LOBPCG driver (Engine::lobpcg_tile, k_lob_small in kernels.hip.hpp): the Rayleigh-Ritz
// step on the basis [X W P] of s = 3 k <= 48 columns -- Hermitian parts of the two Grams, the scaled pivoted Cholesky that
// orthonormalizes the basis and drops its dependent columns, the reduced matrix, its Hermitian eigendecomposition by a cyclic
// Jacobi method, and the coefficient matrices [C Cp] of the row pass.  Plain C++17, no HIP include: the one-workgroup kernel
// and host programs built with g++ (tests/cpp/lobpcg_small_test.cpp) run the same code.  The Cholesky, the triangular
// inverse, the products and the shared constructions (bcg::stage, clear, factor_staged) are blockcg_small.hpp's, and so are the conventions: row-major matrices of row stride kLd = 64,
// functions called by every thread of a Team, every output element computed by one thread with its sums in a fixed order (the
// team's size does not change a bit), a barrier at the end of every function.
#pragma once
#include "blockcg_small.hpp"

namespace hifamd {
namespace lob {

using bcg::kLd;
constexpr int kMaxK = 16;       // widest block of eigenvector candidates
constexpr int kMaxS = 3 * kMaxK;  // widest basis [X W P]
constexpr int kMaxSweeps = 30;  // Jacobi sweeps before the eigendecomposition counts as broken down

// G := its Hermitian part as given by its upper triangle: G[j][i] = conj(G[i][j]) for i < j, a real diagonal.  (The Gram
// kernel accumulates the upper block triangle only; what the lower one holds is never read.)
template <class T, class Team>
HIFAMD_HD inline void hermitize_upper(T *G, int m, const Team &tm) {
  for (int e = tm.rank(); e < m * m; e += tm.size()) {
    const int i = e / m, j = e - i * m;
    if (i == j) bcg::set(G[i * kLd + i], bcg::re(G[i * kLd + i]));
    if (i > j) G[i * kLd + j] = bcg::cj(G[j * kLd + i]);
  }
  tm.sync();
}

// dsc[j] = G[j][j]^(-1/2), 0 where the diagonal is not positive; G := D G D on the upper triangle, mirrored (hermitize_upper)
template <class T, class Team>
HIFAMD_HD inline void scale_unit_diagonal(T *G, int m, double *dsc, const Team &tm) {
  for (int j = tm.rank(); j < m; j += tm.size()) {
    const double g = bcg::re(G[j * kLd + j]);
    dsc[j] = g > 0.0 ? 1.0 / std::sqrt(g) : 0.0;
  }
  tm.sync();
  for (int e = tm.rank(); e < m * m; e += tm.size()) {
    const int i = e / m, j = e - i * m;
    if (i <= j) G[i * kLd + j] = bcg::scale(dsc[j], bcg::scale(dsc[i], G[i * kLd + j]));
  }
  tm.sync();
  hermitize_upper(G, m, tm);
}

// true when an entry of the m x m matrix G is not finite; word: one int of scratch that every thread may write
template <class T, class Team>
HIFAMD_HD inline bool any_nonfinite(const T *G, int m, int *word, const Team &tm) {
  if (tm.rank() == 0) *word = 0;
  tm.sync();
  for (int e = tm.rank(); e < m * m; e += tm.size())
    if (!bcg::finite(G[(e / m) * kLd + e % m])) *word = 1;
  tm.sync();
  const bool bad = *word != 0;
  tm.sync();
  return bad;
}

// Out (b x c) = A^H B, A (a x b), B (a x c).  Out must not alias A or B.
template <class T, class Team>
HIFAMD_HD inline void matmul_ah(const T *A, const T *B, int a, int b, int c, T *Out, const Team &tm) {
  for (int e = tm.rank(); e < b * c; e += tm.size()) {
    const int i = e / c, j = e - i * c;
    T acc;
    bcg::set(acc, 0.0);
    HIFAMD_BCG_UNROLL
    for (int l = 0; l < a; ++l) acc = bcg::add(acc, bcg::mul(bcg::cj(A[l * kLd + i]), B[l * kLd + j]));
    Out[i * kLd + j] = acc;
  }
  tm.sync();
}

template <class T, class Team>
HIFAMD_HD inline void identity(T *V, int m, const Team &tm) {
  for (int e = tm.rank(); e < m * m; e += tm.size()) bcg::set(V[(e / m) * kLd + e % m], e / m == e % m ? 1.0 : 0.0);
  tm.sync();
}

// The pair that index i (0 <= i < m / 2) plays in round t (0 <= t < m - 1) of the round-robin schedule of m players, m even:
// m - 1 rounds of m / 2 disjoint pairs that together hold every pair once.  p < q.
HIFAMD_HD inline void round_robin_pair(int m, int t, int i, int &p, int &q) {
  const int a = (i == 0) ? m - 1 : (t + i) % (m - 1), b = (i == 0) ? t : (t - i + m - 1) % (m - 1);
  p = a < b ? a : b, q = a < b ? b : a;
}

// scratch of jacobi(): per index its partner in the round, the cosine, and the sine of the rotation of its pair
template <class T>
struct JacobiScratch {
  int *mate;    // [64] partner of the index in this round; the index itself where no rotation is due
  double *c;    // [64]
  T *s;         // [64]  J[p][q] of the pair, stored at p and at q
  int *count;   // [1]   rotations of the running sweep
};

// Hermitian eigendecomposition of H (r x r) by the cyclic Jacobi method: on return H is diagonal up to entries of at most
// 2^-53 ||H||_F (the eigenvalues are its diagonal, in no particular order), V := V J for the product J of all rotations
// (V = I gives the eigenvectors as columns).  The pair order is the round-robin schedule above, the same for every team:
// the rotations of a round act on disjoint index pairs, so the round is one two-sided update H <- J^H H J (columns, then
// rows; every entry is changed by one thread per half) and V <- V J.  A pair rotates when |h_pq| > 2^-53 ||H||_F of the
// start; the method ends when a full sweep rotates nothing.  -> sweeps done (the clean one included), or -1 after
// kMaxSweeps sweeps that all rotated.
template <class T, class Team>
HIFAMD_HD inline int jacobi(T *H, T *V, int r, const JacobiScratch<T> &w, const Team &tm) {
  const int m = r + (r & 1);
  double f2 = 0.0;  // (every thread sums every entry in the same order: no reduction, no dependence on the team)
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < r; ++j) f2 += bcg::abs2(H[i * kLd + j]);
  const double thr = std::sqrt(f2) * 0x1p-53;
  tm.sync();
  for (int sweep = 1; sweep <= kMaxSweeps; ++sweep) {
    if (tm.rank() == 0) *w.count = 0;
    tm.sync();
    for (int t = 0; t < m - 1; ++t) {
      for (int i = tm.rank(); i < m / 2; i += tm.size()) {
        int p, q;
        round_robin_pair(m, t, i, p, q);
        if (q >= r) {  // the bye of an odd order
          w.mate[p] = p;
          continue;
        }
        const T g = H[p * kLd + q];
        const double ag = std::sqrt(bcg::abs2(g));
        if (!(ag > thr)) {
          w.mate[p] = p, w.mate[q] = q;
          continue;
        }
        const double a = bcg::re(H[p * kLd + p]), b = bcg::re(H[q * kLd + q]);
        const double tau = (b - a) / (2.0 * ag);
        const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
        const double cs = 1.0 / std::sqrt(1.0 + tt * tt), sn = tt * cs;
        w.mate[p] = q, w.mate[q] = p;
        w.c[p] = w.c[q] = cs;
        w.s[p] = w.s[q] = bcg::scale(sn / ag, g);  // sn e^{i phi}, g = |g| e^{i phi}
        *w.count = 1;  // (several threads may store the same value; it is read after the sweep's last barrier)
      }
      tm.sync();
      // columns: (h_ap, h_aq) <- (h_ap c - h_aq conj(s), h_ap s + h_aq c), and the same for V
      for (int e = tm.rank(); e < r * (m / 2); e += tm.size()) {
        const int a = e / (m / 2);
        int p, q;
        round_robin_pair(m, t, e - a * (m / 2), p, q);
        if (q >= r || w.mate[p] == p) continue;
        const double cs = w.c[p];
        const T s = w.s[p], sc = bcg::cj(s);
        const T hp = H[a * kLd + p], hq = H[a * kLd + q], vp = V[a * kLd + p], vq = V[a * kLd + q];
        H[a * kLd + p] = bcg::sub(bcg::scale(cs, hp), bcg::mul(hq, sc));
        H[a * kLd + q] = bcg::add(bcg::mul(hp, s), bcg::scale(cs, hq));
        V[a * kLd + p] = bcg::sub(bcg::scale(cs, vp), bcg::mul(vq, sc));
        V[a * kLd + q] = bcg::add(bcg::mul(vp, s), bcg::scale(cs, vq));
      }
      tm.sync();
      // rows: (h_pb, h_qb) <- (c h_pb - s h_qb, conj(s) h_pb + c h_qb); the rotated pair's own entries are set exactly
      for (int e = tm.rank(); e < r * (m / 2); e += tm.size()) {
        const int b = e / (m / 2);
        int p, q;
        round_robin_pair(m, t, e - b * (m / 2), p, q);
        if (q >= r || w.mate[p] == p) continue;
        const double cs = w.c[p];
        const T s = w.s[p], sc = bcg::cj(s);
        const T hp = H[p * kLd + b], hq = H[q * kLd + b];
        T np = bcg::sub(bcg::scale(cs, hp), bcg::mul(s, hq)), nq = bcg::add(bcg::mul(sc, hp), bcg::scale(cs, hq));
        if (b == p) bcg::set(np, bcg::re(np)), bcg::set(nq, 0.0);
        if (b == q) bcg::set(np, 0.0), bcg::set(nq, bcg::re(nq));
        H[p * kLd + b] = np;
        H[q * kLd + b] = nq;
      }
      tm.sync();
    }
    const bool clean = *w.count == 0;
    tm.sync();
    if (clean) return sweep;
  }
  return -1;
}

// perm[j] = the index of the j-th smallest of d[0 .. r - 1]; equal values in index order
template <class Team>
HIFAMD_HD inline void order_ascending(const double *d, int r, int *perm, const Team &tm) {
  for (int i = tm.rank(); i < r; i += tm.size()) {
    int pos = 0;
    for (int j = 0; j < r; ++j) pos += (d[j] < d[i] || (d[j] == d[i] && j < i)) ? 1 : 0;
    perm[pos] = i;
  }
  tm.sync();
}

struct Ritz {
  int r;       // rank of the basis (columns kept by the Cholesky; the basis size where none is run)
  int sweeps;  // Jacobi sweeps (0: not reached)
  bool bad;    // breakdown: a non-finite Gram, the Cholesky's own, r < k, a Jacobi method that does not end
  bcg::Chol f;  // what the Cholesky left (chol == true)
};

// what rayleigh_ritz() works in: W1, W2 are the hot matrices (LDS on the device), X1 .. X3 may be slow (HBM); all [64][64].  All
// but X1 .. X3 is carved from the kernel's dynamic LDS of bytes() bytes: W1 | W2 | jac.s | d | dsc | jac.c | piv | taken | perm | mate | count
template <class T>
struct RitzScratch {
  T *W1, *W2, *X1, *X2, *X3;
  double *d, *dsc;  // [64] each
  int *piv, *taken, *perm;  // [64] each
  JacobiScratch<T> jac;
  HIFAMD_HD bcg::Work<T> work() const { return bcg::Work<T>{W1, W2, d, piv, taken}; }  // (what block CG's constructions take)
  static constexpr size_t bytes() { return bcg::Work<T>::bytes() + kLd * sizeof(T) + 2 * kLd * sizeof(double) + (2 * kLd + 4) * sizeof(int); }
  HIFAMD_HD static RitzScratch carve(void *base, T *X1, T *X2, T *X3) {
    T *W1 = (T *)base, *W2 = W1 + kLd * kLd, *js = W2 + kLd * kLd;
    double *d = (double *)(js + kLd), *dsc = d + kLd, *jc = dsc + kLd;
    int *piv = (int *)(jc + kLd), *taken = piv + kLd, *perm = taken + kLd, *mate = perm + kLd;
    return RitzScratch{W1, W2, X1, X2, X3, d, dsc, piv, taken, perm, JacobiScratch<T>{mate, jc, js, mate + kLd}};
  }
};

// One Rayleigh-Ritz step on a basis S of s columns with the summed Grams GB = S^H S and GA = S^H A S (upper triangles):
//   chol: D = diag(GB)^(-1/2) (0 where the diagonal is not positive), D GB D = T^H T pivoted Cholesky stopped
//         at deftol, rank r (r < k: bad), E = D I[:, piv] inv(T[:, piv]) (s x r);   else: E = I (s x s), r = s
//   H = E^H GA E = V Theta V^H, ascending (ties: lowest index), C = E V[:, :k], lam = Theta[:k]
//   CC [64][64]: columns 0 .. k - 1 = C, columns 16 .. 16 + k - 1 = C with its first k rows zero (Cp); rows >= s and the other
//   columns < 32 zero.
// On bad, CC and lam are left alone.
template <class T, class Team>
HIFAMD_HD inline Ritz rayleigh_ritz(const T *GB, const T *GA, int s, int k, double deftol, bool chol,
                                    const RitzScratch<T> &w, T *CC, double *lam, const Team &tm) {
  Ritz out{s, 0, false, bcg::Chol{0, false, 0.0, 0.0, 0.0}};
  T *W1 = w.W1, *W2 = w.W2;
  if (chol) {
    bcg::stage(GB, W1, s, s, tm);
    hermitize_upper(W1, s, tm);
    if (any_nonfinite(W1, s, w.jac.count, tm)) {
      out.bad = true;
      return out;
    }
    scale_unit_diagonal(W1, s, w.dsc, tm);
    out.f = bcg::factor_staged(w.work(), s, deftol, W2, tm);  // (W2: the factor, then I[:, piv] inv(T[:, piv]))
    out.r = out.f.r;
    if (out.f.bad || out.r < k) {
      out.bad = true;
      return out;
    }
    for (int e = tm.rank(); e < s * out.r; e += tm.size()) {
      T &v = W2[(e / out.r) * kLd + e % out.r];
      v = bcg::scale(w.dsc[e / out.r], v);
    }
    tm.sync();
  } else {
    identity(W2, s, tm);
  }
  const int r = out.r;
  bcg::stage((const T *)W2, w.X1, s, r, tm);  // E
  bcg::stage(GA, W1, s, s, tm);
  hermitize_upper(W1, s, tm);
  bcg::matmul(W1, W2, false, s, s, r, (const double *)nullptr, w.X2, tm);  // GA E
  matmul_ah(W2, w.X2, s, r, r, w.X3, tm);                                   // E^H GA E
  bcg::stage((const T *)w.X3, W1, r, r, tm);
  bcg::hermitize(W1, w.X3, r, tm);
  if (any_nonfinite(W1, r, w.jac.count, tm)) {
    out.bad = true;
    return out;
  }
  identity(W2, r, tm);
  out.sweeps = jacobi(W1, W2, r, w.jac, tm);
  if (out.sweeps < 0) {
    out.bad = true;
    return out;
  }
  for (int i = tm.rank(); i < r; i += tm.size()) w.d[i] = bcg::re(W1[i * kLd + i]);
  tm.sync();
  order_ascending(w.d, r, w.perm, tm);
  for (int e = tm.rank(); e < kLd * 2 * kMaxK; e += tm.size()) {
    const int i = e / (2 * kMaxK), c = e - i * (2 * kMaxK), j = c % kMaxK;
    T acc;
    bcg::set(acc, 0.0);
    if (i < s && j < k && !(c >= kMaxK && i < k)) {
      const int col = w.perm[j];
      HIFAMD_BCG_UNROLL
      for (int l = 0; l < r; ++l) acc = bcg::add(acc, bcg::mul(w.X1[i * kLd + l], W2[l * kLd + col]));
    }
    CC[i * kLd + c] = acc;
  }
  for (int j = tm.rank(); j < k; j += tm.size()) lam[j] = w.d[w.perm[j]];
  tm.sync();
  return out;
}

// ---- the decisions of a tile: what k_lob_small runs, mode by mode -------------------------------------------------------------
// The tile's state as the decisions see it.  ctl: [0] 1 while the tile runs, [1] rank of the basis in the last step,
// [2] largest Jacobi sweep count, [3] the start's verdict (kStart*).  flag / iter / active / lam / res: [64] each; active[c] = 1
// for a column that the last test did not find converged.
constexpr int kStartFine = 0, kStartRankDeficient = 1, kStartNotFinite = 2, kStartRitzFailed = 3;
template <class T>
struct Small {
  T *GB, *GA, *CC;  // [64][64]: the summed Grams (upper triangles), [C Cp] of the next row pass
  double *lam, *res;
  int *flag, *iter, *active, *ctl;
  double tol, deftol, anorm;
  int maxit, k, nev;
  double bnorm = 0.0;  // ||B||_inf of the generalized problem (residual_gen); the standard test does not read it
};

// The start's factorization: GB = X0^H X0 (k x k) -> pivoted Cholesky.  Not finite / rank < k (or a leftover below -deftol):
// ctl[3] = kStartNotFinite / kStartRankDeficient and the tile is over; else CC = [E 0], E = I[:, piv] inv(S[:, piv]).
// Resets every per-column word.
template <class T, class Team>
HIFAMD_HD inline void start_factor(const Small<T> &S, const RitzScratch<T> &w, const Team &tm) {
  const int k = S.k;
  for (int t = tm.rank(); t < kLd; t += tm.size())
    S.flag[t] = 0, S.iter[t] = 0, S.active[t] = t < k ? 1 : 0, S.res[t] = HUGE_VAL, S.lam[t] = 0.0;
  if (tm.rank() == 0) S.ctl[0] = 1, S.ctl[1] = k, S.ctl[2] = 0, S.ctl[3] = kStartFine;
  bcg::clear(S.CC, tm);
  bcg::stage((const T *)S.GB, w.W1, k, k, tm);
  hermitize_upper(w.W1, k, tm);
  const bool inf = any_nonfinite(w.W1, k, w.jac.count, tm);
  bcg::Chol f{0, false, 0.0, 0.0, 0.0};
  if (!inf) f = bcg::factor_staged(w.work(), k, S.deftol, S.CC, tm);  // (the Gram arrives as an upper triangle: no factor_basis)
  if ((inf || f.bad || f.r < k) && tm.rank() == 0) S.ctl[0] = 0, S.ctl[3] = inf ? kStartNotFinite : kStartRankDeficient;
  tm.sync();
}

// res_j of the standard problem from nb partials of |r_j|^2 (partial[b][16], summed in block order): sqrt(sum) / ||A||_inf
template <class T>
HIFAMD_HD inline double residual_std(const Small<T> &S, const double *partial, int nb, int c) {
  double tot = partial[c];
  for (int b = 1; b < nb; ++b) tot += partial[b * kMaxK + c];
  return S.anorm > 0.0 ? std::sqrt(tot) / S.anorm : std::sqrt(tot);
}

// res_j of the generalized problem A x = lambda B x from nb partials of |r_j|^2 and |x_j|^2 (partial[b][32]: |r_j|^2 at j,
// |x_j|^2 at 16 + j; summed in block order), r_j = A x_j - lambda_j B x_j:
// res_j = ||r_j|| / ((||A||_inf + |lambda_j| ||B||_inf) ||x_j||), the normwise backward error of the pair -- the vectors are
// B-normalized, so ||x_j|| belongs in the scale.  A scale of exactly zero (x_j = 0, or both norms zero) leaves res_j = ||r_j||;
// a scale that is not finite counts as not converged (res_j = HUGE_VAL), and so does a partial that is not finite (res_j is
// NaN).
template <class T>
HIFAMD_HD inline double residual_gen(const Small<T> &S, const double *partial, int nb, int c) {
  double rr = partial[c], xx = partial[kMaxK + c];
  for (int b = 1; b < nb; ++b) rr += partial[b * 2 * kMaxK + c], xx += partial[b * 2 * kMaxK + kMaxK + c];
  const double scale = (S.anorm + std::fabs(S.lam[c]) * S.bnorm) * std::sqrt(xx);
  double res = scale == 0.0 ? std::sqrt(rr) : std::sqrt(rr) / scale;
  if (scale > 1.7976931348623157e308) res = HUGE_VAL;
  return res;
}

// The residual test after `step` completed steps: res_j = res_of(c) for every column (residual_std or residual_gen of the
// partials), active_j = res_j > tol; every j < nev converged, or step >= maxit: flags 0 / 2 by each column's own res_j,
// iter = step, and the tile is over.  A tile that is over is left alone.
template <class T, class Team, class ResOf>
HIFAMD_HD inline void residual_verdict(const Small<T> &S, int step, const Team &tm, const ResOf &res_of) {
  const bool over = S.ctl[0] == 0;
  tm.sync();  // (everybody has read ctl before thread 0 may change it)
  if (over) return;
  for (int c = tm.rank(); c < S.k; c += tm.size()) {
    const double res = res_of(c);
    S.res[c] = res;
    S.active[c] = res <= S.tol ? 0 : 1;
  }
  tm.sync();
  bool all = true;
  for (int c = 0; c < S.nev; ++c) all = all && S.active[c] == 0;
  if (all || step >= S.maxit) {
    for (int c = tm.rank(); c < S.k; c += tm.size()) S.flag[c] = S.active[c] ? 2 : 0, S.iter[c] = step;
    if (tm.rank() == 0) S.ctl[0] = 0;
  }
  tm.sync();
}
template <class T, class Team>
HIFAMD_HD inline void residual_test(const Small<T> &S, const double *partial, int nb, int step, const Team &tm) {
  residual_verdict(S, step, tm, [&](int c) { return residual_std(S, partial, nb, c); });
}
template <class T, class Team>
HIFAMD_HD inline void residual_test_gen(const Small<T> &S, const double *partial, int nb, int step, const Team &tm) {
  residual_verdict(S, step, tm, [&](int c) { return residual_gen(S, partial, nb, c); });
}

// The Rayleigh-Ritz step of the tile after `step` completed steps.  start: on GA = X^H A X (k x k), no Cholesky; a failure
// (GA not finite, a Jacobi method that does not end) is ctl[3] = kStartRitzFailed and the tile is over.  Else on GB, GA
// (3 k x 3 k): CC = [C Cp], lambda, ctl[1] = rank; a breakdown ends the tile: flag 1 for every column that was not converged
// at the last test, iter = step, and CC = [I 0], so that the row pass leaves X and AX as they are.  A tile that is over is
// left alone.
template <class T, class Team>
HIFAMD_HD inline void ritz_step(const Small<T> &S, const RitzScratch<T> &w, bool start, int step, const Team &tm) {
  const bool over = S.ctl[0] == 0;
  tm.sync();
  if (over) return;
  const int k = S.k;
  const Ritz out = rayleigh_ritz((const T *)S.GB, (const T *)S.GA, start ? k : 3 * k, k, S.deftol, !start, w, S.CC, S.lam, tm);
  if (out.bad && start) {
    if (tm.rank() == 0) S.ctl[0] = 0, S.ctl[3] = kStartRitzFailed;
  } else if (out.bad) {
    for (int e = tm.rank(); e < kLd * kLd; e += tm.size()) bcg::set(S.CC[e], (e / kLd == e % kLd && e % kLd < k) ? 1.0 : 0.0);
    for (int c = tm.rank(); c < k; c += tm.size()) S.flag[c] = S.active[c] ? 1 : 0, S.iter[c] = step;
    if (tm.rank() == 0) S.ctl[0] = 0;
  } else if (tm.rank() == 0) {
    S.ctl[1] = out.r, S.ctl[2] = out.sweeps > S.ctl[2] ? out.sweeps : S.ctl[2];
  }
  tm.sync();
}

// ---- the decisions between the locked sweeps (Engine::eigs_dev): host only, no device state -------------------------------------
constexpr int kMaxLocked = 128;  // widest constraint block: the caller's m0 columns plus the nev locked ones

// columns the sweep asks its tile for: what is still wanted, at most the block without its guard columns
inline int sweep_want(int nev, int locked, int k, int guard) {
  const int left = nev - locked, room = k - guard;
  return left < room ? left : room;
}

// length of the leading run of flag-0 columns among the first `want`: what the sweep locks.  (A converged column behind an
// unconverged one is not locked: lambda comes back in lock order, ascending up to the tolerance.)
inline int lock_prefix(const int *flags, int want) {
  int p = 0;
  while (p < want && flags[p] == 0) ++p;
  return p;
}

// the flag of an output column that the last sweep left unlocked: the tile's 1 (breakdown) stays, everything else -- not
// converged, or converged behind an unconverged column -- is 2: 0 means locked
inline int unlocked_flag(int tile_flag) { return tile_flag == 1 ? 1 : 2; }

// the sweep loop's verdict on its arguments; nullptr when they are fine (the caps of the constraint buffers)
inline const char *sweep_args(long long nev, long long k, long long guard, long long m0) {
  if (k < 1 || k > kMaxK) return "eigs: need 1 <= k <= 16";
  if (guard < 0 || guard >= k) return "eigs: need 0 <= guard < k";
  if (nev < 1) return "eigs: need nev >= 1";
  if (m0 < 0 || m0 + nev > kMaxLocked) return "eigs: need m0 >= 0 and m0 + nev <= 128";
  return nullptr;
}

}  // namespace lob
}  // namespace hifamd
