// The small-matrix arithmetic and every decision of the block CG driver (Engine::bcg_tile, k_bcg_beta and k_bcg_small in
// kernels.hip.hpp): Hermitian Grams of at most 64 x 64, their Cholesky factors, triangular inverses, products and quadratic
// forms; the constructions that blockgcr_small.hpp and lobpcg_small.hpp share with it; the tile's decisions, mode by mode.
// Plain C++17, no HIP include: the one-workgroup kernels and host programs built with g++ (tests/cpp/blockcg_small_test.cpp,
// tests/cpp/blockcg_tile_test.cpp) run the same code.
//
// Every matrix is row-major with the row stride kLd = 64, whatever its size.  T is double or a struct {double x, y}.
// A function is called by every thread of a team: Team gives rank() (0 .. size() - 1), size() and sync() (a barrier that also
// publishes memory; Serial is the host's team of one).  Every output element is computed by one thread with its sums in a
// fixed order, so the result does not depend on the team's size.  A function ends with a barrier unless it says otherwise.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifndef HIFAMD_HD
#if defined(__HIP__) || defined(__HIPCC__)
#define HIFAMD_HD __host__ __device__
#else
#define HIFAMD_HD
#endif
#endif

// (inner loops over LDS operands: unrolled so that their loads are in flight together; the sums keep their order)
#if defined(__clang__)
#define HIFAMD_BCG_UNROLL _Pragma("unroll 8")
#else
#define HIFAMD_BCG_UNROLL _Pragma("GCC unroll 8")
#endif

namespace hifamd {

// what the states of the lock-step solvers (PCG, BiCGSTAB, symmetric QMR, ...) and of the block methods share
struct KrylovState {
  double *bnorm;                    // [64]  ||b||
  int *iter, *flag, *active, *ctl;  // [64] each; ctl[0]: columns still active
  int maxit;
  double rtol;
};

namespace bcg {

constexpr int kLd = 64;  // row stride (and the largest block)

struct Serial {
  HIFAMD_HD int rank() const { return 0; }
  HIFAMD_HD int size() const { return 1; }
  HIFAMD_HD void sync() const {}
};

// ---- value arithmetic --------------------------------------------------------------------------------------------------
HIFAMD_HD inline double re(double a) { return a; }
template <class Z> HIFAMD_HD inline double re(const Z &a) { return a.x; }
HIFAMD_HD inline double cj(double a) { return a; }
template <class Z> HIFAMD_HD inline Z cj(const Z &a) { return Z{a.x, -a.y}; }
HIFAMD_HD inline double add(double a, double b) { return a + b; }
template <class Z> HIFAMD_HD inline Z add(const Z &a, const Z &b) { return Z{a.x + b.x, a.y + b.y}; }
HIFAMD_HD inline double sub(double a, double b) { return a - b; }
template <class Z> HIFAMD_HD inline Z sub(const Z &a, const Z &b) { return Z{a.x - b.x, a.y - b.y}; }
HIFAMD_HD inline double mul(double a, double b) { return a * b; }
template <class Z> HIFAMD_HD inline Z mul(const Z &a, const Z &b) { return Z{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
HIFAMD_HD inline double scale(double s, double a) { return s * a; }
template <class Z> HIFAMD_HD inline Z scale(double s, const Z &a) { return Z{s * a.x, s * a.y}; }
HIFAMD_HD inline double abs2(double a) { return a * a; }
template <class Z> HIFAMD_HD inline double abs2(const Z &a) { return a.x * a.x + a.y * a.y; }
HIFAMD_HD inline bool finite(double a) { return a - a == 0.0; }  // (no <cmath> overload sets: the same on host and device)
template <class Z> HIFAMD_HD inline bool finite(const Z &a) { return a.x - a.x == 0.0 && a.y - a.y == 0.0; }
HIFAMD_HD inline void set(double &a, double r) { a = r; }  // a = r + 0 i
template <class Z> HIFAMD_HD inline void set(Z &a, double r) { a.x = r, a.y = 0.0; }

// what one factorization leaves besides S: everything a caller decides on (the same in every thread)
struct Chol {
  int r;           // pivots taken
  bool bad;        // breakdown: non-finite entry, a leftover below -deftol * top (pivoted), a pivot <= 0 (unpivoted)
  double top;      // largest diagonal of G
  double kept;     // smallest pivot taken / top (r == 0: 0)
  double dropped;  // leftover diagonal of largest magnitude / top (none left, or top == 0: 0)
};

// G[i][j] = sum over b = 0 .. nb - 1, in that order, of part[b][i][j], i, j < m  (part: [nb][64][64])
template <class T, class Team>
HIFAMD_HD inline void sum_partials(const T *part, int nb, int m, T *G, const Team &tm) {
  for (int e = tm.rank(); e < m * m; e += tm.size()) {
    const int i = e / m, j = e - i * m;
    const T *p = part + i * kLd + j;
    T acc = p[0];
    int b = 1;
    for (; b + 8 <= nb; b += 8) {  // (eight loads in flight; the additions keep their order)
      T v[8];
      for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(b + u) * kLd * kLd];
      for (int u = 0; u < 8; ++u) acc = add(acc, v[u]);
    }
    for (; b < nb; ++b) acc = add(acc, p[(int64_t)b * kLd * kLd]);
    G[i * kLd + j] = acc;
  }
  tm.sync();
}

// G := (G + G^H) / 2 with a real diagonal, m x m; H is scratch of the same size
template <class T, class Team>
HIFAMD_HD inline void hermitize(T *G, T *H, int m, const Team &tm) {
  for (int e = tm.rank(); e < m * m; e += tm.size()) {
    const int i = e / m, j = e - i * m;
    T v = scale(0.5, add(G[i * kLd + j], cj(G[j * kLd + i])));
    if (i == j) set(v, re(v));
    H[i * kLd + j] = v;
  }
  tm.sync();
  for (int e = tm.rank(); e < m * m; e += tm.size()) {
    const int i = e / m, j = e - i * m;
    G[i * kLd + j] = H[i * kLd + j];
  }
  tm.sync();
}

// Upper Cholesky of the Hermitian m x m matrix G: S (r x m) with G ~= S^H S, S[:, piv] upper triangular.
//   pivoted: every step takes the largest remaining diagonal (ties: the lowest index) and stops when that is
//            <= deftol * top; a leftover below -deftol * top is a breakdown, smaller ones of either sign are dropped;
//   else:    pivots in natural order; one that is not positive and finite is a breakdown.
// Rows >= r of S are left alone.  d [64] (double), taken [64] (int) are scratch, piv [64] receives the pivots.
template <class T, class Team>
HIFAMD_HD inline Chol chol(const T *G, int m, double deftol, bool pivoted, T *S, int *piv, double *d, int *taken, const Team &tm) {
  Chol out{0, false, 0.0, 0.0, 0.0};
  if (tm.rank() == 0) piv[0] = 0;  // (until the first pivot: has anybody seen a non-finite entry)
  tm.sync();
  for (int e = tm.rank(); e < m * m; e += tm.size())
    if (!finite(G[(e / m) * kLd + e % m])) piv[0] = 1;
  for (int j = tm.rank(); j < m; j += tm.size()) d[j] = re(G[j * kLd + j]), taken[j] = 0;
  tm.sync();
  const bool fin = piv[0] == 0;
  tm.sync();
  if (!fin) {
    out.bad = true;
    return out;
  }
  for (int j = 0; j < m; ++j) out.top = (j == 0 || d[j] > out.top) ? d[j] : out.top;
  double kept = 0.0;
  for (int k = 0; k < m; ++k) {
    int p = -1;
    if (pivoted) {
      double best = 0.0;  // (the running maximum in a register: the loads do not wait for the comparison)
      HIFAMD_BCG_UNROLL
      for (int j = 0; j < m; ++j) {
        const double dj = d[j];
        if (!taken[j] && (p < 0 || dj > best)) p = j, best = dj;
      }
      if (!(best > deftol * out.top)) break;
    } else {
      p = k;
      if (!(d[p] > 0.0) || !finite(d[p])) {
        out.bad = true;
        break;
      }
    }
    const double dp = d[p], root = std::sqrt(dp);
    kept = (k == 0 || dp < kept) ? dp : kept;
    tm.sync();  // every thread has chosen before d and taken change
    for (int j = tm.rank(); j < m; j += tm.size()) {
      T v;
      set(v, 0.0);
      if (j == p) {
        set(v, root);
        taken[p] = 1;
        piv[k] = p;
      } else if (!taken[j]) {
        T acc = G[p * kLd + j];
        HIFAMD_BCG_UNROLL
        for (int i = 0; i < k; ++i) acc = sub(acc, mul(cj(S[i * kLd + p]), S[i * kLd + j]));
        v = scale(1.0 / root, acc);
        d[j] -= abs2(v);
      }
      S[k * kLd + j] = v;
    }
    tm.sync();
    out.r = k + 1;
  }
  out.kept = (out.r && out.top > 0.0) ? kept / out.top : 0.0;
  for (int j = 0; j < m; ++j) {
    if (!finite(d[j])) out.bad = true;
    if (taken[j] || !pivoted) continue;
    if (d[j] < -deftol * out.top) out.bad = true;
    const double rel = out.top > 0.0 ? d[j] / out.top : 0.0;
    if (std::fabs(rel) > std::fabs(out.dropped)) out.dropped = rel;
  }
  tm.sync();  // (d and taken may be reused)
  return out;
}

// Ti = inv(S[:, piv]) (r x r upper triangular; the strict lower triangle is set to zero), column by column by back substitution
template <class T, class Team>
HIFAMD_HD inline void tri_inv(const T *S, const int *piv, int r, T *Ti, const Team &tm) {
  for (int c = tm.rank(); c < r; c += tm.size()) {
    const T one_over = scale(1.0 / re(S[c * kLd + piv[c]]), T{1.0});
    Ti[c * kLd + c] = one_over;
    for (int i = c + 1; i < r; ++i) set(Ti[i * kLd + c], 0.0);
    for (int i = c - 1; i >= 0; --i) {
      T acc;
      set(acc, 0.0);
      HIFAMD_BCG_UNROLL
      for (int l = i + 1; l <= c; ++l) acc = add(acc, mul(S[i * kLd + piv[l]], Ti[l * kLd + c]));
      Ti[i * kLd + c] = scale(-1.0 / re(S[i * kLd + piv[i]]), acc);
    }
  }
  tm.sync();
}

// E (m x w, zero-padded to w columns) = I[:, piv] Ti: row piv[i] of E is row i of Ti (r x r), every other entry zero
template <class T, class Team>
HIFAMD_HD inline void select_rows(const T *Ti, const int *piv, int r, int m, int w, T *E, const Team &tm) {
  for (int e = tm.rank(); e < m * w; e += tm.size()) set(E[(e / w) * kLd + e % w], 0.0);
  tm.sync();
  for (int e = tm.rank(); e < r * r; e += tm.size()) {
    const int i = e / r, j = e - i * r;
    E[piv[i] * kLd + j] = Ti[i * kLd + j];
  }
  tm.sync();
}

// Out (a x c) = A (a x b) B (b x c), or A B^H with B (c x b) when bh; colscale (may be null): column j times colscale[j].
// Out must not alias A or B.
template <class T, class Team>
HIFAMD_HD inline void matmul(const T *A, const T *B, bool bh, int a, int b, int c, const double *colscale, T *Out, const Team &tm) {
  for (int e = tm.rank(); e < a * c; e += tm.size()) {
    const int i = e / c, j = e - i * c;
    T acc;
    set(acc, 0.0);
    HIFAMD_BCG_UNROLL
    for (int l = 0; l < b; ++l) acc = add(acc, mul(A[i * kLd + l], bh ? cj(B[j * kLd + l]) : B[l * kLd + j]));
    Out[i * kLd + j] = colscale ? scale(colscale[j], acc) : acc;
  }
  tm.sync();
}

// Out (b x a) = A^H, A (a x b)
template <class T, class Team>
HIFAMD_HD inline void adjoint(const T *A, int a, int b, T *Out, const Team &tm) {
  for (int e = tm.rank(); e < a * b; e += tm.size()) {
    const int i = e / b, j = e - i * b;
    Out[j * kLd + i] = cj(A[i * kLd + j]);
  }
  tm.sync();
}

// out[j] = sqrt(max(0, c_j^H H c_j)), c_j column j of C (r x s), H (r x r) Hermitian; HC (r x s) receives H C
template <class T, class Team>
HIFAMD_HD inline void quad_forms(const T *H, const T *C, int r, int s, T *HC, double *out, const Team &tm) {
  matmul(H, C, false, r, r, s, (const double *)nullptr, HC, tm);
  for (int j = tm.rank(); j < s; j += tm.size()) {
    double tot = 0.0;
    for (int i = 0; i < r; ++i) tot += re(mul(cj(C[i * kLd + j]), HC[i * kLd + j]));
    out[j] = std::sqrt(tot > 0.0 ? tot : 0.0);
  }
  tm.sync();
}

// ---- what block CG, block GCR and LOBPCG build from the functions above ---------------------------------------------------------
// The small state of a tile of s <= 64 columns (the kernels' BcgState).  bnorm: beta = ||b||; active: 1 for a column of the block (not
// zero, not excluded); ctl: [0] 1 while the tile runs, [1] rank after the start, [2] rank during the last step, [3] current rank
template <class T>
struct Small : KrylovState {
  T *C, *E1, *E2, *G;  // [64][64] each: R = Q C | the two coefficient matrices of the next row pass | the summed Gram
  double *relres;      // [64]  ||r|| / ||b|| at the last test (infinite before the first)
  double deftol;
};

// What a one-workgroup kernel works in: W1 | W2 | d [64] | piv [64] | taken [64], carved from its dynamic LDS of bytes() bytes
template <class T>
struct Work {
  T *W1, *W2;
  double *d;
  int *piv, *taken;
  static constexpr size_t bytes() { return 2 * kLd * kLd * sizeof(T) + kLd * sizeof(double) + 2 * kLd * sizeof(int); }
  HIFAMD_HD static Work carve(void *base) {
    T *W1 = (T *)base;
    double *d = (double *)(W1 + 2 * kLd * kLd);
    return Work{W1, W1 + kLd * kLd, d, (int *)(d + kLd), (int *)(d + kLd) + kLd};
  }
};

// to = from on rows x cols, zero on the rest of the 64 x 64 (the state's matrices into LDS: no inner loop reads HBM)
template <class T, class Team>
HIFAMD_HD inline void stage(const T *from, T *to, int rows, int cols, const Team &tm) {
  for (int e = tm.rank(); e < kLd * kLd; e += tm.size()) {
    T v;
    set(v, 0.0);
    if (e / kLd < rows && e % kLd < cols) v = from[e];  // (not a choice between two lvalues: the zero stays in registers)
    to[e] = v;
  }
  tm.sync();
}

template <class T, class Team>
HIFAMD_HD inline void clear(T *E, const Team &tm) {
  for (int e = tm.rank(); e < kLd * kLd; e += tm.size()) set(E[e], 0.0);
  tm.sync();
}

template <class Team>
HIFAMD_HD inline void set_state(const KrylovState &S, int v, const Team &tm) {  // ctl[0] = v
  if (tm.rank() == 0) S.ctl[0] = v;
  tm.sync();
}

// The tile is over: a block column gets flag 0 where res (its last tested ratio) is <= rtol, else `miss`; `done` is its count
template <class Team>
HIFAMD_HD inline void end_tile(const KrylovState &S, const double *res, int s, int miss, int done, const Team &tm) {
  for (int c = tm.rank(); c < s; c += tm.size())
    if (S.active[c]) S.flag[c] = res[c] <= S.rtol ? 0 : miss, S.iter[c] = done;
  set_state(S, 0, tm);
}

// The Hermitian m x m matrix in W.W1 -> pivoted Cholesky factor S (r x m) in W.W2 and, unless it broke down or r == 0,
// E1 (cleared by the caller) = I[:, piv] inv(S[:, piv]); W.W1 is overwritten.
template <class T, class Team>
HIFAMD_HD inline Chol factor_staged(const Work<T> &W, int m, double deftol, T *E1, const Team &tm) {
  const Chol f = chol(W.W1, m, deftol, true, W.W2, W.piv, W.d, W.taken, tm);
  if (!f.bad && f.r > 0) tri_inv(W.W2, W.piv, f.r, W.W1, tm), select_rows(W.W1, W.piv, f.r, m, f.r, E1, tm);
  return f;
}

// The same on the summed Gram G (m x m), staged into W.W1 and made Hermitian; E1 and E2 are cleared first.
template <class T, class Team>
HIFAMD_HD inline Chol factor_basis(const T *G, int m, double deftol, const Work<T> &W, T *E1, T *E2, const Team &tm) {
  clear(E1, tm);
  clear(E2, tm);
  stage(G, W.W1, m, m, tm);
  hermitize(W.W1, W.W2, m, tm);
  return factor_staged(W, m, deftol, E1, tm);
}

// C (r x s) <- S C (r_new x s), zero-padded, with the factor S (r_new x r) in W.W2; W.W1 and G are scratch
template <class T, class Team>
HIFAMD_HD inline void advance_C(const Work<T> &W, int r_new, int r, int s, T *C, T *G, const Team &tm) {
  stage(C, W.W1, r, s, tm);
  matmul(W.W2, W.W1, false, r_new, r, s, (const double *)nullptr, G, tm);
  stage(G, C, r_new, s, tm);
}

// E1 = A C diag(beta) (a x s), A (a x r) in LDS, beta = 0 for a column outside the block; Cw (LDS) receives C, d the betas
template <class T, class Team>
HIFAMD_HD inline void times_C_beta(const T *A, int a, int r, int s, const Small<T> &S, T *Cw, double *d, const Team &tm) {
  for (int c = tm.rank(); c < kLd; c += tm.size()) d[c] = (c < s && S.active[c]) ? S.bnorm[c] : 0.0;
  stage(S.C, Cw, r, s, tm);
  matmul(A, Cw, false, a, r, s, d, S.E1, tm);
}

// ---- the decisions of a block CG tile: what k_bcg_beta and k_bcg_small run, mode by mode ----------------------------------
// The start's scalars from b2[c] = |b_c|^2: beta_c, and which columns enter the block.  A zero column is done (x = 0,
// flag 0), a column whose |b|^2 is not finite is excluded (x = 0, flag 1); both 0 iterations.
template <class T, class Team>
HIFAMD_HD inline void start_columns(const Small<T> &S, int nc, const double *b2, const Team &tm) {
  for (int c = tm.rank(); c < nc; c += tm.size()) {
    const double v = b2[c];
    const bool in = v != 0.0 && finite(v);
    S.bnorm[c] = in ? std::sqrt(v) : 0.0, S.active[c] = in ? 1 : 0, S.flag[c] = (v == 0.0 || in) ? 0 : 1;
    S.iter[c] = 0, S.relres[c] = HUGE_VAL;
  }
  if (tm.rank() == 0) S.ctl[0] = 1, S.ctl[1] = S.ctl[2] = 0, S.ctl[3] = nc;
  tm.sync();
}

// A breakdown (a Cholesky's, or a next block of rank 0) ends the tile: every column of the block that was not <= rtol at
// its last test gets flag 1, all get the completed steps, and E1 = E2 = 0 so that the step's remaining passes change nothing.
// Mode 1, the start: G = R^H Z -> pivoted Cholesky S, rank r; E1 = I[:, piv] inv(S[:, piv]), E2 = 0, C = S.  r == 0 and not bad: every
// column is zero or excluded, the flags stay.  (Every mode leaves a tile that is over alone, and reads ctl before thread 0 may change it.)
template <class T, class Team>
HIFAMD_HD inline void start_factor(const Small<T> &S, const Work<T> &W, int s, const Team &tm) {
  if (S.ctl[0] == 0) return;
  tm.sync();
  const Chol f = factor_basis(S.G, s, S.deftol, W, S.E1, S.E2, tm);
  if (f.bad) return end_tile(S, S.relres, s, 1, 0, tm);
  if (f.r == 0) return set_state(S, 0, tm);
  stage(W.W2, S.C, f.r, s, tm);
  if (tm.rank() == 0) S.ctl[1] = S.ctl[2] = S.ctl[3] = f.r;
  tm.sync();
}

// Mode 2 of step k: Sigma = P^H A P (r x r) -> unpivoted Cholesky, alpha = Sigma^-1; E1 = alpha C diag(beta), E2 = alpha.
// A Sigma that is not positive definite is a breakdown after k - 1 steps.
template <class T, class Team>
HIFAMD_HD inline void step_alpha(const Small<T> &S, const Work<T> &W, int s, int k, const Team &tm) {
  if (S.ctl[0] == 0) return;
  tm.sync();
  const int r = S.ctl[3];
  clear(S.E1, tm);
  clear(S.E2, tm);
  stage(S.G, W.W1, r, r, tm);
  hermitize(W.W1, W.W2, r, tm);
  const Chol f = chol(W.W1, r, S.deftol, false, W.W2, W.piv, W.d, W.taken, tm);
  if (f.bad) return end_tile(S, S.relres, s, 1, k - 1, tm);
  tri_inv(W.W2, W.piv, f.r, W.W1, tm);
  matmul(W.W1, W.W1, true, f.r, f.r, f.r, (const double *)nullptr, W.W2, tm);  // alpha = Ti Ti^H
  stage(W.W2, S.E2, f.r, f.r, tm);
  times_C_beta(W.W2, f.r, f.r, s, S, W.W1, W.d, tm);
  if (tm.rank() == 0) S.ctl[2] = f.r;
  tm.sync();
}

// Mode 3 of step k: H = Q^H Q (r x r) -> relres_j = sqrt(c_j^H H c_j).  Every column of the block <= rtol: flag 0, k
// iterations; k == maxit: flag 0 / 2.  Otherwise the tile goes on.
template <class T, class Team>
HIFAMD_HD inline void step_test(const Small<T> &S, const Work<T> &W, int s, int k, const Team &tm) {
  if (S.ctl[0] == 0) return;
  tm.sync();
  const int r = S.ctl[3];
  stage(S.G, W.W1, r, r, tm);
  hermitize(W.W1, W.W2, r, tm);
  stage(S.C, W.W2, r, s, tm);
  quad_forms(W.W1, W.W2, r, s, S.G, S.relres, tm);
  bool all = true;
  for (int c = 0; c < s; ++c) all = all && (!S.active[c] || S.relres[c] <= S.rtol);
  if (all || k >= S.maxit) end_tile(S, S.relres, s, 2, k, tm);
}

// Mode 4 of step k: G = Q^H W (r x r) -> pivoted Cholesky S, rank r'; E1 = I[:, piv] inv(S[:, piv]), E2 = S^H, C <- S C,
// r <- r'.  A bad Gram or r' == 0 is a breakdown after k steps.
template <class T, class Team>
HIFAMD_HD inline void step_next(const Small<T> &S, const Work<T> &W, int s, int k, const Team &tm) {
  if (S.ctl[0] == 0) return;
  tm.sync();
  const int r = S.ctl[3];
  const Chol f = factor_basis(S.G, r, S.deftol, W, S.E1, S.E2, tm);
  if (f.bad || f.r == 0) return end_tile(S, S.relres, s, 1, k, tm);
  adjoint(W.W2, f.r, r, S.E2, tm);
  advance_C(W, f.r, r, s, S.C, S.G, tm);
  if (tm.rank() == 0) S.ctl[3] = f.r;
  tm.sync();
}

}  // namespace bcg
}  // namespace hifamd
