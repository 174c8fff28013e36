// The small-matrix arithmetic of the block CG driver (Engine::bcg_tile, k_bcg_small in kernels.hip.hpp): Hermitian Grams of
// at most 64 x 64, their pivoted / unpivoted Cholesky factors, triangular inverses and the products and quadratic forms around
// them.  Plain C++17, no HIP include: the one-workgroup kernel and host programs built with g++
// (tests/cpp/blockcg_small_test.cpp) run the same code.
//
// Every matrix is row-major with the row stride kLd = 64, whatever its size.  T is double or a struct {double x, y}.
// A function is called by every thread of a team: Team gives rank() (0 .. size() - 1), size() and sync() (a barrier that also
// publishes memory; Serial is the host's team of one).  Every output element is computed by one thread with its sums in a
// fixed order, so the result does not depend on the team's size.  A function ends with a barrier unless it says otherwise.
#pragma once
#include <cmath>
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

}  // namespace bcg
}  // namespace hifamd
