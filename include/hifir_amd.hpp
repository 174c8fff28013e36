// hifir_amd.hpp -- header-only C++11 facade over the C ABI (hifir_amd.h) that mirrors the apply-side
// interface of hif::HIF<ValueType, int, std::ptrdiff_t> (reference: src/hif/builder.hpp:107-513), so
// that header-only users of the reference keep their call sites:
//
//     hif::HIF<double> M;  M.factorize(A, params);          // host, unchanged (builder.hpp:264)
//     hifamd::HIF<double> G;  G.attach(M);  G.set_matrix(A); // once: hierarchy + matrix to HBM
//     G.solve(b, x);                                         // was M.solve(b, x)           :409-423
//     G.solve(b, x, true);                                   // was M.solve(b, x, true)     (prec_solve_tran)
//     G.solve_mrhs(B, X);                                    // was M.solve_mrhs(B, X)      :433-445
//     G.hifir(A, b, N, x);  G.hifir(A, b, N, betas, x);      // was M.hifir(...)            :459-489
//     G.mmultiply(x, y);                                     // was M.mmultiply(x, y)       :503-513
//
// Same names, argument meaning and defaults; errors are thrown as std::runtime_error carrying
// hifamd_last_error() (the reference built with HIF_THROW throws std::runtime_error too).  Array
// arguments are anything with data() and size() (hif::Array, std::vector, ...); multi-RHS blocks are
// arrays of std::array<T, Nrhs> like hif::Array<std::array<T, Nrhs>> (CompressedStorage.hpp:2127).
// Not thread-safe per object, like hif::HIF (mutable work space, builder.hpp:579).
#ifndef HIFIR_AMD_HPP
#define HIFIR_AMD_HPP

#include <array>
#include <complex>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "hifir_amd.h"

namespace hifamd {

namespace detail {
template <class T>
struct value_tag;
template <>
struct value_tag<double> {
  static HifAmdValueType value() { return HIFAMD_D; }
};
template <>
struct value_tag<std::complex<double>> {
  static HifAmdValueType value() { return HIFAMD_Z; }
};
inline void check(HifAmdStatus st) {
  if (st == HIFAMD_SUCCESS) return;
  const char *msg = hifamd_last_error();
  throw std::runtime_error(std::string("hifir_amd: ") + (msg ? msg : "error without message"));
}
inline std::int64_t rank_arg(std::size_t r) {  // size_type(-1) = full rank (builder.hpp:461)
  return r == static_cast<std::size_t>(-1) ? -1 : static_cast<std::int64_t>(r);
}
}  // namespace detail

template <class ValueType>
class HIF {
 public:
  typedef ValueType value_type;
  typedef std::size_t size_type;

  explicit HIF(int device = -1) : _h(nullptr), _device(device), _has_A(false), _has_B(false), _zop(0) {}
  ~HIF() { clear(); }
  HIF(const HIF &) = delete;
  HIF &operator=(const HIF &) = delete;
  HIF(HIF &&o) noexcept : _h(o._h), _device(o._device), _has_A(o._has_A), _has_B(o._has_B), _zop(o._zop) { o._h = nullptr; }

  /// Complex hierarchies: the explicit operators the next attach() asks for (HIFAMD_ZOP_TAIL | HIFAMD_ZOP_TOP,
  /// hifamd_set_complex_operators; 0, the default, keeps the plan complex handles always had).  They are planner options,
  /// fixed when the levels are imported: a hierarchy that is already attached keeps the ones it was attached with.
  void set_complex_operators(const int flags) { _zop = flags; }

  /// Ship the hierarchy of a factorized hif::HIF (or anything with the same precs() interface,
  /// alg/Prec.hpp:309-357) to HBM.  max_nrhs sizes the device work arena (wider batches are tiled).
  /// spd: Options::spd of the factorization (only read for is_symm hierarchies: truncation rule of SYEIG).
  template <class RefHif>
  void attach(const RefHif &M, const size_type max_nrhs = 64, const int spd = 0) {
    clear();
    detail::check(hifamd_create(detail::value_tag<value_type>::value(), _device, &_h));
    try {
      if (_zop) detail::check(hifamd_set_complex_operators(_h, _zop));
      for (auto itr = M.precs().cbegin(); itr != M.precs().cend(); ++itr) {
        const auto &p = *itr;
        // CCS accessors: ds/CompressedStorage.hpp:1910-1915; pointer type may be any integer
        const std::vector<std::int64_t> Lp(p.L_B.col_start().cbegin(), p.L_B.col_start().cend()),
            Up(p.U_B.col_start().cbegin(), p.U_B.col_start().cend()),
            Ep(p.E.col_start().cbegin(), p.E.col_start().cend()), Fp(p.F.col_start().cbegin(), p.F.col_start().cend());
        const std::vector<std::int32_t> Li(p.L_B.row_ind().cbegin(), p.L_B.row_ind().cend()),
            Ui(p.U_B.row_ind().cbegin(), p.U_B.row_ind().cend()), Ei(p.E.row_ind().cbegin(), p.E.row_ind().cend()),
            Fi(p.F.row_ind().cbegin(), p.F.row_ind().cend());
        const std::vector<std::int32_t> pp(p.p.cbegin(), p.p.cend()), pi(p.p_inv.cbegin(), p.p_inv.cend()),
            qq(p.q.cbegin(), p.q.cend()), qi(p.q_inv.cbegin(), p.q_inv.cend());
        const std::vector<double> ss(p.s.cbegin(), p.s.cend()), tt(p.t.cbegin(), p.t.cend());
        const std::int64_t F_ncols = static_cast<std::int64_t>(p.F.ncols());
        detail::check(hifamd_add_level(_h, (std::int64_t)p.m, (std::int64_t)p.n, Lp.data(), Li.data(), p.L_B.vals().data(),
                                       Up.data(), Ui.data(), p.U_B.vals().data(), Ep.data(), Ei.data(), p.E.vals().data(),
                                       F_ncols, F_ncols ? Fp.data() : nullptr, Fi.data(), p.F.vals().data(),
                                       p.d_B.data(), ss.data(), tt.data(), pp.data(), pi.data(), qq.data(), qi.data()));
        if (!p.dense_solver.empty()) {  // the UNFACTORED block, Prec::inquire_or_export_dense (Prec.hpp:275-293)
          const auto &D = p.dense_solver.mat_backup();
          if (std::strcmp(p.dense_solver.method(), "LUP") == 0)  // reference built with HIF_DENSE_MODE=0
            detail::check(hifamd_set_dense_lup(_h, (std::int64_t)D.nrows(), D.data()));
          else
            detail::check(hifamd_set_dense(_h, (std::int64_t)D.nrows(), D.data(), 0.0));
        } else if (!p.symm_dense_solver.empty()) {  // is_symm factorizations (symm_factor.hpp:654-657): SYEIG
          const auto &D = p.symm_dense_solver.mat_backup();
          detail::check(hifamd_set_dense_symm(_h, (std::int64_t)D.nrows(), D.data(), spd));
        }
      }
      detail::check(hifamd_finalize(_h, (std::int64_t)max_nrhs));
    } catch (...) {
      clear();
      throw;
    }
  }

  /// The matrix of the iterative-refinement / GMRES loops (0- or 1-based CRS, copied to HBM).
  void set_matrix(const size_type n, const std::int64_t *indptr, const std::int32_t *indices, const value_type *vals) {
    require();
    detail::check(hifamd_set_matrix(_h, (std::int64_t)n, indptr, indices, vals));
    _has_A = true;
  }
  /// ... from a hif::CRS-like object (row_start(), col_ind(), vals(); CompressedStorage.hpp:812-817)
  template <class Crs>
  void set_matrix(const Crs &A) {
    const std::vector<std::int64_t> ip(A.row_start().cbegin(), A.row_start().cend());
    const std::vector<std::int32_t> ci(A.col_ind().cbegin(), A.col_ind().cend());
    set_matrix(A.nrows(), ip.data(), ci.data(), A.vals().data());
  }

  // ---- queries (builder.hpp:136-199) --------------------------------------------------------------
  bool empty() const { return !_h; }
  size_type levels() const { return _h ? (size_type)hifamd_levels(_h) : 0u; }
  size_type nnz() const { return _h ? (size_type)hifamd_nnz(_h) : 0u; }
  size_type nrows() const { return _h ? (size_type)hifamd_nrows(_h) : 0u; }
  size_type ncols() const { return nrows(); }
  size_type schur_rank() const { return _h ? (size_type)hifamd_schur_rank(_h) : 0u; }
  size_type schur_size() const { return _h ? (size_type)hifamd_schur_size(_h) : 0u; }
  size_type rank() const { return empty() ? 0u : nrows() - (schur_size() - schur_rank()); }
  void clear() {
    if (_h) hifamd_destroy(_h);
    _h = nullptr;
    _has_A = _has_B = false;
  }
  HifAmdHdl handle() const { return _h; }  ///< for the device-pointer entry points of hifir_amd.h
  /// HIF::nsp / nsp_tran with NspFilter::set_nsp_const (NspFilter.hpp:118-125); start > end removes it
  void set_nsp_const(const size_type start = 0, const size_type end = static_cast<size_type>(-1), const bool trans = false) {
    require();
    detail::check(hifamd_set_nsp_const(_h, trans ? HIFAMD_SH : HIFAMD_S, (std::int64_t)start,
                                       end == static_cast<size_type>(-1) ? -1 : (std::int64_t)end));
  }
  /// Basis mode of the filter (the device form of NspFilter's user routine): V holds k vectors of nrows() entries one
  /// after the other (k = V.size() / nrows(), 1 <= k <= HIFAMD_NSP_MAX) that span the null space; every solve result x
  /// becomes x - Q (Q^H x).  An empty V removes it.
  template <class Array>
  void set_nsp_basis(const Array &V, const bool trans = false) {
    require();
    const size_type n = nrows(), k = n ? V.size() / n : 0u;
    if (k * n != V.size()) throw std::runtime_error("hifir_amd: a null-space basis holds k vectors of nrows() entries");
    std::vector<value_type> W(V.size());  // [n][k] row-interleaved, the layout of the C ABI
    for (size_type j = 0; j < k; ++j)
      for (size_type i = 0; i < n; ++i) W[i * k + j] = V.data()[j * n + i];
    detail::check(hifamd_set_nsp_basis(_h, trans ? HIFAMD_SH : HIFAMD_S, (std::int64_t)k, k ? W.data() : nullptr, (std::int64_t)k));
  }
  size_type nsp_dim(const bool trans = false) const {
    const std::int64_t k = _h ? hifamd_nsp_dim(_h, trans ? HIFAMD_SH : HIFAMD_S) : 0;
    return k > 0 ? (size_type)k : 0u;
  }
  /// Find the null space of the attached matrix (trans: of A^H) on the device (hifamd_nsp_find, device-generated
  /// probes of `seed`): returns the number of vectors found (at most kmax); Q receives them one after the other
  /// (found * nrows() entries, the layout set_nsp_basis takes); resid16 / info4 as in hifir_amd.h (may be null).
  /// install: they become the basis filter.
  size_type find_nullspace(std::vector<value_type> &Q, const size_type kmax = HIFAMD_NSP_MAX, const double tol = 1e-7,
                           const double rtol = 1e-10, const int restart = 30, const int maxit = 500, const bool trans = false,
                           const bool install = true, const std::uint64_t seed = 0u, const bool full_rank = false,
                           double *resid16 = nullptr, int *info4 = nullptr) {
    require();
    const size_type n = nrows(), kq = kmax ? kmax : 1u;
    std::vector<value_type> W(n * kq);  // [n][kmax] row-interleaved, the layout of the C ABI
    std::int64_t found = 0;
    detail::check(hifamd_nsp_find(_h, trans ? HIFAMD_SH : HIFAMD_S, (std::int64_t)kmax, tol, rtol, restart, maxit,
                                  full_rank ? -1 : 0, nullptr, 0, seed, install ? 1 : 0, &found, W.data(), (std::int64_t)kq,
                                  resid16, info4));
    Q.assign((size_type)found * n, value_type(0));
    for (size_type j = 0; j < (size_type)found; ++j)
      for (size_type i = 0; i < n; ++i) Q[j * n + i] = W[i * kq + j];
    return (size_type)found;
  }
  /// the orthonormal basis of the basis filter in force, nsp_dim(trans) vectors one after the other (empty: none)
  std::vector<value_type> nsp_basis(const bool trans = false) const {
    require();
    const size_type n = nrows(), k = nsp_dim(trans);
    std::vector<value_type> Q(k * n);
    if (!k) return Q;
    std::vector<value_type> W(k * n);
    if (hifamd_nsp_get_basis(_h, trans ? HIFAMD_SH : HIFAMD_S, W.data(), (std::int64_t)k) != (std::int64_t)k)
      throw std::runtime_error("hifir_amd: the null-space basis could not be read back");
    for (size_type j = 0; j < k; ++j)
      for (size_type i = 0; i < n; ++i) Q[j * n + i] = W[i * k + j];
    return Q;
  }
  /// the filter in force alone, in place, on one vector (what makes a right-hand side consistent)
  template <class Array>
  void nsp_filter(Array &x, const bool trans = false) const {
    require();
    if (x.size() != nrows()) throw std::runtime_error("hifir_amd: unmatched sizes");
    detail::check(hifamd_nsp_filter_batch(_h, trans ? HIFAMD_SH : HIFAMD_S, x.data(), 1, 1));
  }

  // ---- x = M^{-1} b / M^{-H} b (builder.hpp:409-423) ---------------------------------------------
  template <class RhsType, class SolType>
  void solve(const RhsType &b, SolType &x, const bool trans = false, const size_type r = 0u) const {
    require();
    if (b.size() != x.size()) throw std::runtime_error("hifir_amd: unmatched sizes");
    detail::check(hifamd_apply_batch(_h, trans ? HIFAMD_SH : HIFAMD_S, b.data(), 1, x.data(), 1, 1, 1, nullptr,
                                     detail::rank_arg(r), nullptr));
  }

  // ---- X = M^{-1} B, B and X arrays of std::array<T, Nrhs> (builder.hpp:433-445) -------------------
  template <class RhsBlock, class SolBlock>
  void solve_mrhs(const RhsBlock &b, SolBlock &x, const size_type r = 0u) const {
    require();
    typedef typename std::remove_cv<typename std::remove_reference<decltype(b.data()[0])>::type>::type row_type;
    const std::int64_t nrhs = (std::int64_t)std::tuple_size<row_type>::value;
    if (b.size() != x.size()) throw std::runtime_error("hifir_amd: unmatched sizes");
    detail::check(hifamd_solve_batch(_h, b.data(), nrhs, x.data(), nrhs, nrhs, detail::rank_arg(r)));
  }

  // ---- iterative refinement (builder.hpp:459-489).  A is the matrix handed to set_matrix(); when none
  //      was attached yet and A looks like a hif::CRS it is attached on the fly. -------------------------
  template <class Matrix, class RhsType, class SolType>
  void hifir(const Matrix &A, const RhsType &b, const size_type N, SolType &x, const bool trans = false,
             const size_type r = static_cast<size_type>(-1)) {
    ensure_matrix(A);
    detail::check(hifamd_apply_batch(_h, trans ? HIFAMD_SH : HIFAMD_S, b.data(), 1, x.data(), 1, 1, (int)N, nullptr,
                                     detail::rank_arg(r), nullptr));
  }
  template <class Matrix, class RhsType, class SolType>
  std::pair<size_type, int> hifir(const Matrix &A, const RhsType &b, const size_type N, const double *betas, SolType &x,
                                  const bool trans = false, const size_type r = static_cast<size_type>(-1)) {
    ensure_matrix(A);
    int st[2] = {0, 0};
    detail::check(hifamd_apply_batch(_h, trans ? HIFAMD_SH : HIFAMD_S, b.data(), 1, x.data(), 1, 1, (int)N, betas,
                                     detail::rank_arg(r), st));
    return std::make_pair((size_type)st[0], st[1]);
  }

  // ---- y = M x / M^H x (builder.hpp:503-513) ------------------------------------------------------
  template <class RhsType, class SolType>
  void mmultiply(const RhsType &x, SolType &y, const bool trans = false, const size_type r = 0u) const {
    require();
    if (y.size() != x.size()) throw std::runtime_error("hifir_amd: unmatched sizes");
    detail::check(hifamd_apply_batch(_h, trans ? HIFAMD_MH : HIFAMD_M, x.data(), 1, y.data(), 1, 1, 1, nullptr,
                                     detail::rank_arg(r), nullptr));
  }

  // ---- the example driver of examples/advanced/gmres.hpp:19-123 on the device (real or complex; Hermitian inner product) ----
  template <class Matrix, class ArrayType>
  std::tuple<ArrayType, int, int> gmres(const Matrix &A, const ArrayType &b, const int restart, const double rtol,
                                        const int maxit, const bool full_rank = false) {
    ensure_matrix(A);
    ArrayType x(b.size());
    int flag = 0, iters = 0;
    detail::check(hifamd_gmres_batch(_h, b.data(), 1, x.data(), 1, 1, restart, rtol, maxit, full_rank ? -1 : 0, &flag, &iters));
    return std::make_tuple(std::move(x), flag, iters);
  }

  // ---- extra-precise residuals (hifamd_set_residual_precision, hifamd_residual_batch, hifamd_gmres_ir_batch) ----
  // HIFAMD_RESID_COMPENSATED: hifir and the restart residuals of gmres form b - A x as if in twice the working precision.
  void set_residual_precision(const int mode) {
    require();
    detail::check(hifamd_set_residual_precision(_h, mode));
  }
  int residual_precision() const { return _h ? hifamd_residual_precision(_h) : -1; }
  /// r = b - A x (trans: b - A^H x); mode HIFAMD_RESID_WORKING / HIFAMD_RESID_COMPENSATED, -1: the handle's
  template <class Matrix, class RhsType, class SolType, class ResType>
  void residual(const Matrix &A, const RhsType &b, const SolType &x, ResType &r, const bool trans = false, const int mode = -1) {
    ensure_matrix(A);
    if (b.size() != x.size() || b.size() != r.size()) throw std::runtime_error("hifir_amd: unmatched sizes");
    detail::check(hifamd_residual_batch(_h, trans ? HIFAMD_SH : HIFAMD_S, b.data(), 1, x.data(), 1, r.data(), 1, 1, mode));
  }
  /// GMRES-based iterative refinement: (x, flag, corrections in x, inner GMRES iterations, compensated ||b - A x|| / ||b||);
  /// flag 0 converged, 1 stagnated, 2 reached max_outer
  template <class Matrix, class ArrayType>
  std::tuple<ArrayType, int, int, int, double> gmres_ir(const Matrix &A, const ArrayType &b, const int restart = 30,
                                                        const double rtol = 1e-14, const double inner_rtol = 1e-6,
                                                        const int max_outer = 10, const int inner_maxit = 500,
                                                        const bool full_rank = false) {
    ensure_matrix(A);
    ArrayType x(b.size());
    int flag = 0, outer = 0, iters = 0;
    double relres = 0.0;
    detail::check(hifamd_gmres_ir_batch(_h, b.data(), 1, x.data(), 1, 1, restart, rtol, inner_rtol, max_outer, inner_maxit,
                                        full_rank ? -1 : 0, &flag, &outer, &iters, &relres));
    return std::make_tuple(std::move(x), flag, outer, iters, relres);
  }

  // ---- preconditioned CG for a Hermitian positive-definite pair (A, M) on the device (hifamd_pcg_batch) ----
  // Needs an is_symm hierarchy: is_hermitian(); flag 0 converged, 1 breakdown, 2 reached maxit.
  template <class Matrix, class ArrayType>
  std::tuple<ArrayType, int, int> pcg(const Matrix &A, const ArrayType &b, const double rtol, const int maxit,
                                      const bool full_rank = false) {
    ensure_matrix(A);
    ArrayType x(b.size());
    int flag = 0, iters = 0;
    detail::check(hifamd_pcg_batch(_h, b.data(), 1, x.data(), 1, 1, rtol, maxit, full_rank ? -1 : 0, &flag, &iters));
    return std::make_tuple(std::move(x), flag, iters);
  }
  bool is_hermitian() const { return _h && hifamd_hermitian(_h) == 1; }

  // ---- breakdown-free block CG for a Hermitian positive-definite pair (A, M) on the device (hifamd_bcg_batch) ----
  // B and the returned X hold nrhs columns row-interleaved ([n][nrhs]); the columns of every tile of `block` <= 64 share one
  // block Krylov space.  -> (X, flags, iters, ranks): per column flag 0 converged, 1 breakdown or excluded, 2 reached maxit
  // and the steps of its tile; per tile its rank after the start and during its last step.
  template <class Matrix, class ArrayType>
  std::tuple<ArrayType, std::vector<int>, std::vector<int>, std::vector<int>> bcg(
      const Matrix &A, const ArrayType &B, const int nrhs, const int block, const double rtol, const int maxit,
      const double deftol = 1e-12, const bool full_rank = false) {
    ensure_matrix(A);
    if (nrhs < 1 || block < 1) throw std::runtime_error("hifir_amd: bcg needs nrhs >= 1 and block >= 1");
    ArrayType X(B.size());
    std::vector<int> flags(nrhs, 0), iters(nrhs, 0), ranks(2 * ((nrhs + block - 1) / block), 0);
    detail::check(hifamd_bcg_batch(_h, B.data(), nrhs, X.data(), nrhs, nrhs, block, rtol, deftol, maxit, full_rank ? -1 : 0,
                                   flags.data(), iters.data(), ranks.data()));
    return std::make_tuple(std::move(X), std::move(flags), std::move(iters), std::move(ranks));
  }

  // ---- restarted block GCR for a general pair (A, M) on the device (hifamd_bgcr_batch) ----
  // As bcg, with nothing asked of the hierarchy: the columns of every tile of `block` <= 64 share one block Krylov space,
  // restarted every `restart` <= HIFAMD_BGCR_MAX_RESTART steps; every flag 0 is decided on a true residual.
  // -> (X, flags, iters, ranks): per column flag 0 converged, 1 stagnated / bad Gram / excluded, 2 reached maxit and the
  // steps of its tile; per tile its rank after the start of its first cycle and during its last step.
  template <class Matrix, class ArrayType>
  std::tuple<ArrayType, std::vector<int>, std::vector<int>, std::vector<int>> bgcr(
      const Matrix &A, const ArrayType &B, const int nrhs, const int block, const int restart, const double rtol,
      const int maxit, const double deftol = 1e-12, const bool full_rank = false) {
    ensure_matrix(A);
    if (nrhs < 1 || block < 1) throw std::runtime_error("hifir_amd: bgcr needs nrhs >= 1 and block >= 1");
    ArrayType X(B.size());
    std::vector<int> flags(nrhs, 0), iters(nrhs, 0), ranks(2 * ((nrhs + block - 1) / block), 0);
    detail::check(hifamd_bgcr_batch(_h, B.data(), nrhs, X.data(), nrhs, nrhs, block, restart, rtol, deftol, maxit,
                                    full_rank ? -1 : 0, flags.data(), iters.data(), ranks.data()));
    return std::make_tuple(std::move(X), std::move(flags), std::move(iters), std::move(ranks));
  }

  // ---- LOBPCG: the nev smallest eigenpairs of the Hermitian matrix A, preconditioned by M (hifamd_lobpcg) ----
  // A block of k <= 16 candidates started from X0 ([n][k] row-interleaved) or, for an empty X0, from the generated block of
  // `seed`.  -> (lambda, X, res, flags, steps): lambda ascending, X [n][k] orthonormal, res_j = ||A x_j - lambda_j x_j|| /
  // ||A||_inf at the last test, per column flag 0 converged, 1 breakdown, 2 not converged at maxit.
  template <class Matrix, class ArrayType>
  std::tuple<std::vector<double>, ArrayType, std::vector<double>, std::vector<int>, int> lobpcg(
      const Matrix &A, const int k, const int nev, const ArrayType &X0, const double tol, const int maxit,
      const std::uint64_t seed = 0, const double deftol = 1e-12, const bool full_rank = false) {
    ensure_matrix(A);
    return lobpcg_call<ArrayType>(hifamd_lobpcg, "lobpcg", k, nev, X0, tol, maxit, seed, deftol, full_rank);
  }

  // ---- generalized LOBPCG: the nev smallest eigenpairs of A x = lambda B x (hifamd_lobpcg_gen) ----
  // B: the mass matrix (copied to HBM beside A by set_mass_matrix; lobpcg_gen sends it once per facade object).
  void set_mass_matrix(const size_type n, const std::int64_t *indptr, const std::int32_t *indices, const value_type *vals) {
    require();
    detail::check(hifamd_set_mass_matrix(_h, (std::int64_t)n, indptr, indices, vals));
    _has_B = true;
  }
  template <class Crs>
  void set_mass_matrix(const Crs &B) {
    const std::vector<std::int64_t> ip(B.row_start().cbegin(), B.row_start().cend());
    const std::vector<std::int32_t> ci(B.col_ind().cbegin(), B.col_ind().cend());
    set_mass_matrix(B.nrows(), ip.data(), ci.data(), B.vals().data());
  }
  // Arguments and returns of lobpcg; X comes back with X^H B X = I and res_j = ||A x_j - lambda_j B x_j|| /
  // ((||A||_inf + |lambda_j| ||B||_inf) ||x_j||).  No null-space filter may be in force.
  template <class Matrix, class ArrayType>
  std::tuple<std::vector<double>, ArrayType, std::vector<double>, std::vector<int>, int> lobpcg_gen(
      const Matrix &A, const Matrix &B, const int k, const int nev, const ArrayType &X0, const double tol, const int maxit,
      const std::uint64_t seed = 0, const double deftol = 1e-12, const bool full_rank = false) {
    ensure_matrix(A);
    if (!_has_B) set_mass_matrix(B);
    return lobpcg_call<ArrayType>(hifamd_lobpcg_gen, "lobpcg_gen", k, nev, X0, tol, maxit, seed, deftol, full_rank);
  }

  // ---- locked LOBPCG sweeps: up to 128 eigenpairs under a block of constraints (hifamd_eigs, hifamd_eig_project) ----
  // W <- W - Y (B Y)^H W in place: Y [n][m] (m <= 128, B-orthonormal columns), W [n][kw] (kw <= 16), both row-interleaved;
  // gen: B is the mass matrix of set_mass_matrix, else the identity.
  template <class ArrayType>
  void b_project(ArrayType &W, const int kw, const ArrayType &Y, const int m, const bool gen = false) {
    require();
    if (m < 1 || kw < 1 || (std::size_t)Y.size() != (std::size_t)nrows() * m || (std::size_t)W.size() != (std::size_t)nrows() * kw)
      throw std::runtime_error("hifir_amd: b_project needs Y of nrows() * m and W of nrows() * kw entries");
    detail::check(hifamd_eig_project(_h, gen ? 1 : 0, m, Y.data(), m, kw, W.data(), kw));
  }
  // The nev smallest eigenpairs of A (with a Matrix B: of the pencil A x = lambda B x) by sweeps of blocks of k <= 16
  // candidates with `guard` guard columns; Y ([n][m0], B-orthonormal, may be empty; m0 + nev <= 128) seeds the constraints,
  // X0 ([n][k], may be empty) the first sweep; maxit is per sweep.  -> (lambda, X, res, flags, info4): lambda in lock order,
  // X [n][nev], flags 0 locked / 1 breakdown / 2 not converged, info4 = {total steps, sweeps, locked, smallest basis rank}.
  template <class Matrix, class ArrayType>
  std::tuple<std::vector<double>, ArrayType, std::vector<double>, std::vector<int>, std::vector<int>> eigsh(
      const Matrix &A, const int nev, const int k, const int guard, const ArrayType &Y, const int m0, const ArrayType &X0,
      const double tol, const int maxit, const std::uint64_t seed = 0, const double deftol = 1e-12, const bool full_rank = false) {
    ensure_matrix(A);
    return eigs_call(false, nev, k, guard, Y, m0, X0, tol, maxit, seed, deftol, full_rank);
  }
  template <class Matrix, class ArrayType>
  std::tuple<std::vector<double>, ArrayType, std::vector<double>, std::vector<int>, std::vector<int>> eigsh(
      const Matrix &A, const Matrix &B, const int nev, const int k, const int guard, const ArrayType &Y, const int m0,
      const ArrayType &X0, const double tol, const int maxit, const std::uint64_t seed = 0, const double deftol = 1e-12,
      const bool full_rank = false) {
    ensure_matrix(A);
    if (!_has_B) set_mass_matrix(B);
    return eigs_call(true, nev, k, guard, Y, m0, X0, tol, maxit, seed, deftol, full_rank);
  }

  // ---- symmetric QMR for a Hermitian indefinite pair (A, M) on the device (hifamd_sqmr_batch) ----
  // Needs an is_symm hierarchy: is_hermitian(); neither A nor M has to be definite.  iters counts iterations (one apply
  // plus one SpMM each); flag 0 converged, 1 breakdown, 2 reached maxit.
  template <class Matrix, class ArrayType>
  std::tuple<ArrayType, int, int> sqmr(const Matrix &A, const ArrayType &b, const double rtol, const int maxit,
                                       const bool full_rank = false) {
    ensure_matrix(A);
    ArrayType x(b.size());
    int flag = 0, iters = 0;
    detail::check(hifamd_sqmr_batch(_h, b.data(), 1, x.data(), 1, 1, rtol, maxit, full_rank ? -1 : 0, &flag, &iters));
    return std::make_tuple(std::move(x), flag, iters);
  }

  // ---- right-preconditioned BiCGSTAB for a general pair (A, M) on the device (hifamd_bicgstab_batch) ----
  // iters counts steps (one apply plus one SpMM each); flag 0 converged, 1 breakdown, 2 reached maxit.
  template <class Matrix, class ArrayType>
  std::tuple<ArrayType, int, int> bicgstab(const Matrix &A, const ArrayType &b, const double rtol, const int maxit,
                                           const bool full_rank = false) {
    ensure_matrix(A);
    ArrayType x(b.size());
    int flag = 0, iters = 0;
    detail::check(
        hifamd_bicgstab_batch(_h, b.data(), 1, x.data(), 1, 1, rtol, maxit, full_rank ? -1 : 0, &flag, &iters));
    return std::make_tuple(std::move(x), flag, iters);
  }

  // ---- right-preconditioned IDR(s) for a general pair (A, M) on the device (hifamd_idrs_batch) ----
  // s: 1 .. HIFAMD_IDRS_MAX; the shadow block is generated from seed.  iters counts steps (one apply plus one SpMM each);
  // flag 0 converged, 1 breakdown, 2 reached maxit.
  template <class Matrix, class ArrayType>
  std::tuple<ArrayType, int, int> idrs(const Matrix &A, const ArrayType &b, const int s, const double rtol, const int maxit,
                                       const bool full_rank = false, const std::uint64_t seed = 0) {
    ensure_matrix(A);
    ArrayType x(b.size());
    int flag = 0, iters = 0;
    detail::check(hifamd_idrs_batch(_h, b.data(), 1, x.data(), 1, 1, s, nullptr, 0, seed, rtol, maxit, full_rank ? -1 : 0,
                                    &flag, &iters));
    return std::make_tuple(std::move(x), flag, iters);
  }

 private:
  // what lobpcg and lobpcg_gen share: the size checks (in the caller's name), the outputs, the call, the tuple
  template <class ArrayType, class Entry>
  std::tuple<std::vector<double>, ArrayType, std::vector<double>, std::vector<int>, int> lobpcg_call(
      Entry entry, const std::string &method, const int k, const int nev, const ArrayType &X0, const double tol, const int maxit,
      const std::uint64_t seed, const double deftol, const bool full_rank) {
    if (k < 1) throw std::runtime_error("hifir_amd: " + method + " needs k >= 1");
    if (X0.size() && (std::size_t)X0.size() != (std::size_t)nrows() * k)
      throw std::runtime_error("hifir_amd: " + method + " needs an empty X0 or one of nrows() * k entries");
    ArrayType X((std::size_t)nrows() * k);
    std::vector<double> lambda(k, 0.0), res(k, 0.0);
    std::vector<int> flags(k, 0);
    int info3[3] = {0, 0, 0};
    detail::check(entry(_h, k, nev, X0.size() ? X0.data() : nullptr, k, seed, tol, deftol, maxit, full_rank ? -1 : 0, lambda.data(),
                        X.data(), k, res.data(), flags.data(), info3));
    return std::make_tuple(std::move(lambda), std::move(X), std::move(res), std::move(flags), info3[0]);
  }
  template <class ArrayType>
  std::tuple<std::vector<double>, ArrayType, std::vector<double>, std::vector<int>, std::vector<int>> eigs_call(
      const bool gen, const int nev, const int k, const int guard, const ArrayType &Y, const int m0, const ArrayType &X0,
      const double tol, const int maxit, const std::uint64_t seed, const double deftol, const bool full_rank) {
    if (nev < 1 || k < 1 || m0 < 0) throw std::runtime_error("hifir_amd: eigsh needs nev >= 1, k >= 1 and m0 >= 0");
    if ((std::size_t)Y.size() != (std::size_t)nrows() * m0 || (X0.size() && (std::size_t)X0.size() != (std::size_t)nrows() * k))
      throw std::runtime_error("hifir_amd: eigsh needs Y of nrows() * m0 entries and an empty X0 or one of nrows() * k entries");
    ArrayType X((std::size_t)nrows() * nev);
    std::vector<double> lambda(nev, 0.0), res(nev, 0.0);
    std::vector<int> flags(nev, 0), info4(4, 0);
    detail::check(hifamd_eigs(_h, gen ? 1 : 0, nev, k, guard, m0 ? Y.data() : nullptr, m0, m0, X0.size() ? X0.data() : nullptr, k, seed,
                              tol, deftol, maxit, full_rank ? -1 : 0, lambda.data(), X.data(), nev, res.data(), flags.data(),
                              info4.data()));
    return std::make_tuple(std::move(lambda), std::move(X), std::move(res), std::move(flags), std::move(info4));
  }
  void require() const {
    if (!_h) throw std::runtime_error("hifir_amd: MILU-Prec is empty!");  // builder.hpp:412
  }
  template <class Matrix>
  void ensure_matrix(const Matrix &A) {
    require();
    if (!_has_A) set_matrix(A);
  }

  HifAmdHdl _h;
  int _device;
  bool _has_A, _has_B;
  int _zop;  // set_complex_operators: applied by attach()
};

}  // namespace hifamd

#endif  // HIFIR_AMD_HPP
