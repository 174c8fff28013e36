"""CPU: the symmetric QMR driver (hifamd_sqmr_batch / HIF.sqmr) without a GPU -- its two Hermitian indefinite fixtures load,
import and pass the Hermitian test; a numpy restatement of the recurrence around the oracle's apply (lockstep_edges_util.sqmr_restated,
shared with test_gpu_sqmr.py) converges on them where the PCG restatement breaks down; every stopping decision the GPU
test compares iteration counts on keeps a margin; and the entry points refuse a NULL handle and an unfinalized
hierarchy (no CPU fallback)."""
import numpy as np
import pytest
import scipy.sparse as sp

import hifir_amd
from hifir_amd._lib import lib
import lockstep_edges_util
from lockstep_edges_util import sqmr_restated  # noqa: F401  (test_gpu_sqmr.py takes it from here)
from oracle import orc
from util import load_hier

INDEFINITE = ("shift2d_32_symm", "kktr_24_symm")
RTOLS = (1e-6, 1e-10)
MAXIT = 300
# the projected comparison (twobody_symm): at 1e-6 the restatement's |s| / |b| on bstar passes 1.013 rtol one iteration
# before it stops, inside the margin below, so that tolerance is not used for a count comparison there
PROJ_RTOLS = (1e-8, 1e-10)
MARGIN = 1.02  # the last two ||s|| / ||b|| of every compared column lie outside [rtol / MARGIN, MARGIN * rtol]


def pcg_restated(solve, A, b, rtol, maxit):
    """PCG's flag and iterations for one column (lockstep_edges_util.pcg_restated: a non-positive or non-finite p^H A p or
    r^H M^{-1} r is a breakdown, flag 1)."""
    X, fl, it = lockstep_edges_util.pcg_restated(solve, A, b, rtol, maxit)
    return int(fl[0]), int(it[0])


def matrix(d):
    n = len(d["b"])
    return sp.csr_matrix((d["A_vals"], d["A_indices"], d["A_indptr"]), shape=(n, n))


def columns(d, A):
    """[random, zeros, the fixture's b, A 1, 1e-30 x random]: the columns of test_gpu_sqmr.py's comparison"""
    n = len(d["b"])
    rng = np.random.default_rng(5)
    return np.stack([rng.uniform(-1, 1, n), np.zeros(n), d["b"], A @ np.ones(n), 1e-30 * rng.uniform(-1, 1, n)], axis=1)


def margins(hist, rtol):
    """for every column that iterated: (last two |s| / |b|) / rtol"""
    return [[v / rtol for v in h[-2:]] for h in hist if h]


def assert_margin(hist, rtol, what):
    for c, m in enumerate(margins(hist, rtol)):
        for v in m:
            assert not (1.0 / MARGIN <= v <= MARGIN), (what, rtol, c, m)


def _import(levels):
    """add_level / set_dense* as HIF.from_levels does, without finalize (no GPU needed)."""
    M = hifir_amd.HIF(np.float64)
    for lv in levels:
        M.add_level(lv)
    last = levels[-1]
    assert int(last.get("dense_n", 0)) > 0 and int(last.get("dense_symm", 0))
    M.set_dense_symm(last["dense"], int(last.get("spd", 0)))
    return M


_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        levels, d = load_hier(name)
        _CACHE[name] = (levels, d, orc.Oracle(levels), matrix(d))
    return _CACHE[name]


@pytest.mark.parametrize("name", INDEFINITE)
def test_fixtures_load_import_and_are_hermitian(name):
    levels, d, O, A = fixture(name)
    assert len(levels) == 2 and int(levels[-1]["dense_symm"]) == 1
    assert abs(A - A.T).max() == 0.0
    w = np.linalg.eigvalsh(A.toarray())
    assert (w < 0).sum() == {"shift2d_32_symm": 20, "kktr_24_symm": 150}[name]
    M = _import(levels)
    assert M.is_hermitian()
    assert lib().hifamd_hermitian(M._h) == 1


@pytest.mark.parametrize("rtol", RTOLS)
@pytest.mark.parametrize("name", INDEFINITE)
def test_restatement_converges_with_a_margin(name, rtol):
    levels, d, O, A = fixture(name)
    B = columns(d, A)
    hist = []
    X, fl, it = sqmr_restated(O.solve, A, B, rtol, MAXIT, hist)
    print(name, rtol, "iters", it.tolist(), "margins", margins(hist, rtol))
    assert fl.tolist() == [0] * 5 and it[1] == 0 and not np.any(X[:, 1])
    for c in (0, 2, 3, 4):
        assert 1 < it[c] <= 40
        assert np.linalg.norm(B[:, c] - A @ X[:, c]) / np.linalg.norm(B[:, c]) <= rtol, c
    assert_margin(hist, rtol, name)


def complex_case():
    """shift2d_32_symm under the diagonal unitary similarity of test_gpu_pcg._phase_similarity: (complex levels, complex
    matrix, phases, the real block B, the genuinely complex block Bz) of test_gpu_sqmr.py's complex comparison"""
    from test_gpu_pcg import _phase_similarity

    levels, d, O, A = fixture("shift2d_32_symm")
    lz, Az, phi = _phase_similarity(levels, A)
    n = A.shape[0]
    rng = np.random.default_rng(23)
    B = np.stack([d["b"], rng.uniform(-1, 1, n)], axis=1)
    Bz = np.stack([phi * d["b"], rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n), np.zeros(n, dtype=np.complex128)], axis=1)
    return lz, Az, phi, B, Bz


def projected_case():
    """twobody_symm with its null-space basis: (levels, data, A, Q orthonormal, the filtered apply, P [bstar, b])"""
    levels, d, O, A = fixture("twobody_symm")
    Q = np.linalg.qr(d["V"])[0]

    def proj(X):
        return X - Q @ (Q.conj().T @ X)

    return levels, d, A, Q, (lambda r: proj(O.solve(r))), proj(np.stack([d["bstar"], d["b"]], axis=1))


def test_margin_of_the_other_compared_columns():
    # (the 70-column batch of the GPU test is compared with other GPU runs only, bit for bit: no margin is needed there)
    # the SPD pair of the comparison
    levels, d, O, A = fixture("p2d_32_symm")
    for rtol in RTOLS:
        hist = []
        X, fl, it = sqmr_restated(O.solve, A, columns(d, A), rtol, MAXIT, hist)
        assert fl.tolist() == [0] * 5
        assert_margin(hist, rtol, "p2d_32_symm")
    # the complex Hermitian indefinite pair: the similarity keeps the counts, and the complex columns
    levels, d, O, A = fixture("shift2d_32_symm")
    lz, Az, phi, B, Bz = complex_case()
    Oz = orc.Oracle(lz)
    hist = []
    X, fl, it = sqmr_restated(O.solve, A, B, 1e-10, MAXIT, hist)
    Xz, flz, itz = sqmr_restated(Oz.solve, Az, phi[:, None] * B, 1e-10, MAXIT, hist)
    assert fl.tolist() == flz.tolist() == [0, 0] and it.tolist() == itz.tolist()
    assert np.abs(Xz - phi[:, None] * X).max() / np.abs(X).max() <= 1e-10
    X, fl, it = sqmr_restated(Oz.solve, Az, Bz, 1e-10, MAXIT, hist)
    assert fl.tolist() == [0, 0, 0]
    assert_margin(hist, 1e-10, "shift2d_32_symm complex")
    # the projected iteration
    levels, d, A, Q, solve, PB = projected_case()
    for rtol in PROJ_RTOLS:
        hist = []
        X, fl, it = sqmr_restated(solve, A, PB, rtol, MAXIT, hist)
        assert fl.tolist() == [0, 0]
        assert np.abs(Q.T @ X).max() <= 1e-10 * np.linalg.norm(X, axis=0).min()
        assert_margin(hist, rtol, "twobody_symm projected")


@pytest.mark.parametrize("name", INDEFINITE)
def test_pcg_breaks_down_where_sqmr_converges(name):
    levels, d, O, A = fixture(name)
    b = columns(d, A)[:, 0]
    flag, it = pcg_restated(O.solve, A, b, 1e-6, MAXIT)
    assert flag == 1 and it <= 3, (flag, it)
    x, fl, its = sqmr_restated(O.solve, A, b, 1e-6, MAXIT)
    assert fl.tolist() == [0]


def test_sqmr_has_no_cpu_fallback():
    levels, d, O, A = fixture("shift2d_32_symm")
    M = _import(levels)
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.sqmr(d["b"])  # not finalized: never a CPU result
    assert e.value.code == 3
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.sqmr(np.stack([d["b"], d["b"]], axis=1), rtol=1e-8, maxit=4)
    assert e.value.code == 3


def test_null_handle():
    fl = np.zeros(1, dtype=np.int32)
    it = np.zeros(1, dtype=np.int32)
    b = np.ones(4)
    x = np.zeros(4)
    for name in ("hifamd_sqmr_batch", "hifamd_sqmr_batch_dev"):
        st = getattr(lib(), name)(None, b.ctypes.data, 1, x.ctypes.data, 1, 1, 1e-6, 10, 0, fl.ctypes.data, it.ctypes.data)
        assert st == 1, (name, st)  # HIFAMD_NULL_OBJ


def test_symbols_declared_exported_and_typed():
    import ctypes
    import os
    import re

    from hifir_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "hifir_amd.h")).read()
    declared = set(re.findall(r"\b(hifamd_\w+)\s*\(", hdr))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("hifamd_sqmr_batch", "hifamd_sqmr_batch_dev"):
        assert name in declared and hasattr(L, name) and name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("sqmr", "pcg")], name  # the signature of the PCG pair


def test_cpp_facade_sqmr_compiles(tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sqmr_facade.cpp"
    src.write_text(r'''
#include <complex>
#include <tuple>
#include <vector>
#include "hifir_amd.hpp"
template <class V>
struct MockCrs {
  std::vector<long> rs{0};
  std::vector<int> ci;
  std::vector<V> v;
  const std::vector<long>& row_start() const { return rs; }
  const std::vector<int>& col_ind() const { return ci; }
  const std::vector<V>& vals() const { return v; }
  size_t nrows() const { return 0; }
};
template <class V>
int run() {
  hifamd::HIF<V> G;
  MockCrs<V> A;
  std::vector<V> b(4);
  if (false) {
    auto out = G.sqmr(A, b, 1e-6, 100);
    auto out2 = G.sqmr(A, b, 1e-6, 100, true);
    std::vector<V> x = std::get<0>(out);
    return std::get<1>(out) + std::get<2>(out2) + (int)x.size();
  }
  return 0;
}
int main() { return run<double>() + run<std::complex<double>>(); }
''')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(root, "include"), str(src)])
