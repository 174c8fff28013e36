"""CPU: the basis mode of the null-space filter (hifamd_set_nsp_basis / hifamd_nsp_dim / hifamd_nsp_filter_batch /
_dev, HIF.set_nsp_basis / nsp_dim / nsp_filter, the C++ facade's methods) is declared, exported and typed; its
refusals come in the documented order and never produce a CPU result; the host orthonormalization (import.hpp
nsp_orthonormalize) runs clean under ASan + UBSan (tests/cpp/nsp_basis_test.cpp)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hifir_amd
from hifir_amd import _lib
from hifir_amd._lib import lib
from util import load_hier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hifamd_set_nsp_basis", "hifamd_nsp_dim", "hifamd_nsp_filter_batch", "hifamd_nsp_filter_batch_dev")
NULL_OBJ, MISMATCHED_SIZES, BAD_PREC, HIFIR_ERROR = 1, 2, 3, 4
OP_S, OP_SH, OP_M, OP_MH = 0, 1, 2, 3


def test_symbols_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "hifir_amd.h")).read()
    declared = set(re.findall(r"\b(hifamd_\w+)\s*\(", hdr))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define\s+HIFAMD_NSP_MAX\s+16\b", hdr)
    vp, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert _lib.SIGNATURES["hifamd_set_nsp_basis"] == (i, [vp, i, i64, vp, i64])
    assert _lib.SIGNATURES["hifamd_nsp_dim"] == (i64, [vp, i])
    assert _lib.SIGNATURES["hifamd_nsp_filter_batch"] == (i, [vp, i, vp, i64, i64])
    assert _lib.SIGNATURES["hifamd_nsp_filter_batch_dev"] == (i, [vp, i, vp, i64, i64, vp])
    # the shim's extension header keeps its 16 entry points: libhifir's C API has no filter entry to map onto
    ext = open(os.path.join(ROOT, "include", "libhifir_amd_ext.h")).read()
    assert "nsp" not in ext.lower()


def test_null_handle():
    v = np.ones((4, 1))
    assert lib().hifamd_set_nsp_basis(None, OP_S, 1, v.ctypes.data, 1) == NULL_OBJ
    assert lib().hifamd_nsp_dim(None, OP_S) == -1
    assert lib().hifamd_nsp_filter_batch(None, OP_S, v.ctypes.data, 1, 1) == NULL_OBJ
    assert lib().hifamd_nsp_filter_batch_dev(None, OP_S, v.ctypes.data, 1, 1, None) == NULL_OBJ


def _import(name):
    """add_level / set_dense* as HIF.from_levels does, without finalize (no GPU needed)."""
    levels, d = load_hier(name)
    M = hifir_amd.HIF(np.float64)
    for lv in levels:
        M.add_level(lv)
    last = levels[-1]
    if int(last.get("dense_n", 0)) > 0:
        if int(last.get("dense_symm", 0)):
            M.set_dense_symm(last["dense"], int(last.get("spd", 0)))
        else:
            M.set_dense(last["dense"])
    return M, d


@pytest.mark.parametrize("name", ["neu2d_32_symm", "twobody_symm", "pcd2d_32"])
def test_fixture_is_what_the_issue_describes(name):
    """The committed fixtures: A V = 0 (and A^T VL = 0), bstar = A xstar, the symmetric two pass the Hermitian test."""
    import scipy.sparse as sp

    M, d = _import(name)
    n = len(d["b"])
    A = sp.csr_matrix((d["A_vals"], d["A_indices"], d["A_indptr"]), shape=(n, n))
    V = d["V"]
    assert V.shape == (n, {"neu2d_32_symm": 1, "twobody_symm": 2, "pcd2d_32": 1}[name])
    scale = np.abs(A.data).max()
    assert np.abs(A @ V).max() <= 1e-14 * scale
    assert np.array_equal(d["bstar"], A @ d["xstar"]) and np.abs(d["xstar"]).max() < 1.0
    assert n == {"neu2d_32_symm": 1024, "twobody_symm": 976, "pcd2d_32": 1024}[name] == M.nrows()
    assert int(d["nlevels"]) == 2
    if name == "pcd2d_32":
        assert np.abs(A.T @ d["VL"]).max() <= 1e-14 * scale
        assert not M.is_hermitian()
        assert M.schur_size() == 62
    else:
        assert M.is_hermitian()
        assert M.schur_size() == 27
    if name == "neu2d_32_symm":
        assert abs(d["x_nspc"].mean()) <= 1e-14 * np.abs(d["x_nspc"]).max()


def test_refusals_in_order_without_a_gpu():
    """Bad op, k out of range, NULL V and ldv < k are MISMATCHED_SIZES before the handle's state is looked at; an
    unfinalized handle is BAD_PREC; nothing returns a CPU result."""
    M, d = _import("twobody_symm")
    V = np.ascontiguousarray(d["V"])
    n, k = V.shape
    h = M._h
    V17 = np.ones((n, 17))
    for op in (OP_M, OP_MH, 7, -1):
        assert lib().hifamd_set_nsp_basis(h, op, k, V.ctypes.data, k) == MISMATCHED_SIZES, op
        assert "HIFAMD_S" in lib().hifamd_last_error().decode()
    assert lib().hifamd_set_nsp_basis(h, OP_S, -1, V.ctypes.data, k) == MISMATCHED_SIZES
    assert lib().hifamd_set_nsp_basis(h, OP_S, 17, V17.ctypes.data, 17) == MISMATCHED_SIZES
    assert "16" in lib().hifamd_last_error().decode()
    assert lib().hifamd_set_nsp_basis(h, OP_S, k, None, k) == MISMATCHED_SIZES
    assert lib().hifamd_set_nsp_basis(h, OP_SH, k, V.ctypes.data, k - 1) == MISMATCHED_SIZES
    # in range, but the handle is not finalized
    for op in (OP_S, OP_SH):
        assert lib().hifamd_set_nsp_basis(h, op, k, V.ctypes.data, k) == BAD_PREC
        assert "finalize" in lib().hifamd_last_error().decode()
        assert lib().hifamd_set_nsp_basis(h, op, 0, None, 0) == BAD_PREC
        assert lib().hifamd_nsp_dim(h, op) == 0
    assert lib().hifamd_nsp_dim(h, OP_M) == 0
    X = np.ascontiguousarray(d["bstar"]).copy()
    X0 = X.copy()
    assert lib().hifamd_nsp_filter_batch(h, OP_M, X.ctypes.data, 1, 1) == MISMATCHED_SIZES
    assert lib().hifamd_nsp_filter_batch(h, OP_S, X.ctypes.data, 1, 1) == BAD_PREC
    assert lib().hifamd_nsp_filter_batch_dev(h, OP_S, X.ctypes.data, 1, 1, None) == BAD_PREC
    assert np.array_equal(X, X0)
    # the Python class: same codes, and wrong shapes are refused before the library is called
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.set_nsp_basis(V)
    assert e.value.code == BAD_PREC
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.set_nsp_basis(V17)
    assert e.value.code == MISMATCHED_SIZES
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.set_nsp_basis(V[:-1])
    assert e.value.code == MISMATCHED_SIZES
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.nsp_filter(X)
    assert e.value.code == BAD_PREC
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.nsp_filter(X[:-1].copy())
    assert e.value.code == MISMATCHED_SIZES
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.nsp_filter(X.astype(np.float32))
    assert e.value.code == MISMATCHED_SIZES
    assert M.nsp_dim() == 0 and M.nsp_dim(trans=True) == 0
    if lib().hifamd_device_count() == 0:
        with pytest.raises(hifir_amd.HifAmdError) as e:
            M.finalize(1)
        assert e.value.code == HIFIR_ERROR and "no CPU fallback" in e.value.msg
        with pytest.raises(hifir_amd.HifAmdError):
            M.set_nsp_basis(V)
        with pytest.raises(hifir_amd.HifAmdError):
            M.nsp_filter(X)
        assert np.array_equal(X, X0)


def test_stats_ext_reports_the_basis_bytes():
    M, d = _import("neu2d_32_symm")
    se = M.stats_ext()
    assert list(se)[22] == "nsp_basis_bytes" and se["nsp_basis_bytes"] == 0.0
    # (slots 23-25 are ls_stats(); the component-band counts of slots 26 / 27 follow the 23 keys, zero before finalize)
    assert list(se)[23:] == ["cd_components", "cd_shared_workgroups"] and len(se) == 25
    assert se["cd_components"] == 0.0 and se["cd_shared_workgroups"] == 0.0


def test_cpp_facade_nsp_basis_compiles(tmp_path):
    src = tmp_path / "nsp_facade.cpp"
    src.write_text(r'''
#include <complex>
#include <vector>
#include "hifir_amd.hpp"
template <class V>
int run() {
  hifamd::HIF<V> G;
  std::vector<V> basis(8), x(4);
  if (false) {
    G.set_nsp_basis(basis);
    G.set_nsp_basis(basis, true);
    G.set_nsp_basis(std::vector<V>());
    G.nsp_filter(x);
    G.nsp_filter(x, true);
    const hifamd::HIF<V> &C = G;
    return (int)C.nsp_dim() + (int)C.nsp_dim(true);
  }
  static_assert(HIFAMD_NSP_MAX == 16, "HIFAMD_NSP_MAX");
  return 0;
}
int main() { return run<double>() + run<std::complex<double>>(); }
''')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])
    # the C header alone, as C
    csrc = tmp_path / "nsp_c.c"
    csrc.write_text('#include "hifir_amd.h"\nint f(HifAmdHdl h, double *v) { return (int)hifamd_set_nsp_basis(h, HIFAMD_S, 1, v, 1)'
                    ' + (int)hifamd_nsp_dim(h, HIFAMD_SH) + (int)hifamd_nsp_filter_batch(h, HIFAMD_S, v, 1, 1)'
                    ' + (int)hifamd_nsp_filter_batch_dev(h, HIFAMD_S, v, 1, 1, 0) + HIFAMD_NSP_MAX; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(csrc)])


def test_host_orthonormalization_under_sanitizers(tmp_path):
    """import.hpp nsp_orthonormalize under ASan + UBSan: Q^H Q = I to 1e-12 for k = 1, 3, 16, real and complex, strides
    ldv > k, span(Q) = span(V); duplicated / zero / non-finite vectors refused by index (tests/cpp/nsp_basis_test.cpp)."""
    exe = str(tmp_path / "nsp_basis_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "hifir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "nsp_basis_test.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "nsp_basis_test -> ok" in r.stderr
