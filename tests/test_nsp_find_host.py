"""CPU: the null-space search (hifamd_nsp_find / hifamd_nsp_get_basis, HIF.find_nullspace / nsp_basis, the C++ facade's
methods) is declared, exported and typed; its refusals come in the documented order and never produce a CPU result; the
host steps between its device passes (import.hpp nsp_find_rotation / nsp_chol_inverse) run clean under ASan + UBSan
(tests/cpp/nsp_find_test.cpp), and the host twin of the probe generator equals the header's formula restated in numpy
bit for bit."""
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
NAMES = ("hifamd_nsp_find", "hifamd_nsp_get_basis")
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
    vp, i64, i, d, u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_uint64
    assert _lib.SIGNATURES["hifamd_nsp_find"] == (i, [vp, i, i64, d, d, i, i, i64, vp, i64, u64, i, vp, vp, i64, vp, vp])
    assert _lib.SIGNATURES["hifamd_nsp_get_basis"] == (i64, [vp, i, vp, i64])
    # the shim's extension header keeps its entry points: libhifir's C API has nothing to map the search onto
    ext = open(os.path.join(ROOT, "include", "libhifir_amd_ext.h")).read()
    assert "nsp" not in ext.lower()
    # the header states the generator and the relation of the two tolerances
    for needle in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "sigma_min+", "rtol sqrt(n / k)"):
        assert needle in hdr, needle


def _import(name, dtype=np.float64):
    """add_level / set_dense* as HIF.from_levels does, without finalize (no GPU needed)."""
    levels, d = load_hier(name)
    M = hifir_amd.HIF(dtype)
    for lv in levels:
        M.add_level(lv)
    last = levels[-1]
    if int(last.get("dense_n", 0)) > 0:
        if int(last.get("dense_symm", 0)):
            M.set_dense_symm(last["dense"], int(last.get("spd", 0)))
        else:
            M.set_dense(last["dense"])
    return M, d


def _find(h, op=OP_S, kmax=16, tol=1e-7, rtol=1e-10, restart=30, maxit=500, rank=0, X0=None, ldx0=16, seed=0, install=1,
          found=True, Q=None, ldq=16, resid=None, info=None):
    f = ctypes.c_int64(-7)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    st = lib().hifamd_nsp_find(h, op, kmax, tol, rtol, restart, maxit, rank, p(X0), ldx0, seed, install,
                               ctypes.byref(f) if found else None, p(Q), ldq, p(resid), p(info))
    return st, f.value


def test_null_handle():
    assert _find(None)[0] == NULL_OBJ
    assert _find(None, op=OP_M, kmax=0)[0] == NULL_OBJ  # before every other refusal
    q = np.zeros((4, 1))
    assert lib().hifamd_nsp_get_basis(None, OP_S, q.ctypes.data, 1) == -1
    assert lib().hifamd_nsp_get_basis(None, OP_SH, None, 0) == -1


@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_refusals_in_order_without_a_gpu(dtype):
    """Bad op, kmax, tol, rtol, restart, maxit, ldx0, ldq and a NULL `found` are MISMATCHED_SIZES before the handle's
    state is looked at -- each one with every later argument bad as well, so the order is what is tested; an unfinalized
    handle is BAD_PREC; nothing is written and nothing returns a CPU result."""
    M, d = _import("twobody_symm", dtype)
    h = M._h
    n = M.nrows()
    X0 = np.ones((n, 16), dtype=dtype)
    Q = np.full((n, 16), 5.0, dtype=dtype)
    resid = np.full(16, 5.0)
    info = np.full(4, 5, dtype=np.int32)
    nan = float("nan")
    # one bad argument at a time: the message names it
    cases = [
        (dict(op=OP_M), "HIFAMD_S"), (dict(op=OP_MH), "HIFAMD_S"), (dict(op=7), "HIFAMD_S"), (dict(op=-1), "HIFAMD_S"),
        (dict(kmax=0), "kmax"), (dict(kmax=-3), "kmax"), (dict(kmax=17), "kmax"),
        (dict(tol=0.0), "tol"), (dict(tol=-1e-8), "tol"), (dict(tol=nan), "tol"),
        (dict(rtol=0.0), "rtol"), (dict(rtol=nan), "rtol"),
        (dict(restart=0), "restart"), (dict(maxit=0), "maxit"),
        (dict(X0=X0, ldx0=15), "probe"), (dict(Q=Q, ldq=15), "basis output"), (dict(Q=Q, kmax=3, ldq=2), "basis output"),
        (dict(found=False), "found"),
    ]
    for kw, needle in cases:
        st, f = _find(h, **kw)
        assert st == MISMATCHED_SIZES, kw
        assert needle in lib().hifamd_last_error().decode(), kw
        assert f == -7 or not kw.get("found", True)
    # the order: everything from position i on is bad, the message is position i's
    chain = [("op", OP_M, "HIFAMD_S"), ("kmax", 17, "kmax"), ("tol", 0.0, "tol"), ("restart", 0, "restart"),
             ("ldx0", 3, "probe"), ("ldq", 1, "basis output"), ("found", False, "found")]
    for i in range(len(chain)):
        kw = dict(X0=X0, Q=Q)
        for key, bad, _ in chain[i:]:
            kw[key] = bad
        if "kmax" not in kw:
            kw["kmax"] = 4  # (ldq = 1 < kmax)
        st, _ = _find(h, **kw)
        assert st == MISMATCHED_SIZES, chain[i][0]
        assert chain[i][2] in lib().hifamd_last_error().decode(), chain[i][0]
    # ldq is only looked at when Q is given, ldx0 only when X0 is: a well-formed call on an unfinalized handle
    for op in (OP_S, OP_SH):
        st, f = _find(h, op=op, ldx0=0, ldq=0, resid=resid, info=info)
        assert st == BAD_PREC and f == 0
        assert "finalize" in lib().hifamd_last_error().decode()
        st, f = _find(h, op=op, X0=X0, Q=Q, resid=resid, info=info, kmax=16)
        assert st == BAD_PREC and f == 0
        assert lib().hifamd_nsp_dim(h, op) == 0
        assert lib().hifamd_nsp_get_basis(h, op, Q.ctypes.data, 16) == 0
    assert lib().hifamd_nsp_get_basis(h, OP_M, Q.ctypes.data, 16) == 0
    assert np.all(Q == 5.0) and np.all(resid == 5.0) and np.all(info == 5)
    # the Python class: same codes, and a wrong probe block is refused before the library is called
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.find_nullspace()
    assert e.value.code == BAD_PREC
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.find_nullspace(kmax=17)
    assert e.value.code == MISMATCHED_SIZES
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.find_nullspace(tol=0.0)
    assert e.value.code == MISMATCHED_SIZES
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.find_nullspace(X0=X0[:, :8])
    assert e.value.code == MISMATCHED_SIZES
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.find_nullspace(X0=X0[:-1])
    assert e.value.code == MISMATCHED_SIZES
    assert M.nsp_basis() is None and M.nsp_basis(trans=True) is None
    if lib().hifamd_device_count() == 0:
        # matrix-less and device-less: the matrix cannot be attached before finalize, finalize has no device
        with pytest.raises(hifir_amd.HifAmdError) as e:
            M.set_matrix(d["A_indptr"], d["A_indices"], d["A_vals"])
        assert e.value.code == BAD_PREC
        with pytest.raises(hifir_amd.HifAmdError) as e:
            M.finalize(16)
        assert e.value.code == HIFIR_ERROR and "no CPU fallback" in e.value.msg
        with pytest.raises(hifir_amd.HifAmdError) as e:
            M.find_nullspace()
        assert e.value.code == BAD_PREC
        assert M.nsp_basis() is None


def test_cpp_facade_nsp_find_compiles(tmp_path):
    src = tmp_path / "nsp_find_facade.cpp"
    src.write_text(r'''
#include <complex>
#include <vector>
#include "hifir_amd.hpp"
template <class V>
int run() {
  hifamd::HIF<V> G;
  std::vector<V> Q;
  double resid[16];
  int info[4];
  if (false) {
    std::size_t k = G.find_nullspace(Q);
    k += G.find_nullspace(Q, 4, 1e-8, 1e-10, 30, 500, true, false, 7u, true, resid, info);
    const hifamd::HIF<V> &C = G;
    Q = C.nsp_basis();
    Q = C.nsp_basis(true);
    return (int)k;
  }
  return 0;
}
int main() { return run<double>() + run<std::complex<double>>(); }
''')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])
    csrc = tmp_path / "nsp_find_c.c"
    csrc.write_text('#include "hifir_amd.h"\nint f(HifAmdHdl h, double *v, int64_t *k, int *info) { return (int)hifamd_nsp_find(h, '
                    'HIFAMD_SH, 4, 1e-7, 1e-10, 30, 500, 0, v, 16, 0, 1, k, v, 4, v, info) + (int)hifamd_nsp_get_basis(h, HIFAMD_S, v, 4); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(csrc)])


def _probe_numpy(n, seed, cplx):
    """The generator as include/hifir_amd.h states it."""
    def f(c):
        with np.errstate(over="ignore"):
            z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * c.astype(np.uint64)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
        u = (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        return 2.0 * u - 1.0
    i, j = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(16, dtype=np.uint64), indexing="ij")
    re = f(np.uint64(16) * i + j + np.uint64(1))
    if not cplx:
        return re
    return re + 1j * f(np.uint64(16) * (np.uint64(n) + i) + j + np.uint64(1))


def test_host_steps_under_sanitizers_and_probe_generator(tmp_path):
    """import.hpp nsp_find_rotation / nsp_chol_inverse under ASan + UBSan (graded spectrum, rank-deficient, zero, NaN,
    Inf, a negative pivot; real and complex), and nsp_probe_fill against the numpy restatement of the header's formula:
    bit-equal for four seeds, every row (first and last included), real and complex."""
    exe = str(tmp_path / "nsp_find_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "hifir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "nsp_find_test.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    out = str(tmp_path / "probes.bin")
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "nsp_find_test -> ok" in r.stderr
    raw = open(out, "rb").read()
    off = 0
    for seed in (0, 1, 0x123456789ABCDEF, 0xFFFFFFFFFFFFFFFF):
        n = int(np.frombuffer(raw, dtype=np.int64, count=1, offset=off)[0])
        off += 8
        assert n == 1000
        R = np.frombuffer(raw, dtype=np.float64, count=n * 16, offset=off).reshape(n, 16)
        off += n * 16 * 8
        Z = np.frombuffer(raw, dtype=np.complex128, count=n * 16, offset=off).reshape(n, 16)
        off += n * 16 * 16
        Rn, Zn = _probe_numpy(n, seed, False), _probe_numpy(n, seed, True)
        assert np.array_equal(R[0], Rn[0]) and np.array_equal(R[-1], Rn[-1]), seed
        assert np.array_equal(R, Rn) and np.array_equal(Z, Zn), seed
        assert np.array_equal(Z.real, R), seed  # (the real parts share the counters of the real block)
        assert R.min() >= -1.0 and R.max() < 1.0 and abs(R.mean()) < 0.02
    assert off == len(raw)
