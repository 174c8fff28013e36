"""CPU: the BiCGSTAB entry points (hifamd_bicgstab_batch / _dev, HIF.bicgstab, the C++ facade's bicgstab) are declared,
exported and typed, refuse a NULL handle and an unfinalized hierarchy, and never return a CPU result."""
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
NAMES = ("hifamd_bicgstab_batch", "hifamd_bicgstab_batch_dev")


def test_symbols_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "hifir_amd.h")).read()
    declared = set(re.findall(r"\b(hifamd_\w+)\s*\(", hdr))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
        # the signature of the hifamd_pcg_batch* pair
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("bicgstab", "pcg")], name


def test_null_handle():
    fl = np.zeros(1, dtype=np.int32)
    it = np.zeros(1, dtype=np.int32)
    b = np.ones(4)
    x = np.zeros(4)
    for name in NAMES:
        st = getattr(lib(), name)(None, b.ctypes.data, 1, x.ctypes.data, 1, 1, 1e-6, 10, 0, fl.ctypes.data,
                                  it.ctypes.data)
        assert st == 1, (name, st)  # HIFAMD_NULL_OBJ


def _import(name):
    """add_level / set_dense* as HIF.from_levels does, without finalize (no GPU needed)."""
    levels, d = load_hier(name)
    cplx = any(np.iscomplexobj(lv["L_vals"]) or np.iscomplexobj(lv["d"]) for lv in levels)
    M = hifir_amd.HIF(np.complex128 if cplx else np.float64)
    for lv in levels:
        M.add_level(lv)
    last = levels[-1]
    if int(last.get("dense_n", 0)) > 0:
        if int(last.get("dense_lup", 0)):
            M.set_dense_lup(last["dense"])
        elif int(last.get("dense_symm", 0)):
            M.set_dense_symm(last["dense"], int(last.get("spd", 0)))
        else:
            M.set_dense(last["dense"])
    return M, d


@pytest.mark.parametrize("name", ["cd2d_48", "young1c"])
def test_bicgstab_has_no_cpu_fallback(name):
    M, d = _import(name)
    b = np.asarray(d["b"], dtype=M.dtype)
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.bicgstab(b)  # not finalized: never a CPU result
    assert e.value.code == 3  # HIFAMD_BAD_PREC
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.bicgstab(np.stack([b, b], axis=1), rtol=1e-8, maxit=4)
    assert e.value.code == 3
    if lib().hifamd_device_count() == 0:
        with pytest.raises(hifir_amd.HifAmdError) as e:
            M.finalize(1)
        assert e.value.code == 4 and "no CPU fallback" in e.value.msg
        with pytest.raises(hifir_amd.HifAmdError):
            M.bicgstab(b)


def test_cpp_facade_bicgstab_compiles(tmp_path):
    src = tmp_path / "bicgstab_facade.cpp"
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
    auto out = G.bicgstab(A, b, 1e-6, 100);
    auto out2 = G.bicgstab(A, b, 1e-6, 100, true);
    std::vector<V> x = std::get<0>(out);
    return std::get<1>(out) + std::get<2>(out2) + (int)x.size();
  }
  return 0;
}
int main() { return run<double>() + run<std::complex<double>>(); }
''')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])
