"""CPU: the opt-in explicit operators of complex handles (hifamd_set_complex_operators / hifamd_load_ex, HIF(...,
complex_operators=)).  Both entry points are declared, exported and typed; the refusals come in the documented order; the
planner gives a complex handle combined tops exactly when the flag asks for them; a file written by a handle without the
flags loads into the plan of the flags it is loaded with, analysis trailer or not.  Nothing here is finalized: no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import hifir_amd
from hifir_amd import _lib
from hifir_amd._lib import lib
from complex_operators_util import ZOP_TAIL, ZOP_TOP, blocks_levels, import_levels
from util import load_hier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hifamd_set_complex_operators", "hifamd_load_ex")
NULL_OBJ, MISMATCHED_SIZES, BAD_PREC = 1, 2, 3
BASE = {"HIFIR_AMD_DENSE_BLOCK": "2048", "HIFIR_AMD_MIN_LOGR": "6"}  # (BASE of test_gpu_variants.py)


@pytest.fixture(autouse=True)
def _base_env(monkeypatch):
    for k, v in BASE.items():
        monkeypatch.setenv(k, v)
    for k in ("HIFIR_AMD_TOP_ROWS", "HIFIR_AMD_TOP_WGS", "HIFIR_AMD_TAIL_ROWS", "HIFIR_AMD_LOAD_ANALYSIS"):
        monkeypatch.delenv(k, raising=False)


def test_symbols_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "hifir_amd.h")).read()
    declared = set(re.findall(r"\b(hifamd_\w+)\s*\(", hdr))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["hifamd_set_complex_operators"] == (i, [vp, i])
    assert _lib.SIGNATURES["hifamd_load_ex"] == (i, [ctypes.c_char_p, i, i, ctypes.POINTER(vp)])
    assert re.search(r"#define\s+HIFAMD_ZOP_TAIL\s+1\b", hdr) and re.search(r"#define\s+HIFAMD_ZOP_TOP\s+2\b", hdr)
    assert (hifir_amd.hif.ZOP_TAIL, hifir_amd.hif.ZOP_TOP) == (ZOP_TAIL, ZOP_TOP) == (1, 2)
    # the shim's extension header keeps its entry points, the C++ facade has the member
    ext = open(os.path.join(ROOT, "include", "libhifir_amd_ext.h")).read()
    assert "complex_operators" not in ext
    assert "set_complex_operators" in open(os.path.join(ROOT, "include", "hifir_amd.hpp")).read()


def test_refusals_in_order():
    f = lib().hifamd_set_complex_operators
    # NULL handle before everything else
    for flags in (0, 1, -1, 4):
        assert f(None, flags) == NULL_OBJ
    levels, _ = load_hier("p2d_5")
    R = hifir_amd.HIF(np.float64)
    Z = hifir_amd.HIF(np.complex128)
    # flags outside 0 ... 3: before the handle's value type and state are looked at
    for flags in (-1, 4, 7, 1 << 20):
        assert f(R._h, flags) == MISMATCHED_SIZES
        assert f(Z._h, flags) == MISMATCHED_SIZES
    # a real handle has both operators already: the message says so; flags 0 is a no-op there
    for flags in (1, 2, 3):
        assert f(R._h, flags) == BAD_PREC
        assert b"already" in lib().hifamd_last_error()
    assert f(R._h, 0) == 0
    # a fresh complex handle takes every value, any number of times; slot 29 reports the flags in force
    for flags in (0, 1, 2, 3, 0, 3):
        assert f(Z._h, flags) == 0
        assert Z.complex_operators() == flags
    assert R.complex_operators() == 0
    # ... until it has a level: the planner options shaped that level's analysis
    kkt, _ = load_hier("kkt_26")
    Z.add_level(kkt[0])
    for flags in (-1, 4):
        assert f(Z._h, flags) == MISMATCHED_SIZES  # (still the earlier refusal)
    for flags in (0, 1, 2, 3):
        assert f(Z._h, flags) == BAD_PREC
        assert b"before the first" in lib().hifamd_last_error()
    assert Z.complex_operators() == 3
    R.add_level(levels[0])
    assert f(R._h, 2) == BAD_PREC and f(R._h, 0) == 0
    with pytest.raises(hifir_amd.HifAmdError) as e:
        hifir_amd.HIF(np.float64, complex_operators=1)
    assert e.value.code == BAD_PREC
    with pytest.raises(hifir_amd.HifAmdError) as e:
        hifir_amd.HIF(np.complex128, complex_operators=4)
    assert e.value.code == MISMATCHED_SIZES


# `blocksz` of test_gpu_variants.py, and two more of its kind whose crowns have 17 and 65 rows.  What the planner closes
# into a top is the crown plus whatever rows the closure under L and U adds (level 1 of the 17-row crown: 62 rows).
HIERS = {"blocksz": dict(), "crown17": dict(crowns=(17, 17), seed=34), "crown65": dict(crowns=(65, 65), seed=35)}


def _tops(M):
    return [int(M.level_stats(l)["top_rows"]) for l in range(3)]


@pytest.mark.parametrize("name", list(HIERS))
def test_planner_gives_tops_on_request_only(name):
    levels = blocks_levels(**HIERS[name])
    if name == "blocksz":
        import test_gpu_variants

        ref = test_gpu_variants._blocks(np.complex128)
        assert all(np.array_equal(a[k], b[k]) for a, b in zip(levels, ref) for k in b)  # the very same hierarchy
    tops = {}
    for flags in (0, ZOP_TAIL, ZOP_TOP, ZOP_TAIL | ZOP_TOP):
        M = import_levels(levels, complex_operators=flags)
        tops[flags] = _tops(M)
        print(f"{name} flags {flags}: top rows per level {tops[flags]}, bands L/U",
              [(int(M.level_stats(l)["bands_L"]), int(M.level_stats(l)["bands_U"])) for l in range(3)])
        M.close()
    assert tops[0] == [0, 0, 0] and tops[ZOP_TAIL] == [0, 0, 0]
    assert tops[ZOP_TOP][0] > 0 and tops[ZOP_TOP][1] > 0 and tops[3] == tops[ZOP_TOP]
    crown = HIERS[name].get("crowns", (160, 120))
    assert tops[ZOP_TOP][0] >= crown[0] and tops[ZOP_TOP][1] >= crown[1]
    if name != "blocksz":  # sizes that are no multiple of 16 or 64
        assert all(t % 16 for t in tops[ZOP_TOP][:2]), tops


def _level_stats(M):
    return [M.level_stats(l) for l in range(int(M.stats()["sparse_levels"]))]


@pytest.mark.parametrize("analysis", [False, True])
def test_load_ex_plans_with_the_readers_flags(tmp_path, analysis):
    levels = blocks_levels()
    M0 = import_levels(levels, complex_operators=0)
    M2 = import_levels(levels, complex_operators=ZOP_TOP)
    want0, want2 = _level_stats(M0), _level_stats(M2)
    assert want0 != want2
    p = str(tmp_path / "blocksz.hif")
    M0.save(p, analysis=analysis)
    # hifamd_load == hifamd_load_ex(..., 0): the writer's plan (adopted from the trailer where there is one)
    A = hifir_amd.HIF.load(p, max_nrhs=0)
    assert _level_stats(A) == want0 and A.complex_operators() == 0
    assert int(A.stats_ext()["analysis_cached_levels"]) == (3 if analysis else 0)
    h = ctypes.c_void_p()
    assert lib().hifamd_load(p.encode(), -1, ctypes.byref(h)) == 0
    st = np.zeros(32)
    assert lib().hifamd_stats_ext(h, st.ctypes.data_as(ctypes.c_void_p), 32) >= 30 and st[29] == 0
    lib().hifamd_destroy(h)
    # the reader's flags: the plan of a handle imported under them; a trailer written under other options is not adopted
    B = hifir_amd.HIF.load(p, max_nrhs=0, complex_operators=ZOP_TOP)
    assert _level_stats(B) == want2 and B.complex_operators() == ZOP_TOP
    assert int(B.stats_ext()["analysis_cached_levels"]) == 0
    # ... and the other way round
    M2.save(p, analysis=analysis)
    assert _level_stats(hifir_amd.HIF.load(p, max_nrhs=0)) == want0
    C2 = hifir_amd.HIF.load(p, max_nrhs=0, complex_operators=ZOP_TOP)
    assert _level_stats(C2) == want2 and int(C2.stats_ext()["analysis_cached_levels"]) == (3 if analysis else 0)
    # refusals of the flags come back from the load, and no handle with them
    for flags, code in ((4, MISMATCHED_SIZES), (-1, MISMATCHED_SIZES)):
        h = ctypes.c_void_p()
        assert lib().hifamd_load_ex(p.encode(), -1, flags, ctypes.byref(h)) == code and not h.value
    R = import_levels(load_hier("p2d_5")[0], dtype=np.float64)
    pr = str(tmp_path / "real.hif")
    R.save(pr)
    h = ctypes.c_void_p()
    assert lib().hifamd_load_ex(pr.encode(), -1, ZOP_TAIL, ctypes.byref(h)) == BAD_PREC and not h.value
    assert lib().hifamd_load_ex(pr.encode(), -1, 0, ctypes.byref(h)) == 0 and h.value
    lib().hifamd_destroy(h)
