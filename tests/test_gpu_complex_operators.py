"""GPU (-m gpu): the opt-in explicit operators of complex handles (HIF(..., complex_operators=ZOP_TAIL | ZOP_TOP)): the
tail of the hierarchy and the closed top of every triangle pair as dense products on the f64 matrix cores (kernels
k_top_gemm_z / k_top_reduce_z), against the oracle and against the handle without them.

The bar is the project's (test_gpu_variants.py): every column within 1e-12 of the oracle in relative max norm, forwards and
conjugate-transposed; a column's bits do not depend on the batch width (complex column tiles end at multiples of 8: the
widths step over every one of those edges up to 48); an all-NaN batch between two applies leaves no trace; the launch
census shows that the product kernels ran (a planner threshold or a guard that kept them away FAILS the test).

Every test here fails without the feature: the constructor argument does not exist."""
import contextlib
import os

import numpy as np
import pytest

from complex_operators_util import ZOP_TAIL, ZOP_TOP, blocks_levels, edge_levels
from util import load_hier, rand_rhs

pytestmark = pytest.mark.gpu

TOL = 1e-12
WIDTHS = (1, 7, 8, 9, 16, 17, 24, 25, 32, 33, 48, 49)
BASE = {"HIFIR_AMD_DENSE_BLOCK": "2048", "HIFIR_AMD_MIN_LOGR": "6"}  # (BASE of test_gpu_variants.py: the defaults, stated)
EDGE_TAILS = (15, 16, 17, 33, 63, 64, 65, 130, 513)  # strip, chunk, 64-row tile and K split edges (513: nine tiles, five splits)


def _synthz():
    import test_gpu_variants

    return test_gpu_variants._synth(np.complex128)


HIERS = {
    "blocksz": blocks_levels,  # tops of 164 and 210 rows, tail of 2,600 (test_complex_operators_host.py prints them)
    "crown17": lambda: blocks_levels(crowns=(17, 17), seed=34),  # tops of 17 and 62 rows
    "crown65": lambda: blocks_levels(crowns=(65, 65), seed=35),  # tops of 65 and 65 rows
    "synthz": _synthz,  # tail of 1,500 rows; no crown: the planner closes no top on it, with the flag or without
    "kkt_26": lambda: load_hier("kkt_26")[0],
    "young1c": lambda: load_hier("young1c")[0],
    "herm_24_symm": lambda: load_hier("herm_24_symm")[0],
}
for _n in EDGE_TAILS:
    HIERS[f"edge{_n}"] = lambda _n=_n: edge_levels(_n)
HIERS["edge130-m20"] = lambda: edge_levels(130, m0=20)  # the tail's right-hand side starts 20 rows into the arena
CROWNED = ("blocksz", "crown17", "crown65")

_cache = {}


def _hier(name, width=100):
    """levels, a batch and the oracle's two answers: once per hierarchy, never written to."""
    if name not in _cache:
        from oracle import orc

        levels = HIERS[name]()
        n = int(levels[0]["n"])
        B = rand_rhs(np.random.default_rng(41), (n, width), np.complex128)
        O = orc.Oracle(levels, dtype=np.complex128)
        h = dict(name=name, levels=levels, B=B, Xo=O.solve_batch(B, threads=4), XoT=O.solve_batch(B, threads=4, trans=True))
        for a in (h["B"], h["Xo"], h["XoT"]):
            a.setflags(write=False)
        _cache[name] = h
    return _cache[name]


@contextlib.contextmanager
def _env(extra=None):
    """The environment a handle is created under, restored before anything is solved."""
    kw = dict(BASE, **(extra or {}))
    names = set(kw) | {"HIFIR_AMD_TAIL_GROWTH", "HIFIR_AMD_TAIL_PROBE_TOL", "HIFIR_AMD_TAIL_ROWS", "HIFIR_AMD_TOP_ROWS"}
    keep = {k: os.environ.get(k) for k in names}
    for k in names:
        os.environ.pop(k, None)
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _handle(h, flags, extra=None):
    import hifir_amd

    with _env(extra):
        return hifir_amd.HIF.from_levels(h["levels"], max_nrhs=64, dtype=np.complex128, complex_operators=flags)


def _colerr(X, Xo):
    return float(max(np.abs(X[:, c] - Xo[:, c]).max() / max(np.abs(Xo[:, c]).max(), 1e-300) for c in range(X.shape[1])))


def _numerics(M, h, widths=WIDTHS, slice_4048=True):
    """Oracle error over the whole batch, width bits and replay, both directions (asserted); the censuses by width."""
    B = h["B"]
    w = min(64, B.shape[1])
    B64 = np.ascontiguousarray(B[:, :w])
    out = {}
    for tr in (False, True):
        e = _colerr(M.solve_mrhs(B, trans=tr), h["XoT" if tr else "Xo"])
        print(f"  {h['name']} trans={tr}: relerr {e:.2e} over {B.shape[1]} columns")
        assert e <= TOL, (tr, e)
        X = M.solve_mrhs(B64, trans=tr)
        out[("X", tr)] = X
        out[("census", w, tr)] = M.kernel_census()
        out[("lower", w, tr)] = M.kernel_census(lower=True)
        for k in widths:
            Xk = M.solve_mrhs(np.ascontiguousarray(B[:, :k]), trans=tr)
            out[("census", k, tr)] = M.kernel_census()
            assert np.array_equal(Xk, X[:, :k]), (tr, k, _colerr(Xk, X[:, :k]))
        if slice_4048:
            Xs = M.solve_mrhs(np.ascontiguousarray(B[:, 40:48]), trans=tr)
            assert np.array_equal(Xs, X[:, 40:48]), (tr, "40:48", _colerr(Xs, X[:, 40:48]))
        M.solve_mrhs(np.full_like(B64, np.nan), trans=tr)
        X3 = M.solve_mrhs(B64, trans=tr)
        assert np.array_equal(X3, X), (tr, int(np.isnan(X3).sum()), _colerr(np.nan_to_num(X3), X))
    return out


def _fmt(c):
    return " ".join(f"{k}={n}" for k, n in c.items() if n)


# ---- 1. every flag on the hierarchies with crowns and on synthz ----------------------------------------------------------
@pytest.mark.parametrize("hier", CROWNED + ("synthz",))
@pytest.mark.parametrize("flags", [ZOP_TAIL, ZOP_TOP, ZOP_TAIL | ZOP_TOP])
def test_operators(flags, hier):
    h = _hier(hier)
    M = _handle(h, flags)
    se = M.stats_ext()
    tops = [int(M.level_stats(l)["top_rows"]) for l in range(len(h["levels"]))]
    print(f"{hier} flags {flags}: tail rows {se['tail_rows']:.0f} (level {se['tail_level']:.0f}, probe {se['tail_probe_relerr']:.2e}, "
          f"max |G| {se['tail_max_abs']:.2e}, rejected {se['tail_rejected']:.0f}), top rows {tops}, top bytes {se['bytes_top']:.0f}")
    assert M.complex_operators() == flags
    # synthz has no crown: the planner (host.hpp choose_top) closes no top on it whatever the flag says, so ZOP_TOP alone
    # leaves it without an operator -- the one case of this table that must NOT launch the product.  That case (synthz,
    # flags 2) therefore checks only the numerics and that k_top_gemm_z is absent; the product itself is not exercised by it
    has_op = not (hier == "synthz" and flags == ZOP_TOP)
    if flags & ZOP_TAIL:
        assert se["tail_rows"] > 0 and se["tail_rejected"] == 0 and se["bytes_tail"] > 0, se
    else:
        assert se["tail_rows"] == 0 and se["bytes_tail"] == 0, se
    if flags & ZOP_TOP and hier in CROWNED:
        assert tops[0] > 0 and tops[1] > 0 and se["bytes_top"] > 0, (tops, se)
    else:
        assert se["bytes_top"] == 0 and not any(tops), (tops, se)
    r = _numerics(M, h)
    for tr in (False, True):
        for k in (64, 16, 1):
            c = r[("census", k, tr)]
            print(f"  census width {k} trans={tr}: {_fmt(c)}")
            assert (c["top_gemm_z"] > 0) == has_op, (k, tr, c["top_gemm_z"])
            assert c["top_gemm"] == 0 and c["top_reduce"] == 0  # (the real product kernels never see complex data)
        if flags & ZOP_TOP and hier in CROWNED:
            assert r[("lower", 64, tr)]["top_gemm_z"] > 0, "never launched on a level >= 1"
        if flags == ZOP_TAIL:
            assert r[("census", 64, tr)]["dense_gemm"] == 0  # (the dense block lives inside the tail)
    M.close()


# ---- 2. the complex goldens: numerics only (a guard may refuse the tail there) ----------------------------------------------
@pytest.mark.parametrize("hier", ["kkt_26", "young1c", "herm_24_symm"])
def test_goldens(hier):
    h = _hier(hier)
    M = _handle(h, ZOP_TAIL | ZOP_TOP)
    se = M.stats_ext()
    print(f"{hier}: tail rows {se['tail_rows']:.0f} tail_rejected {se['tail_rejected']:.0f} probe {se['tail_probe_relerr']:.3e} "
          f"max |G| {se['tail_max_abs']:.3e} top bytes {se['bytes_top']:.0f}")
    r = _numerics(M, h)
    print(f"  census width 64: {_fmt(r[('census', 64, False)])}")
    M.close()


# ---- 3. flags 0: nothing of it --------------------------------------------------------------------------------------------
def _flags0(hier, rank=0):
    """Bits of the handle without the operators, both directions: once per (hierarchy, rank)."""
    key = ("flags0", hier, rank)
    if key not in _cache:
        h = _hier(hier)
        M = _handle(h, 0)
        B64 = np.ascontiguousarray(h["B"][:, :64])
        X = M.solve_mrhs(B64, rank=rank)
        c = M.kernel_census()
        XT = M.solve_mrhs(B64, rank=rank, trans=True)
        _cache[key] = dict(X=X, XT=XT, census=c, censusT=M.kernel_census(), se=M.stats_ext(), flags=M.complex_operators())
        M.close()
    return _cache[key]


def test_flags_0_is_the_default_handle():
    import hifir_amd

    h = _hier("blocksz")
    r = _flags0("blocksz")
    for c in (r["census"], r["censusT"]):
        assert c["top_gemm_z"] == 0 and c["top_reduce_z"] == 0 and c["zcombine"] > 0 and c["band_cd_z"] > 0, _fmt(c)
    se = r["se"]
    assert se["tail_rows"] == 0 and se["bytes_top"] == 0 and se["bytes_tail"] == 0, se
    assert r["flags"] == 0  # (slot 29 of the finalized handle that was created with complex_operators=0)
    with _env():
        M = hifir_amd.HIF.from_levels(h["levels"], max_nrhs=64, dtype=np.complex128)  # as every caller creates one today
    assert M.complex_operators() == 0  # (slot 29 of the finalized default handle)
    se = M.stats_ext()
    assert se["tail_rows"] == 0 and se["bytes_top"] == 0 and se["bytes_tail"] == 0, se
    B64 = np.ascontiguousarray(h["B"][:, :64])
    assert np.array_equal(M.solve_mrhs(B64), r["X"]) and np.array_equal(M.solve_mrhs(B64, trans=True), r["XT"])
    M.close()


# ---- 4. the edges of the product --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hier", [f"edge{n}" for n in EDGE_TAILS] + ["edge130-m20"])
def test_tail_edges(hier):
    h = _hier(hier, width=64)
    M = _handle(h, ZOP_TAIL)
    se = M.stats_ext()
    print(f"{hier}: tail rows {se['tail_rows']:.0f} probe {se['tail_probe_relerr']:.3e} max |G| {se['tail_max_abs']:.3e} "
          f"rejected {se['tail_rejected']:.0f}")
    assert se["tail_rejected"] == 0 and se["tail_rows"] == int(h["levels"][1]["n"]), se  # (a rejection here is a finding)
    r = _numerics(M, h, widths=(1, 8, 9), slice_4048=False)
    for tr in (False, True):
        c = r[("census", 64, tr)]
        print(f"  census width 64 trans={tr}: {_fmt(c)}")
        assert c["top_gemm_z"] > 0 and c["dense_gemm"] == 0
        if hier == "edge513":  # 544 operand columns in five K splits
            assert c["top_reduce_z"] > 0
    M.close()


# ---- 5. guards and rank -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch,code", [("HIFIR_AMD_TAIL_GROWTH", ("1e-30", 2)), ("HIFIR_AMD_TAIL_PROBE_TOL", ("1e-300", 3))])
def test_guards_keep_the_recursion(switch, code):
    h = _hier("blocksz")
    M = _handle(h, ZOP_TAIL, {switch: code[0]})
    assert switch not in os.environ
    se = M.stats_ext()
    print(f"{switch}={code[0]}: rejected {se['tail_rejected']:.0f} probe {se['tail_probe_relerr']:.3e} max |G| {se['tail_max_abs']:.3e}")
    assert se["tail_rejected"] == code[1] and se["tail_rows"] == 0 and se["bytes_tail"] == 0, se
    ref = _flags0("blocksz")
    B64 = np.ascontiguousarray(h["B"][:, :64])
    for tr in (False, True):
        X = M.solve_mrhs(B64, trans=tr)
        assert M.kernel_census()["top_gemm_z"] == 0
        assert np.array_equal(X, ref["XT" if tr else "X"])
    M.close()


def test_other_rank_runs_the_recursion():
    h = _hier("blocksz")
    rank = int(h["levels"][-1]["dense_n"]) - 1
    M = _handle(h, ZOP_TAIL)
    assert M.stats_ext()["tail_rows"] > 0
    ref = _flags0("blocksz", rank=rank)
    B64 = np.ascontiguousarray(h["B"][:, :64])
    for tr in (False, True):
        X = M.solve_mrhs(B64, rank=rank, trans=tr)
        assert M.kernel_census()["top_gemm_z"] == 0
        assert np.array_equal(X, ref["XT" if tr else "X"])
        M.solve_mrhs(B64, trans=tr)
        assert M.kernel_census()["top_gemm_z"] > 0  # (the numerical rank goes through the operator again)
    M.close()


# ---- 6. save / load -------------------------------------------------------------------------------------------------------------
def test_load_with_flags_has_the_bits_of_from_levels(tmp_path):
    import hifir_amd

    h = _hier("blocksz")
    flags = ZOP_TAIL | ZOP_TOP
    M = _handle(h, flags)
    p = str(tmp_path / "blocksz.hif")
    M.save(p)
    with _env():
        M2 = hifir_amd.HIF.load(p, max_nrhs=64, complex_operators=flags)
    assert M2.complex_operators() == flags and M2.stats_ext()["tail_rows"] == M.stats_ext()["tail_rows"] > 0
    B64 = np.ascontiguousarray(h["B"][:, :64])
    for tr in (False, True):
        assert np.array_equal(M2.solve_mrhs(B64, trans=tr), M.solve_mrhs(B64, trans=tr))
        assert M2.kernel_census()["top_gemm_z"] > 0
    M.close()
    M2.close()
