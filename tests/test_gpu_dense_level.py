"""GPU (-m gpu): the dense last level (Engine::launch_dense / launch_dense_mul / zgemm: products of k_dense_gemm_d<4> with
tri = 0, 1, 2, the jpvt row map, k_row_gather on the adjoint engine, two real planes + k_zcombine for complex handles) at its
tile, K-split and rank edges.

A case is (kind, dtype, nd, m): a one-level hierarchy from dense_level_util.dense_level whose dense block -- QRCP, SYEIG with
spd = 0 / 1, or LUP -- is the last level at level 0, behind an empty front level (m = 0) or a 37-row sparse one (m = 37: the
block starts at row 37 of the work arrays).  Sizes: du.LADDER (complex handles leave out 127 and 300); m = 37 at 17, 65, 129.
Ranks: du.rank_arguments -- QRCP every step rank below nd, nd - 1, nd and the arguments 0, -1, nd + 5; SYEIG the (at most 7)
ranks its spectrum has gaps for; LUP ignores the rank (0 and 7 must give identical bits).

Per case, for M^-1, M^-H, M and M^H:
 1. width 70 (two lanes: 64 + 6 columns), every rank: every column against the reference -- the numpy restatement
    (du.BlockRef + du.level_apply; pinned to the oracle in test_dense_level_host.py) for m = 0, Oracle(levels) for m = 37 --
    at the project's own bars, TOL = 1e-12 of test_gpu_parity.py for the solves and PROD_TOL = 1e-11 of test_gpu_product.py
    for the products.  Rank arguments that mean the same rank give the same bits.
 2. the census after a width-64 call at the truncated rank: exactly the dense_gemm / row_gather / zcombine launches that
    launch_dense / launch_dense_mul / zgemm give for the kind, engine and dtype (du.expected_census), no top_gemm, strip_gemm
    or strip_gemm4 -- a case whose kernel does not run fails.
 3. widths 1, 17, 33, 49 and columns 40:48 alone have the bits of the 64-column call (at the truncated and the full rank).
 4. at the truncated rank (nd - 1, the second largest tested): apply, apply an all-NaN batch, apply again -- the bits of the
    first (the scratch rows >= rk hold 0 * NaN in between); a batch whose column 3 is inf leaves every other column's bits.
test_narrow_arenas: HIFIR_AMD_MIN_LOGR=0, widths 1, 2, 3, 5, 9, 17, 33 (arenas of 1 ... 64 columns, partial 16-column tiles)
against the reference at the same bars; bit equality across those widths is printed, not asserted (the project does not
claim it outside the default arena).

Right-hand sides: du.level_rhs, one batch per operator -- uniform random columns plus a component in the direction every
truncation keeps, so that no column is nearly orthogonal to the kept subspace (du.block_rhs says why).

Measured on an MI355X, 148 cases in 13 s (largest column error over all sizes, ranks and m; DESIGN 5.3 has the table by
dtype): qrcp 3.8e-15, lup 3.5e-15, symm0 4.4e-14 (solves) / 1.6e-14 (products), symm1 4.8e-14 (solves) / 1.2e-13 (products).
"""
import os

import numpy as np
import pytest

import dense_level_util as du
import hifir_amd
from dense_level_util import KINDS, OPS, colerr, engine_apply
from oracle import orc
from test_gpu_parity import TOL
from test_gpu_product import PROD_TOL, _differs

REAL, CPLX = np.float64, np.complex128
DTYPES = {"d": REAL, "z": CPLX}
WIDTHS = (1, 17, 33, 49)
NARROW_WIDTHS = (1, 2, 3, 5, 9, 17, 33)
NEVER = ("top_gemm", "strip_gemm", "strip_gemm4")

CASES = [pytest.param(kind, dt, nd, m, id=f"{kind}-{k}-{nd}-m{m}") for kind in KINDS for k, dt in DTYPES.items()
         for nd, m in [(nd, 0) for nd in (du.LADDER if dt is REAL else du.LADDER_Z)] + [(nd, du.FRONT_ROWS) for nd in du.FRONT_SIZES]]
NARROW = [pytest.param(kind, dt, nd, id=f"{kind}-{k}-{nd}") for kind in ("qrcp", "symm0") for k, dt in DTYPES.items()
          for nd in du.FRONT_SIZES]

_MAX = {}  # (kind, dtype, operator) -> largest column error so far in this process (printed with every case)


def _bar(op):
    return TOL if op in ("S", "SH") else PROD_TOL


def _reference(levels, kind, dtype, m):
    """-> (the block's numpy restatement, (op, X, rank) -> the reference result: numpy for m = 0, the oracle for m = 37)"""
    ref = du.BlockRef(du.block_of(levels), kind)
    if m == 0:
        return ref, lambda op, X, rank: du.level_apply(levels[0], ref, op, X, rank)
    O = orc.Oracle(levels, dtype=dtype)
    assert O.dense_rank == int(levels[-1]["dense_n"])
    return ref, lambda op, X, rank: du.oracle_apply(O, op, X, rank)


def _note(kind, dtype, op, e):
    key = (kind, np.dtype(dtype).name, op)
    _MAX[key] = max(_MAX.get(key, 0.0), e)
    return _MAX[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,dtype,nd,m", CASES)
def test_dense_level(kind, dtype, nd, m):
    levels = du.dense_level(nd, kind, dtype, m)
    n, cplx = m + nd, dtype is CPLX
    ref, reference = _reference(levels, kind, dtype, m)
    rng = np.random.default_rng(7000 + nd + m)
    Bs = {op: du.level_rhs(levels, ref, op, 70, rng, dtype) for op in OPS}  # (du.block_rhs: why not plain random columns)
    assert all(b.shape == (n, 70) for b in Bs.values())
    M = hifir_amd.HIF.from_levels(levels, max_nrhs=64, dtype=dtype)
    assert M.schur_size() == nd and M.schur_rank() == nd and M.stats_ext()["tail_rows"] == 0
    tag = f"DENSE-GPU {kind} {np.dtype(dtype).name} nd={nd} m={m}"

    # 1. every rank, width 70, every column against the reference
    worst, bad, by_rank = {op: (0.0, None) for op in OPS}, [], {}
    for rank in du.rank_arguments(kind, nd):
        for op in OPS:
            X = engine_apply(M, op, Bs[op], rank)
            e = colerr(X, reference(op, Bs[op], rank))
            if not e <= worst[op][0]:
                worst[op] = (e, rank)
            if not e <= _bar(op):
                bad.append((op, rank, e))
            eff = 0 if kind == "lup" else du.eff_rank(rank, nd, nd)
            d = _differs(X, by_rank.setdefault((op, eff), X))
            if d:
                bad.append((op, rank, "bits differ from the same rank under another argument", d))
    print(tag + ": " + "  ".join(f"{op} {worst[op][0]:.2e} (rank {worst[op][1]}; so far {_note(kind, dtype, op, worst[op][0]):.2e})"
                                for op in OPS))
    assert not bad, bad

    # 2. census of a 64-column call at the truncated rank
    X64 = {op: np.ascontiguousarray(Bs[op][:, :64]) for op in OPS}
    rt = du.truncated_rank(kind, nd)
    Y64 = {}
    for op in OPS:
        Y64[op] = engine_apply(M, op, X64[op], rt)
        c, exp = M.kernel_census(), du.expected_census(kind, cplx, op)
        print(f"  census {op}: " + " ".join(f"{k}={v}" for k, v in c.items() if v))
        assert c["dense_gemm"] == exp["dense_gemm"] > 0, (op, c["dense_gemm"], exp)
        assert c["row_gather"] == exp["row_gather"], (op, c["row_gather"], exp)
        # (m = 37: the sparse level's block inverses of a complex handle run through k_zcombine as well)
        assert c["zcombine"] == exp["zcombine"] if m == 0 else c["zcombine"] >= exp["zcombine"], (op, c["zcombine"], exp)
        assert bool(c["zcombine"]) == cplx
        for f in NEVER:
            assert c[f] == 0, (op, f, c[f])

    # 3. a column's bits do not depend on the batch width
    width_bits = []
    for rank in sorted({rt, 0 if kind == "lup" else nd}):
        for op in OPS:
            Y = Y64[op] if rank == rt else engine_apply(M, op, X64[op], rank)
            for k in WIDTHS:
                d = _differs(engine_apply(M, op, np.ascontiguousarray(Bs[op][:, :k]), rank), Y[:, :k])
                if d:
                    width_bits.append((rank, op, k) + d)
            d = _differs(engine_apply(M, op, np.ascontiguousarray(Bs[op][:, 40:48]), rank), Y[:, 40:48])
            if d:
                width_bits.append((rank, op, "40:48") + d)
    assert not width_bits, width_bits

    # 4. replay behind an all-NaN batch; one inf column
    nan = np.full_like(X64["S"], np.nan)
    others = [c for c in range(64) if c != 3]
    stale = []
    for op in OPS:
        Xinf = X64[op].copy()
        Xinf[:, 3] = np.inf
        engine_apply(M, op, nan, rt)
        d = _differs(engine_apply(M, op, X64[op], rt), Y64[op])
        if d:
            stale.append((op, "after NaN") + d)
        d = _differs(engine_apply(M, op, Xinf, rt)[:, others], Y64[op][:, others])
        if d:
            stale.append((op, "inf in column 3") + d)
    assert not stale, stale
    M.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,dtype,nd", NARROW)
def test_narrow_arenas(kind, dtype, nd):
    levels = du.dense_level(nd, kind, dtype, 0)
    ref, reference = _reference(levels, kind, dtype, 0)
    rng = np.random.default_rng(9000 + nd)
    Bs = {op: du.level_rhs(levels, ref, op, max(NARROW_WIDTHS), rng, dtype) for op in OPS}
    keep = os.environ.get("HIFIR_AMD_MIN_LOGR")
    try:
        os.environ["HIFIR_AMD_MIN_LOGR"] = "0"
        M = hifir_amd.HIF.from_levels(levels, max_nrhs=64, dtype=dtype)
    finally:
        if keep is None:
            os.environ.pop("HIFIR_AMD_MIN_LOGR", None)
        else:
            os.environ["HIFIR_AMD_MIN_LOGR"] = keep
    bad, same_bits, worst = [], True, {op: 0.0 for op in OPS}
    for rank in (du.truncated_rank(kind, nd), nd):
        for op in OPS:
            B, Yo = Bs[op], reference(op, Bs[op], rank)
            first = None
            for k in NARROW_WIDTHS:
                Y = engine_apply(M, op, np.ascontiguousarray(B[:, :k]), rank)
                c = M.kernel_census()
                assert c["dense_gemm"] > 0 and all(c[f] == 0 for f in NEVER), (op, k, c)
                e = colerr(Y, Yo[:, :k])
                worst[op] = max(worst[op], e) if e == e else e
                if not e <= _bar(op):
                    bad.append((rank, op, k, e))
                first = Y if first is None else first
                same_bits = same_bits and np.array_equal(Y[:, :1], first[:, :1])
    print(f"DENSE-GPU-NARROW {kind} {np.dtype(dtype).name} nd={nd}: " + "  ".join(f"{op} {worst[op]:.2e}" for op in OPS) +
          f"  column 0 has the same bits at every width: {same_bits}")
    assert not bad, bad
    M.close()
