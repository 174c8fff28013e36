"""CPU: the references test_gpu_dense_level.py leans on, pinned to each other (dense_level_util.py).

For every block kind (QRCP, SYEIG with spd = 0 and 1, LUP), float64 and complex128, the four operators (M^-1, M^-H, M, M^H),
every size nd <= 161 of the ladder and every tested rank argument:

 - the numpy / scipy restatement of the block operator (BlockRef: LAPACK geqp3 / eigh / gesv) against the oracle's own block
   entry points orc.qrcp / orc.syeig / orc.lup (restatements of the reference's QRCP.hpp / SYEIG.hpp / LUP.hpp);
 - the numpy restatement of the m = 0 level around the block (level_apply) against Oracle(levels).solve / .mmultiply.

Bounds, on the references themselves (relative, infinity norm, per column; blocks of condition number <= 100 / 64):
   QRCP_LUP_TOL = 1e-13   largest seen 4.4e-15 (qrcp, complex128, nd = 161, rank argument 166, M^-1 through the level);
                          block alone 2.6e-15, lup 2.0e-15
   SYEIG_TOL    = 1e-12   largest seen 1.45e-13 (symm1, complex128, nd = 161, rank 33, M through the level; symm0 7.1e-14):
                          the oracle's cyclic Jacobi, whose eigenvalues are off by about nd * 2e-16 relative to the largest
Above 161 the oracle's SYEIG is neither quick (one factorization at 417: 6 s real; at 257 complex: 4.4 s) nor tight (against
eigh: 2.7e-13 at 257, 3.9e-13 at 417), which is why the GPU test measures the symmetric kinds against eigh.
The right-hand sides are du.block_rhs / du.level_rhs, like the GPU test's (why: block_rhs).

The generators' promises are asserted on the whole ladder: condition numbers, the factor-2 gap at every tested SYEIG rank, the
signs, exact symmetry; and, with the oracle (nd <= 161), numerical rank = nd."""
import numpy as np
import pytest

import dense_level_util as du
from dense_level_util import KINDS, LADDER, LADDER_Z, OPS, BlockRef, block_of, colerr, dense_level, level_apply, rank_arguments
from oracle import orc

QRCP_LUP_TOL = 1e-13
SYEIG_TOL = 1e-12
HOST_MAX = 161
REAL, CPLX = np.float64, np.complex128
DTYPES = {"d": REAL, "z": CPLX}

CASES = [pytest.param(kind, dt, nd, id=f"{kind}-{k}-{nd}") for kind in KINDS for k, dt in DTYPES.items()
         for nd in (LADDER if dt is REAL else LADDER_Z)]
HOST_CASES = [c for c in CASES if c.values[2] <= HOST_MAX]


def _tol(kind):
    return SYEIG_TOL if kind.startswith("symm") else QRCP_LUP_TOL


def _oracle_block(kind, D, op, c, rank):
    """One column through the oracle's block entry point -> (result, numerical rank)"""
    mat = D.ravel(order="F")
    if kind == "qrcp":
        return orc.qrcp(mat, c, op={"S": 0, "M": 1, "SH": 2, "MH": 3}[op], rank=rank)
    if kind == "lup":
        x, info = orc.lup(mat, c, op={"S": 0, "M": 1, "SH": 2, "MH": 3}[op])
        assert info == 0
        return x, D.shape[0]
    x, rk, _ = orc.syeig(mat, c, op=0 if op in ("S", "SH") else 1, rank=rank, spd=int(kind[-1]))
    return x, rk


def test_rank_ladders():
    for nd in LADDER:
        q, s = du.qrcp_ranks(nd), du.symm_ranks(nd)
        assert q[-1] == nd and q[0] == 1 and all(1 <= r <= nd for r in q)
        assert set(q) == ({r for r in du.STEP_RANKS if r < nd} | {nd - 1, nd}) - {0}
        assert len(s) <= 7 and set(s) <= set(q) and 1 in s and nd in s
        assert du.truncated_rank("qrcp", nd) == (sorted(q)[-2] if nd > 1 else 1)
        assert du.truncated_rank("symm0", nd) == (sorted(s)[-2] if nd > 1 else 1)
    # the top of the ladder, by k_dense_gemm_d's loop: a wave reloads its first operand set at kb + 256 < kend (from 257 on),
    # and 417 = 3 * 128 + 32 + 1 is the first size at which a second wave loads a fourth set (one column of it) in trip two
    assert min(nd for nd in LADDER if nd > 256) == 257 and 300 in LADDER and min(nd for nd in LADDER if nd > 416) == 417


def test_eff_rank_contract():
    """0 means the numerical rank; < 0 or > nd the dimension; anything else itself -- in the restatement, and in the oracle on
    a block whose numerical rank is below its dimension (three exactly dependent columns)."""
    assert [du.eff_rank(r, 20, 17) for r in (0, -1, -7, 21, 10 ** 6, 20, 1, 17)] == [17, 20, 20, 20, 20, 20, 1, 17]
    rng = np.random.default_rng(3)
    nd = 20
    D = rng.normal(size=(nd, nd)) + 4 * np.eye(nd)
    D[:, nd - 3:] = D[:, :3] @ rng.normal(size=(3, 3))
    c = rng.uniform(-1, 1, nd)
    mat = D.ravel(order="F")
    for op in range(4):
        x0, rk = orc.qrcp(mat, c, op=op, rank=0)
        assert rk == nd - 3
        assert np.array_equal(x0, orc.qrcp(mat, c, op=op, rank=nd - 3)[0])
        full = orc.qrcp(mat, c, op=op, rank=nd)[0]
        assert not np.array_equal(x0, full)
        for r in (-1, -5, nd + 1, nd + 5, 10 ** 6):
            assert np.array_equal(orc.qrcp(mat, c, op=op, rank=r)[0], full), (op, r)


@pytest.mark.parametrize("kind,dtype,nd", CASES)
def test_generator_promises(kind, dtype, nd):
    for m in (0, du.FRONT_ROWS) if nd in du.FRONT_SIZES else (0,):
        levels = dense_level(nd, kind, dtype, m)
        lv, D = levels[0], block_of(levels)
        assert (int(lv["m"]), int(lv["n"]), int(lv["dense_n"])) == (m, m + nd, nd) and D.dtype == dtype
        again = dense_level(nd, kind, dtype, m)[0]
        assert np.array_equal(again["dense"], lv["dense"]) and np.array_equal(again["p"], lv["p"])  # (deterministic)
        cond = np.linalg.cond(D)
        if not kind.startswith("symm"):
            assert cond <= du.COND_GENERAL, cond
            continue
        assert cond <= du.COND_SYMM * (1 + 1e-12), cond
        assert np.array_equal(D, D.conj().T)
        ref = BlockRef(D, kind)
        w = ref.w[ref.to]  # eigh's eigenvalues in truncation order
        mod = np.abs(w)
        assert np.abs(mod - np.abs(du.symm_spectrum(nd, int(kind[-1])))).max() <= 1e-13 * mod.max()
        for r in du.symm_ranks(nd):
            if r < nd:  # a factor-2 gap right behind the last kept eigenvalue
                gap = mod[r - 1] / mod[r] if kind == "symm0" else mod[r] / mod[r - 1]
                assert abs(gap - 2.0) <= 1e-12, (r, gap)
        if kind == "symm0":
            assert np.all(np.diff(mod) <= 1e-13) and int((w < 0).sum()) == len(range(2, nd, 3))
        else:
            assert np.all(w > 0) and np.all(np.diff(w) >= -1e-13)


@pytest.mark.parametrize("kind,dtype,nd", HOST_CASES)
def test_block_reference_against_the_oracle(kind, dtype, nd):
    D = block_of(dense_level(nd, kind, dtype))
    ref = BlockRef(D, kind)
    rng = np.random.default_rng(nd)
    worst = (0.0, None)
    symm = kind.startswith("symm")
    ranks = rank_arguments(kind, nd)
    if symm and nd > 65:  # (0, -1 and nd + 5 repeat rank nd: test_level_wrapper_against_the_oracle tries them on one factorization)
        ranks = du.symm_ranks(nd)
    for i, rank in enumerate(ranks):
        # (the oracle factorizes again for every call and its Jacobi sweeps dominate; SYEIG uses one operator for both
        #  directions: a rank takes one solve and one product, the directions in turn -- above 65 one of the four in turn)
        for op in (OPS if not symm else (OPS[i % 4],) if nd > 65 else (("S", "SH")[i % 2], ("M", "MH")[i % 2])):
            c = du.block_rhs(ref, op, 1, rng, dtype)[:, 0]
            x, rk = _oracle_block(kind, D, op, c, rank)
            assert rk == nd, "the generator's block must have full numerical rank"
            e = colerr(ref.apply(op, c[:, None], rank), x[:, None])
            worst = (e, (rank, op)) if e >= worst[0] else worst
            assert e <= _tol(kind), (rank, op, e)
    print(f"DENSE-HOST block {kind} {np.dtype(dtype).name} nd={nd}: max {worst[0]:.2e} at {worst[1]}")


@pytest.mark.parametrize("kind,dtype,nd", HOST_CASES)
def test_level_wrapper_against_the_oracle(kind, dtype, nd):
    levels = dense_level(nd, kind, dtype)
    ref = BlockRef(block_of(levels), kind)
    O = orc.Oracle(levels, dtype=dtype)
    assert O.dense_rank == nd
    rng = np.random.default_rng(nd + 1)
    Bs = {op: du.level_rhs(levels, ref, op, 2, rng, dtype) for op in OPS}
    worst = (0.0, None)
    for rank in rank_arguments(kind, nd):
        for op in OPS:
            B = Bs[op]
            e = colerr(level_apply(levels[0], ref, op, B, rank), du.oracle_apply(O, op, B, rank))
            worst = (e, (rank, op)) if e >= worst[0] else worst
            assert e <= _tol(kind), (rank, op, e)
    O.close()
    print(f"DENSE-HOST level {kind} {np.dtype(dtype).name} nd={nd}: max {worst[0]:.2e} at {worst[1]}")
