"""CPU: pins the inputs of test_gpu_blockcg.py (blockcg_util) around the oracle's apply -- block CG at block 1 takes PCG's
iterations and at block 64 strictly fewer; on every input the GPU tests use, every stopping decision keeps
lockstep_edges_util.MARGIN, every kept pivot is >= 1e-6 and every dropped one <= 1e-16 (four decades either side of deftol);
the true residual of a converged column is within the GPU tests' bar; and the hand-stated ranks and fates hold."""
import numpy as np
import pytest

import blockcg_util as U
from lockstep_edges_util import MARGIN, pcg_restated


@pytest.fixture(scope="module")
def restated():
    """name -> (inputs, (X, flags, iters, ranks), trace), each input restated once"""
    out = {}
    for name, solve, A, B, block, rtol, maxit in U.gpu_inputs():
        tr = []
        out[name] = ((solve, A, B, block, rtol, maxit), U.bcg_restated(solve, A, B, block, rtol, maxit, trace=tr), tr)
    return out


def test_block_one_is_pcg_and_block_64_needs_fewer_steps(restated):
    P = U.p32()
    (solve, A, B, block, rtol, maxit), (X, fl, it, rk), tr = restated["width1"]
    Xp, fp, ip = pcg_restated(P.apply, P.A, B, rtol, maxit)
    assert fl.tolist() == fp.tolist() == [0] and it.tolist() == ip.tolist() == [15]
    assert np.linalg.norm(X - Xp) <= 1e-9 * np.linalg.norm(Xp)
    B64 = restated["width64"][0][2]
    ip64 = pcg_restated(P.apply, P.A, B64, rtol, maxit)[2]
    it64 = restated["width64"][1][2]
    assert it64.max() < ip64.min(), (it64, ip64)
    # the counts of every width: the gain of the shared space, width by width
    assert [int(restated["width%d" % w][1][2][0]) for w in U.WIDTHS] == [15, 13, 11, 9, 8, 8, 7, 7]


def test_every_decision_keeps_its_margin(restated):
    for name, (inp, out, tr) in restated.items():
        assert U.decisions_ok(tr, MARGIN), name
    # (the trace is not empty where it matters)
    assert len(restated["width64"][2][0]["steps"]) == 7 and restated["rank_loss"][2][0]["steps"][0]["dropped"] != 0.0


def test_true_residuals_of_converged_columns(restated):
    for name, ((solve, A, B, block, rtol, maxit), (X, fl, it, rk), tr) in restated.items():
        for c in range(B.shape[1]):
            if fl[c] == 0 and np.any(B[:, c]):
                assert np.linalg.norm(A @ X[:, c] - B[:, c]) / np.linalg.norm(B[:, c]) <= 10 * rtol, (name, c)


def test_stated_ranks_and_fates(restated):
    def of(name):
        X, fl, it, rk = restated[name][1]
        return fl.tolist(), it.tolist(), rk.tolist()

    assert of("deflation")[0] == [0] * 8 and of("deflation")[2] == [5, 5] and of("deflation")[1][4] == 0
    assert of("rank_loss")[0] == [0] * 5 and of("rank_loss")[2] == [5, 3]
    assert of("tiny")[0] == [0] * 5 and of("tiny")[2] == [3, 3]
    assert of("maxit3")[0] == [2] * 16 and of("maxit3")[1] == [3] * 16
    assert of("excluded")[2] == [1, 1] and of("excluded")[0] == [0] * 5
    assert [i > 0 for i in of("excluded")[1]] == [False, False, True, False, False]
    assert of("cut40_16")[2] == [16, 16, 16, 16, 8, 8] and of("cut129_64")[2] == [64, 64, 64, 64, 1, 1]
    assert of("complex")[2] == [4, 4] and of("complex_similar")[1] == of("width5")[1]
    assert of("projected")[0] == [0] * 33
    # (-A, M): breakdown at the first step
    P = U.p32()
    B = U.columns(P.A.shape[0], 16)[:, :2]
    fl, it = U.bcg_restated(P.apply, -P.A, B, 2, U.RTOL, 50)[1:3]
    assert fl.tolist() == [1, 1] and it.tolist() == [0, 0]


def test_non_finite_columns_are_excluded_in_the_restatement():
    from krylov_edges_util import neighbours_replaced

    P = U.p32()
    B = U.columns(P.A.shape[0], 5)
    ref = U.bcg_restated(P.apply, P.A, neighbours_replaced(B, 2, "zero"), 5, U.RTOL, U.MAXIT)
    for how in ("nan", "inf", "big"):
        X, fl, it, rk = U.bcg_restated(P.apply, P.A, neighbours_replaced(B, 2, how), 5, U.RTOL, U.MAXIT)
        assert np.array_equal(X, ref[0]) and fl.tolist() == [1, 1, 0, 1, 1] and np.array_equal(it, ref[2]) and rk.tolist() == [1, 1]
