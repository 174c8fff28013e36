"""CPU: pins the inputs and restatements of tests/krylov_edges_util.py, so that test_gpu_krylov_edges.py cannot pass vacuously --
the refinement restatement against the oracle's own hifir, the fates of the mixed batches under the restated GMRES, the margins
of the stagnating and of the bounded-refinement inputs, and the multiple-of-restart case."""
import numpy as np
import pytest

from krylov_edges_util import (IR_FATES, QUIRK, SCALED_COPY_OF, csr_of, finishing_steps, gmres_ratio_history, ir_mixed_batch, ir_restated, mixed_batch,
                               mixed_fates, perturbed, stagnating_case)
from oracle import orc
from util import load_hier, relerr


@pytest.mark.parametrize("name", ["p2d_30", "cd2d_48", "young1c"])
def test_ir_restated_is_the_oracles_hifir(name):
    levels, d = load_hier(name)
    O, A = orc.Oracle(levels), csr_of(d)
    for b in (d["b"], d["B4"][:, 3].copy()):
        for nirs, betas in ((1, None), (4, None), (16, (1e-10, 1e3)), (3, (1e-10, 1e3)), (16, (1e-4, 1e3))):
            x, it, fl = ir_restated(O, A, b, nirs, betas)
            xo, st = O.hifir(A.indptr, A.indices, A.data, b, nirs, betas)
            assert (it, fl) == st, (nirs, betas)
            assert relerr(x, xo) <= 1e-13, (nirs, betas)
    assert ir_restated(O, A, 0 * d["b"], 16, (1e-10, 1e3))[1:] == (0, 0)


@pytest.mark.parametrize("name", ["p2d_30", "cd2d_48", "young1c"])
def test_ir_restated_transposed_reduces_the_true_residual(name):
    # there is no O.hifir for A^H: the true residual of A^H x = b has to fall sweep over sweep
    levels, d = load_hier(name)
    O, A = orc.Oracle(levels), csr_of(d)
    AH = A.conj().T.tocsr()
    b = d["b"]
    res = [np.linalg.norm(AH @ ir_restated(O, A, b, N, trans=True)[0] - b) / np.linalg.norm(b) for N in (1, 2, 3, 4)]
    assert all(res[i + 1] < 0.5 * res[i] for i in range(3)), res
    hist = []
    x, it, fl = ir_restated(O, A, b, 16, (1e-10, 1e3), trans=True, history=hist)
    assert fl == 0 and 2 <= it < 16 and len(hist) == it
    assert np.linalg.norm(AH @ x - b) / np.linalg.norm(b) == pytest.approx(hist[-1], rel=1e-6) and hist[-1] <= 1e-10


@pytest.mark.parametrize("name,real", [("cd2d_48", True), ("young1c", False)])
def test_mixed_batch_fates(name, real):
    levels, d = load_hier(name)
    O, A = orc.Oracle(levels), perturbed(d, 0.05, real=real)
    assert np.iscomplexobj(A.data) != real
    B, fates = mixed_batch(O, d, A, 65, seed=11)
    assert [fates[i] for i in (0, 31, 32, 33, 63, 64)] == ["hard", "easy", "hard", "easy", "easy", "hard"]
    assert {"zero", "tiny", "huge", "b", "ones"} <= set(fates)
    restart, maxit = 12, 300
    res = [orc.gmres(O, A.indptr, A.indices, A.data, B[:, c].copy(), restart=restart, rtol=1e-9, maxit=maxit) for c in range(65)]
    its = np.array([r[2] for r in res])
    z = fates.index("zero")
    assert res[z][1:] == (0, 0) and not res[z][0].any()
    nz = [c for c in range(65) if fates[c] != "zero"]
    assert all(res[c][1] == 0 and 0 < its[c] < maxit - 1 for c in nz), its
    where = [finishing_steps(its[c], restart) for c in nz]
    cycles = sorted({o for o, _ in where})
    assert len(cycles) >= 2, where  # a column is done one outer cycle before another
    assert max(len({j for o, j in where if o == cyc}) for cyc in cycles) >= 3, where  # three finishing steps in one cycle
    assert all(finishing_steps(its[c], restart)[0] == 0 for c in range(65) if fates[c] == "easy"), its
    assert all(finishing_steps(its[c], restart)[0] >= 1 for c in range(65) if fates[c] == "hard"), its
    for f, of in SCALED_COPY_OF.items():
        assert res[fates.index(f)][1:] == res[fates.index(of)][1:]


def test_mixed_fates_at_every_width():
    for w in (1, 3, 5, 33, 48, 63, 64, 65, 70, 129, 130):
        f = mixed_fates(w)
        assert len(f) == w and f[0] == "hard" and f[w - 1] == "hard"
        assert w < 5 or "zero" in f
        assert w < 34 or (f[31], f[32]) == ("easy", "hard")


def test_stagnating_case_margins():
    S = stagnating_case()
    O, A = orc.Oracle(S["levels"]), S["A"]
    n = A.shape[0]
    assert np.array_equal(O.solve_batch(np.eye(n)), np.eye(n))  # M^-1 = I exactly
    C = A.toarray()
    for name, b in S["columns"].items():
        x, fl, it = orc.gmres(O, A.indptr, A.indices, A.data, b, restart=12, rtol=1e-9, maxit=40)
        assert (fl, it) == S["expected"][name], name
        if name == "edge":  # the comparison itself: the ratio IS the bound, and the restatement takes >= as the reference does
            t = 1.0 * (1.0 - 1e-8)
            assert gmres_ratio_history(C, b, 1)[0] == pytest.approx(t, abs=1e-15) and A[97, 96] == t
        elif fl == 1:
            ratios = gmres_ratio_history(C, b, it + 1)
            msg = "%s: ratios before the stop %s, at the stop %.17g" % (name, ratios[:-1], ratios[-1])
            assert ratios[-1] >= 1.0 - 1e-12, msg  # four orders inside the test resid >= resid_prev * (1 - 1e-8)
            assert all(r <= 1.0 - 1e-4 for r in ratios[:-1]), msg
    x, fl, it = orc.gmres(O, A.indptr, A.indices, A.data, S["columns"]["now"], restart=12, rtol=1e-9, maxit=40)
    assert not x.any()
    x, fl, it = orc.gmres(O, A.indptr, A.indices, A.data, S["columns"]["later"], restart=12, rtol=1e-9, maxit=40)
    assert it >= 1 and relerr(x, 0.5 * S["columns"]["later"]) <= 1e-15


def test_multiple_of_restart_quirk():
    # maxit = k * restart without convergence: the driver runs out of outer cycles before the maxit test (gmres.hpp:94) is
    # reached again, and returns flag 0 with iters == maxit and a residual above rtol
    name, restart, maxit, rtol = QUIRK
    levels, d = load_hier(name)
    O, A = orc.Oracle(levels), perturbed(d, 0.05, real=True)
    assert maxit % restart == 0
    x, fl, it = orc.gmres(O, A.indptr, A.indices, A.data, d["b"], restart=restart, rtol=rtol, maxit=maxit)
    assert (fl, it) == (0, maxit)
    assert np.linalg.norm(A @ x - d["b"]) / np.linalg.norm(d["b"]) > 100 * rtol
    x, fl, it = orc.gmres(O, A.indptr, A.indices, A.data, d["b"], restart=restart, rtol=rtol, maxit=maxit + 1)
    assert (fl, it) == (2, maxit + 1)  # one more and the test is reached


def test_ir_mixed_batch_has_all_fates():
    S = ir_mixed_batch(width=70)
    O, A, B = orc.Oracle(S["levels"]), S["A"], S["B"]
    assert set(S["fates"]) == set(IR_FATES)
    lo, hi = S["betas"]
    seen = set()
    for c in range(B.shape[1]):
        hist = []
        x, it, fl = ir_restated(O, A, B[:, c].copy(), S["nirs"], S["betas"], history=hist)
        assert (it, fl) == S["expected"][c], (c, S["fates"][c])
        xo, st = O.hifir(A.indptr, A.indices, A.data, B[:, c].copy(), S["nirs"], S["betas"])
        assert st == (it, fl) and relerr(x, xo) <= 1e-13
        # every ratio that met the betas is a factor 10 away from both
        assert all((r <= lo / 10 or r >= 10 * lo) and (r <= hi / 10 or r >= 10 * hi) for r in hist), (c, hist)
        seen.add((S["fates"][c], fl))
    assert seen == {("zero", 0), ("two", 0), ("later", 0), ("exhaust", -1), ("diverge", 1)}
    assert {S["expected"][c][0] for c in range(70) if S["fates"][c] == "later"} == {3, 4, 5, 6}
