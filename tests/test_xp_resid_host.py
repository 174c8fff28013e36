"""CPU: the inputs and restatements of xp_resid_util.py do what test_gpu_xp_resid.py relies on.  The restated compensated
residual meets the Dot2 bound against the rational residual on every row where the working-precision one misses it; under it
the restated refinement reaches the integer solution to 2 eps where the plain one stays seven digits away; the restated
GMRES-IR certifies 1e-14, and the rational residual confirms the certificate."""
import numpy as np
import pytest

import xp_resid_util as U

CASES = [(w, z) for w in (0, 1) for z in (False, True)]
IDS = ["graded%d-%s" % (U.GRADED[w][0], "z" if z else "d") for w, z in CASES]


def _plain_iterate(C):
    """an iterate near the solution, where b - A x cancels completely: three sweeps of plain refinement"""
    solve = lambda r: np.linalg.solve(C["A"], r)
    rw = lambda b, x: U.resid_working(C["indptr"], C["indices"], C["vals"], b, x)
    return U.refine(solve, rw, C["B"][:, 0], 3)[-1]


def test_condition_numbers_of_the_graded_cases():
    for w, z in CASES:
        k = np.linalg.cond(U.graded_case(w, z)["A"])
        assert 1e9 <= k <= 1e11, (w, z, k)


@pytest.mark.parametrize("cplx", [False, True], ids=["d", "z"])
def test_compensated_residual_meets_dot2_bound_on_random_sparse_rows(cplx):
    import scipy.sparse as sp

    rng = np.random.default_rng(5)
    n = 60
    A = sp.random(n, n, density=0.15, random_state=np.random.RandomState(3), format="csr")
    A.data = rng.normal(size=A.nnz) * 10.0 ** rng.integers(-6, 6, A.nnz)
    if cplx:
        A = A.astype(np.complex128)
        A.data = A.data + 1j * rng.normal(size=A.nnz) * 10.0 ** rng.integers(-6, 6, A.nnz)
    A.sort_indices()
    ip, ix, v = A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data
    x = rng.normal(size=n) + (1j * rng.normal(size=n) if cplx else 0)
    b = A @ x  # (rounded: the residual is all cancellation)
    ex = U.resid_exact(ip, ix, v, b, x)
    err, bound = U.err_vs_exact(U.resid_dd(ip, ix, v, b, x), ex), U.dot2_bound(ip, ix, v, b, x, ex)
    err_wk = U.err_vs_exact(U.resid_working(ip, ix, v, b, x), ex)
    print("compensated: worst err / bound %.3g; working: worst err / bound %.3g" % (np.max(err / bound), np.max(err_wk / bound)))
    assert np.all(err <= bound)
    assert np.max(err) > 0 and np.max(err_wk / bound) > 1  # (the case is not a trivial one)


@pytest.mark.parametrize("which,cplx", CASES, ids=IDS)
def test_dot2_bound_at_an_iterate_of_plain_refinement(which, cplx):
    C = U.graded_case(which, cplx)
    ip, ix, v, b = C["indptr"], C["indices"], C["vals"], C["B"][:, 0]
    x = _plain_iterate(C)
    ex = U.resid_exact(ip, ix, v, b, x)
    bound = U.dot2_bound(ip, ix, v, b, x, ex)
    err_dd = U.err_vs_exact(U.resid_dd(ip, ix, v, b, x), ex)
    err_wk = U.err_vs_exact(U.resid_working(ip, ix, v, b, x), ex)
    print("rows", C["n"], "compensated: worst err / bound %.3g" % np.max(err_dd / bound),
          "working: rows beyond the bound %d" % int(np.sum(err_wk > bound)))
    assert np.all(err_dd <= bound)
    assert np.sum(err_wk > bound) > C["n"] // 2


@pytest.mark.parametrize("which,cplx", CASES, ids=IDS)
def test_refinement_restated_compensated_reaches_xt_plain_does_not(which, cplx):
    C = U.graded_case(which, cplx)
    solve = lambda r: np.linalg.solve(C["A"], r)
    rd = lambda b, x: U.resid_dd(C["indptr"], C["indices"], C["vals"], b, x)
    rw = lambda b, x: U.resid_working(C["indptr"], C["indices"], C["vals"], b, x)
    xs = U.refine(solve, rd, C["B"], 4)
    assert any(U.fwd_ok(x, C["XT"]) for x in xs), [U.fwd_err(x, C["XT"]) for x in xs]
    xs = U.refine(solve, rw, C["B"], 8)
    for k in range(2, 8):  # sweeps 3 to 8: this margin is what the GPU test's "above 1e-10 under mode 0" stands on
        assert min(U.fwd_err(xs[k][:, c], C["XT"][:, c]) for c in range(U.NCOLS)) > 1e-10


def _confirm(ip, ix, v, b, x, relres):
    """the certificate against the rational residual"""
    true = U.exact_norm(U.resid_exact(ip, ix, v, b, x)) / np.linalg.norm(b)
    assert true <= 2e-14, true
    assert abs(true - relres) <= 1e-3 * true + 1e-30, (true, relres)


@pytest.mark.parametrize("which,cplx", CASES, ids=IDS)
def test_gmres_ir_restated_on_the_graded_cases(which, cplx):
    C = U.graded_case(which, cplx)
    ip, ix, v, A = C["indptr"], C["indices"], C["vals"], C["A"]
    b = C["B"][:, 0]
    args = (lambda y: A @ y, lambda r: np.linalg.solve(A, r), lambda bb, xx: U.resid_dd(ip, ix, v, bb, xx), b)
    x, flag, outer, iters, relres = U.gmres_ir(*args)
    assert flag == 0 and outer <= 4 and relres <= 1e-14, (flag, outer, relres)
    _confirm(ip, ix, v, b, x, relres)
    # a residual of 1e-14 bounds the forward error by cond(A) 1e-14 only: the forward bar needs rtol = eps / cond(A), with the
    # condition numbers pinned above RTOL_FWD; b is exact, so the iteration ends on xt itself with the residual 0
    x, flag, outer, iters, relres = U.gmres_ir(*args, rtol=U.RTOL_FWD)
    assert flag == 0 and outer <= 4 and relres <= U.RTOL_FWD, (flag, outer, relres)
    assert U.fwd_ok(x, C["XT"][:, 0])


@pytest.mark.parametrize("name", U.FIXTURES)
def test_gmres_ir_restated_on_the_fixtures(name):
    from oracle import orc

    C = U.fixture_case(name)
    ip, ix, v, A = C["indptr"], C["indices"], C["vals"], C["A"]
    O = orc.Oracle(C["levels"])
    b = C["B"][:, 0]
    x, flag, outer, iters, relres = U.gmres_ir(lambda y: A @ y, O.solve, lambda bb, xx: U.resid_dd(ip, ix, v, bb, xx), b)
    print(name, "flag", flag, "outer", outer, "inner iterations", iters, "relres %.3g" % relres)
    assert flag == 0 and outer <= 4 and relres <= 1e-14, (flag, outer, relres)
    _confirm(ip, ix, v, b, x, relres)
