"""CPU: pins the inputs of test_gpu_lobpcg.py (lobpcg_util) around the oracle's apply -- on every case the restatement reaches
flag 0 on its first nev columns, its eigenvalues agree with numpy.linalg.eigvalsh of the dense matrix to tol ||A||_inf (the
residual bound, safe in clusters), its vectors are orthonormal, its step counts are the pinned ones, the recurrence's residual
stays within DRIFT of the true one, and every decision keeps its margin (no res_j / tol within lockstep_edges_util.MARGIN of
1, no Cholesky pivot within a factor two of deftol) and survives six runs with one rounding of noise per element, so that a
device decision cannot differ from the restated one.  The indefinite pair is pinned to flag 2."""
import numpy as np
import pytest

import lobpcg_util as U
from lockstep_edges_util import MARGIN


@pytest.fixture(scope="module")
def restated():
    return {c[0]: U.reference(c[0]) for c in U.CASES}


def test_flags_counts_and_eigenvalues(restated):
    for name, fixture, k, nev, tol, basis, want, seed in U.CASES:
        (Cs, solve, X0, _, _, _, Q), (lam, X, res, fl, steps, rank), tr = restated[name]
        assert fl[:nev].tolist() == [0] * nev and steps == want and k <= rank <= 3 * k, (name, fl, steps, rank)
        assert (res[:nev] <= tol).all() and len(tr) == steps + 1, name
        eig = Cs.eig
        if basis:  # on the complement of the null space: its eigenvalues 0 (here one) are skipped
            assert abs(eig[0]) <= 1e-12 * Cs.anorm and eig[1] > 1e-6 * Cs.anorm
            eig = eig[Q.shape[1]:]
            assert np.linalg.norm(Q.conj().T @ X) <= 1e-12, name
        assert np.abs(lam[:nev] - eig[:nev]).max() <= tol * Cs.anorm, (name, np.abs(lam[:nev] - eig[:nev]).max() / Cs.anorm)
        assert (np.diff(lam) >= 0).all() and np.linalg.norm(X.conj().T @ X - np.eye(k)) <= 1e-12, name
    # the guard columns did not hold the solve up
    assert restated["herm_k16_nev8"][1][3][8:].any() and restated["p32_k16_nev1"][1][3].tolist() == [0] + [2] * 15
    assert restated["herm_k6"][0][0].cplx and restated["p32z_k5"][0][0].cplx
    # what the basis filter buys on neu2d_32_symm: the smallest nonzero eigenvalue
    Cs = restated["neu_k5_basis"][0][0]
    assert abs(restated["neu_k5_basis"][1][0][0] - 9.6305e-3) <= 5e-8 and abs(restated["neu_k5"][1][0][0]) <= 1e-8 * Cs.anorm
    assert np.abs(restated["twobody_k4"][1][0][:2]).max() <= 1e-8 * restated["twobody_k4"][0][0].anorm  # both null vectors


def test_recurrence_drift(restated):
    worst = 0.0
    for name, ((Cs, *_), (lam, X, res, fl, steps, rank), tr) in restated.items():
        true = np.linalg.norm(Cs.A @ X - X * lam[None, :], axis=0) / Cs.anorm
        worst = max(worst, float(np.abs(true - res).max()))
    print("largest |res_j - true residual|:", worst)
    assert U.DRIFT / 10 <= worst <= U.DRIFT


def test_every_decision_keeps_its_margin(restated):
    for name, (inp, out, tr) in restated.items():
        assert U.decisions_ok(tr, MARGIN), name
    assert any("kept" in st and st["dropped"] != 0.0 for st in restated["p32_k5"][2])  # (the trace is not empty where it matters)


def test_step_counts_do_not_hang_on_a_rounding(restated):
    for name, ((Cs, solve, X0, k, nev, tol, Q), out, tr) in restated.items():
        for sd in U.NOISE_SEEDS:
            t2 = []
            o = U.lobpcg_restated(solve, Cs.A, X0, nev, tol, U.MAXIT, Q=Q, trace=t2, noise=np.random.default_rng(sd))
            assert o[4] == out[4] and o[3].tolist() == out[3].tolist() and U.decisions_ok(t2, MARGIN), (name, sd, o[4], out[4])


def test_full_blocks_have_pinned_counts_and_pass_the_noise_test():
    for fixture, k, tol, seed, want in U.FULL_BLOCKS:
        Cs = U.case(fixture)
        X0 = U.start_block(Cs.n, k, seed=seed)
        tr = []
        lam, X, res, fl, steps, rank = U.lobpcg_restated(Cs.O, Cs.A, X0, k, tol, U.MAXIT, trace=tr)
        assert fl.tolist() == [0] * k and steps == want and U.decisions_ok(tr, MARGIN), (k, steps)
        assert np.abs(lam - Cs.eig[:k]).max() <= tol * Cs.anorm and np.linalg.norm(X.T @ X - np.eye(k)) <= 1e-12
        for sd in U.NOISE_SEEDS:
            t2 = []
            o = U.lobpcg_restated(Cs.O, Cs.A, X0, k, tol, U.MAXIT, trace=t2, noise=np.random.default_rng(sd))
            assert o[4] == want and o[3].tolist() == [0] * k and U.decisions_ok(t2, MARGIN), (k, sd, o[4])


def test_maxit_and_refused_starts(restated):
    (Cs, solve, X0, k, nev, tol, Q), (lam, X, res, fl, steps, rank), tr = restated["p32_k5"]
    short = U.lobpcg_restated(solve, Cs.A, X0, nev, tol, steps - 1)
    assert short[4] == steps - 1 and 2 in short[3].tolist() and set(short[3].tolist()) <= {0, 2}
    at = U.lobpcg_restated(solve, Cs.A, X0, nev, tol, steps)
    assert at[4] == steps and at[3].tolist() == [0] * k and np.array_equal(at[0], lam)
    dup = X0.copy()
    dup[:, 3] = dup[:, 1]
    with pytest.raises(U.StartRefused, match="rank deficient"):
        U.lobpcg_restated(solve, Cs.A, dup, nev, tol, 10)
    bad = X0.copy()
    bad[7, 2] = np.nan
    with pytest.raises(U.StartRefused, match="non-finite"):
        U.lobpcg_restated(solve, Cs.A, bad, nev, tol, 10)


def test_exact_eigenvectors_take_no_step():
    for n in (37, 101):
        levels, A, a = U.diagonal_case(n)
        order = np.argsort(a)
        X0 = np.zeros((n, 3))
        X0[order[:3], [2, 0, 1]] = [2.0, -1.0, 0.5]  # scaled unit vectors of the three smallest, out of order
        lam, X, res, fl, steps, rank = U.lobpcg_restated(lambda r: r, A, X0, 3, 1e-10, 50)
        assert steps == 0 and fl.tolist() == [0, 0, 0] and lam.tolist() == [1.0, 2.0, 3.0] and not res.any()
        # the random block the GPU test holds to this count: pinned, with its margins, and stable under the noise
        X0 = U.start_block(n, 4, seed=5)
        tr = []
        lam, X, res, fl, steps, rank = U.lobpcg_restated(lambda r: r, A, X0, 2, 1e-9, 400, trace=tr)
        assert fl.tolist() == [0, 0, 2, 2] and np.abs(lam[:2] - [1.0, 2.0]).max() <= 1e-9 * n
        assert steps == {37: 28, 101: 53}[n] and U.decisions_ok(tr, MARGIN)
        for sd in U.NOISE_SEEDS:
            o = U.lobpcg_restated(lambda r: r, A, X0, 2, 1e-9, 400, noise=np.random.default_rng(sd))
            assert o[4] == steps and o[3].tolist() == fl.tolist(), (n, sd)


def test_indefinite_pair_reaches_maxit():
    fixture, k, nev, tol, maxit = U.INDEFINITE
    Cs = U.case(fixture)
    assert Cs.eig[0] < 0 < Cs.eig[-1]
    lam, X, res, fl, steps, rank = U.lobpcg_restated(Cs.O, Cs.A, U.start_block(Cs.n, k), nev, tol, maxit)
    assert fl.tolist() == [2] * k and steps == maxit
