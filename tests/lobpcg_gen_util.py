"""Generalized LOBPCG for the smallest eigenpairs of A x = lambda B x as Engine::lobpcg_tile<true> runs it, restated in numpy
around a solve(r) callback in the order of operations of the device, the mass matrices and the inputs the GPU tests use
(test_lobpcg_gen_host.py pins them on the CPU, test_gpu_lobpcg_gen.py holds the driver against them).  numpy / scipy only.

trace: as lobpcg_util.lobpcg_restated's."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp

import lobpcg_util as U
from blockcg_util import _herm, _select, pchol
from lobpcg_util import DEFTOL, MAXIT, NOISE_SEEDS, StartRefused, decisions_ok, norm_inf, start_block  # noqa: F401

# test_lobpcg_gen_host.py measures, over every case below, the largest |res_j - true backward error of (lambda_j, x_j)| between
# the recurrence's residual (AX and BX are carried, never recomputed) and the true one, asserts it lies in
# [GEN_DRIFT / 10, GEN_DRIFT] and prints it.
GEN_DRIFT = 1e-15  # (test_lobpcg_gen_host.test_recurrence_drift prints the measured figure)


def backward_errors(A, B, lam, X, anorm=None, bnorm=None):
    """||A x_j - lambda_j B x_j||_2 / ((||A||_inf + |lambda_j| ||B||_inf) ||x_j||_2) per column, recomputed from A, B, X"""
    anorm = norm_inf(A) if anorm is None else anorm
    bnorm = norm_inf(B) if bnorm is None else bnorm
    R = A @ X - (B @ X) * lam[None, :]
    return np.linalg.norm(R, axis=0) / ((anorm + np.abs(lam) * bnorm) * np.linalg.norm(X, axis=0))


def lobpcg_gen_restated(solve, A, B, X0, nev, tol, maxit, deftol=DEFTOL, trace=None, noise=None):
    """-> (lam [k], X [n][k], res [k], flags [k], steps, rank of the last step's basis).  solve(r) is M^{-1} r.  Raises
    StartRefused for a start block whose X^H B X is not finite or has Cholesky rank below k.  noise (a numpy Generator): every
    apply's result and every entry of the two Grams is multiplied by 1 + 2^-52 u, u uniform in [-1, 1]."""
    solve = getattr(solve, "solve", solve)
    A, B = sp.csr_matrix(A), sp.csr_matrix(B)
    n, k = X0.shape
    s = 3 * k
    cplx = np.iscomplexobj(X0) or np.iscomplexobj(A.data) or np.iscomplexobj(B.data)
    dt = np.complex128 if cplx else np.float64
    anorm, bnorm = norm_inf(A), norm_inf(B)
    X = X0.astype(dt)
    BX = B @ X
    G = _herm(X.conj().T @ BX)
    if not np.isfinite(G).all():
        raise StartRefused("non-finite")
    S0, piv, r, bad, _, _ = pchol(G, deftol)
    if bad or r < k:
        raise StartRefused("rank deficient, or B not positive definite")
    E = _select(S0, piv, k)
    X, BX = X @ E, BX @ E
    AX = A @ X
    lam, V = np.linalg.eigh(_herm(X.conj().T @ AX))
    X, AX, BX = X @ V, AX @ V, BX @ V
    P, AP, BP = np.zeros_like(X), np.zeros_like(X), np.zeros_like(X)
    flags = np.zeros(k, dtype=np.int32)
    steps, rank = 0, k
    while True:
        R = AX - BX * lam[None, :]
        rr = np.array([np.vdot(R[:, j], R[:, j]).real for j in range(k)])
        xx = np.array([np.vdot(X[:, j], X[:, j]).real for j in range(k)])
        scale = (anorm + np.abs(lam) * bnorm) * np.sqrt(xx)
        with np.errstate(all="ignore"):
            res = np.where(scale == 0.0, np.sqrt(rr), np.sqrt(rr) / np.where(scale == 0.0, 1.0, scale))
            res = np.where(scale > np.finfo(float).max, np.inf, res)
            conv = res <= tol
        if trace is not None:
            trace.append(dict(ratios=(res / tol).tolist()))
        if conv[:nev].all() or steps == maxit:
            flags[:] = np.where(conv, 0, 2)
            break
        W = np.zeros_like(X)
        for j in range(k):
            if not conv[j]:
                W[:, j] = solve(R[:, j].copy())
        if noise is not None:
            W = W * (1.0 + 2.0 ** -52 * noise.uniform(-1, 1, W.shape))
        AW, BW = A @ W, B @ W
        steps += 1
        S, AS, BS = np.hstack([X, W, P]), np.hstack([AX, AW, AP]), np.hstack([BX, BW, BP])
        GB, GA = _herm(S.conj().T @ BS), _herm(S.conj().T @ AS)
        if noise is not None:
            GB = _herm(GB * (1.0 + 2.0 ** -52 * noise.uniform(-1, 1, GB.shape)))
            GA = _herm(GA * (1.0 + 2.0 ** -52 * noise.uniform(-1, 1, GA.shape)))
        dg = GB.diagonal().real
        with np.errstate(all="ignore"):
            D = np.where(dg > 0.0, 1.0 / np.sqrt(np.where(dg > 0.0, dg, 1.0)), 0.0)
        T, piv, r, bad, kept, dropped = pchol(_herm(GB * D[:, None] * D[None, :]), deftol)
        if trace is not None:
            trace[-1].update(rank=r, kept=kept, dropped=dropped)
        if bad or r < k:
            flags[:] = np.where(conv, 0, 1)
            steps -= 1
            break
        rank = r
        E = D[:, None] * _select(T, piv, s)
        th, V = np.linalg.eigh(_herm(E.conj().T @ GA @ E))
        C = E @ V[:, :k]
        lam = th[:k].copy()
        Cp = C.copy()
        Cp[:k] = 0.0
        X, AX, BX, P, AP, BP = S @ C, AS @ C, BS @ C, S @ Cp, AS @ Cp, BS @ Cp
    return lam, X, res, flags, steps, rank


# ---- the mass matrices --------------------------------------------------------------------------------------------------------
def mass2d(nx):
    """the Q1 mass matrix of an nx x nx grid up to its h^2: kron(T, T), T = tridiag(1, 4, 1) / 6"""
    T = sp.diags([np.full(nx - 1, 1.0 / 6.0), np.full(nx, 4.0 / 6.0), np.full(nx - 1, 1.0 / 6.0)], [-1, 0, 1])
    M = sp.csr_matrix(sp.kron(T, T))
    M.sort_indices()
    return M


def lumped(n, seed=3):
    """a lumped (diagonal) mass matrix: uniform[0.5, 2] of default_rng(seed)"""
    M = sp.csr_matrix(sp.diags(np.random.default_rng(seed).uniform(0.5, 2.0, n)))
    M.sort_indices()
    return M


def phase(n, seed=3):
    """the diagonal of the Phi of test_gpu_pcg._phase_similarity (what lobpcg_util.Case puts the _z fixtures under)"""
    return np.exp(1j * np.random.default_rng(seed).uniform(0, 2 * np.pi, n))


def mass_of(fixture):
    """the mass matrix that goes with a fixture of lobpcg_util.case: mass2d for the Poisson grids (Phi B Phi^H, complex
    Hermitian, for the _z ones), the lumped diagonal for twobody_symm"""
    Cs = U.case(fixture)
    if fixture.startswith("twobody"):
        return lumped(Cs.n)
    nx = int(round(np.sqrt(Cs.n)))
    assert nx * nx == Cs.n
    B = mass2d(nx)
    if fixture.endswith("_z"):
        phi = phase(Cs.n)
        Z = sp.csr_matrix(sp.diags(phi) @ B.astype(np.complex128) @ sp.diags(phi.conj()))
        up = sp.triu(Z, 1)  # (the products round: the strict upper triangle mirrored and a real diagonal are exactly Hermitian)
        B = sp.csr_matrix(up + up.conj().T + sp.diags(Z.diagonal().real))
        B.sort_indices()
    return B


_GEIG = {}


def pencil_eigenvalues(fixture):
    """scipy.linalg.eigh(A, B) eigenvalues of the fixture's pencil, once per process"""
    if fixture not in _GEIG:
        Cs = U.case(fixture)
        _GEIG[fixture] = scipy.linalg.eigh(Cs.A.toarray(), mass_of(fixture).toarray(), eigvals_only=True)
    return _GEIG[fixture]


# (name, fixture, k, nev, tol, restated steps, seed of the start block): chosen like lobpcg_util.CASES -- tol from 1e-8 and its
# neighbours and the seed such that decisions_ok holds and the step count is the same under the six one-rounding noise seeds
# (test_lobpcg_gen_host.py).  k = 1, 2, 5, 15, 16 give s = 3, 6, 15, 45, 48: one, two and three 16-column tiles and the padded
# last tile; the wide blocks carry guard columns for the reason lobpcg_util.CASES gives.
GEN_CASES = (
    ("p32_k1", "p2d_32_symm", 1, 1, 1e-8, 8, 83),
    ("p32_k2", "p2d_32_symm", 2, 2, 1e-8, 11, 83),
    ("p32_k5", "p2d_32_symm", 5, 5, 2e-8, 13, 83),
    ("p32_k15", "p2d_32_symm", 15, 11, 1e-8, 11, 83),
    ("p32_k16", "p2d_32_symm", 16, 13, 1e-8, 12, 83),
    ("p32z_k5", "p2d_32_symm_z", 5, 5, 2e-8, 14, 83),
    ("twobody_k4", "twobody_symm", 4, 4, 1e-8, 16, 83),
)
# B = I given explicitly, on p32 and p32z with k = 5, seed 83: through step BIT_EQUAL_MAXIT no column is converged under the
# standard driver's scaling or under the generalized one (every res_j / tol above MARGIN at every test), so neither path locks
# a column and lobpcg_gen(maxit = m) must return the bits of lobpcg(maxit = m).  Pinned by test_lobpcg_gen_host.py.
BIT_EQUAL = ("p32_k5", "p32z_k5")
BIT_EQUAL_MAXIT = 5


def inputs(name):
    """-> (Case, solve, B, X0, k, nev, tol)"""
    _, fixture, k, nev, tol, _, seed = next(c for c in GEN_CASES if c[0] == name)
    Cs = U.case(fixture)
    return Cs, Cs.O, mass_of(fixture), start_block(Cs.n, k, seed=seed, cplx=Cs.cplx), k, nev, tol


_REF = {}


def reference(name, maxit=MAXIT):
    """-> (inputs(name), (lam, X, res, flags, steps, rank), trace), restated once per process"""
    if (name, maxit) not in _REF:
        inp = inputs(name)
        Cs, solve, B, X0, k, nev, tol = inp
        tr = []
        _REF[name, maxit] = (inp, lobpcg_gen_restated(solve, Cs.A, B, X0, nev, tol, maxit, trace=tr), tr)
    return _REF[name, maxit]


def diagonal_mass(n, seed=97):
    """B = diag of powers of two, 1/4, 1 or 4, for lobpcg_util.diagonal_case: the quotients a / b are exact, and so are the
    B-normalized unit vectors (the square roots are powers of two)"""
    b = 4.0 ** np.random.default_rng(seed).integers(-1, 2, n)
    B = sp.csr_matrix(sp.diags(b))
    B.sort_indices()
    return B, b


DIAGONAL_STEPS = {37: 51, 101: 53}  # restated steps of the random block on the diagonal pencils (test_lobpcg_gen_host.py)
