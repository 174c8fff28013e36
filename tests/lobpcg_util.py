"""LOBPCG for the smallest eigenpairs of a Hermitian pair (A, M) as Engine::lobpcg_tile runs it, restated in numpy around a
solve(r) callback in the order of operations of the device, and the inputs the GPU tests use (test_lobpcg_host.py pins them on
the CPU, test_gpu_lobpcg.py holds the driver against them).  numpy / scipy only.

trace (a list) receives one dict per residual test: `ratios` = res_j / tol of every column, and, where the step went on, `rank`
(of the basis [X W P]), `kept` / `dropped` of its pivoted Cholesky."""
import numpy as np
import scipy.sparse as sp

from blockcg_util import _herm, _select, pchol
from lockstep_edges_util import MARGIN, Filtered, diagonal_levels  # noqa: F401

DEFTOL = 1e-12
MAXIT = 200
# test_lobpcg_host.py measures, over every case below, the largest |res_j - ||A x_j - lambda_j x_j|| / ||A||_inf| between the
# recurrence's residual (AX is carried, never recomputed) and the true one, asserts it is below DRIFT and prints it.
DRIFT = 3e-14  # (test_lobpcg_host.test_recurrence_drift prints the measured figure)

# What tests/cpp/lobpcg_small_test.cpp measured against numpy.linalg.eigh on the cases of test_lobpcg_small_host.py, as
# multiples of each case's floor r 2^-52 ||H||_F (the bound is 10 x numpy's own figure, at least the floor):
# largest eigenvalue difference, ||H V - V Theta||_F, ||V^H V - I||_F over all cases.
SMALL_MEASURED = dict(eigenvalues=0.55, residual=0.78, orthogonality=5.0)


def norm_inf(A):
    """largest row sum of |a_ij| (what the engine keeps as A_norm_inf)"""
    return float(abs(sp.csr_matrix(A)).sum(axis=1).max())


def _eigh(H):
    """ascending Hermitian eigendecomposition; ties: lowest index (numpy's order is stable for the sorted values)"""
    w, V = np.linalg.eigh(H)
    return w, V


class StartRefused(Exception):
    pass


def lobpcg_restated(solve, A, X0, nev, tol, maxit, deftol=DEFTOL, Q=None, trace=None, noise=None):
    """-> (lam [k], X [n][k], res [k], flags [k], steps, rank of the last step's basis).  solve(r) is M^{-1} r, filtered where
    the handle filters it; Q (orthonormal columns): the basis filter in force, X0 <- (I - Q Q^H) X0.  Raises StartRefused for
    a non-finite or rank-deficient start block.  noise (a numpy Generator): every apply's result and every entry of the two Grams
    is multiplied by 1 + 2^-52 u, u uniform in [-1, 1] -- what one rounding per element does to the iteration."""
    solve = getattr(solve, "solve", solve)
    A = sp.csr_matrix(A)
    n, k = X0.shape
    s = 3 * k
    cplx = np.iscomplexobj(X0) or np.iscomplexobj(A.data)
    dt = np.complex128 if cplx else np.float64
    anorm = norm_inf(A)
    X = X0.astype(dt)
    if not np.isfinite(X).all():
        raise StartRefused("non-finite")
    if Q is not None:
        X = X - Q @ (Q.conj().T @ X)
    S0, piv, r, bad, _, _ = pchol(_herm(X.conj().T @ X), deftol)
    if bad or r < k:
        raise StartRefused("rank deficient")
    X = X @ _select(S0, piv, k)
    AX = A @ X
    lam, V = _eigh(_herm(X.conj().T @ AX))
    X, AX = X @ V, AX @ V
    P, AP = np.zeros_like(X), np.zeros_like(X)
    flags = np.zeros(k, dtype=np.int32)
    steps, rank = 0, k
    while True:
        R = AX - X * lam[None, :]
        res = np.sqrt(np.array([np.vdot(R[:, j], R[:, j]).real for j in range(k)])) / anorm
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
        AW = A @ W
        steps += 1
        S, AS = np.hstack([X, W, P]), np.hstack([AX, AW, AP])
        GB, GA = _herm(S.conj().T @ S), _herm(S.conj().T @ AS)
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
        th, V = _eigh(_herm(E.conj().T @ GA @ E))
        C = E @ V[:, :k]
        lam = th[:k].copy()
        Cp = C.copy()
        Cp[:k] = 0.0
        X, AX, P, AP = S @ C, AS @ C, S @ Cp, AS @ Cp
    return lam, X, res, flags, steps, rank


def decisions_ok(trace, margin=MARGIN, deftol=DEFTOL):
    """no traced res_j / tol inside [1 / margin, margin]; no kept pivot below 2 deftol and no dropped one above deftol / 2 in
    absolute value.  (A leftover diagonal of 1e-12 of a unit-diagonal Gram of 1024 rows carries rounding of some 1e-14: a
    factor of two either side of deftol is fifty times that.)"""
    for st in trace:
        if any(1.0 / margin <= v <= margin for v in st["ratios"]):
            return False
        if "kept" in st and (st["kept"] < 2.0 * deftol or abs(st["dropped"]) > 0.5 * deftol):
            return False
    return True


def principal_angle(X, Y):
    """sine of the largest principal angle between span X and span Y (orthonormalized here)"""
    Qx, Qy = np.linalg.qr(X)[0], np.linalg.qr(Y)[0]
    return float(np.linalg.norm(Qy - Qx @ (Qx.conj().T @ Qy), 2))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def start_block(n, k, seed=83, cplx=False):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, size=(n, k))
    return X + 1j * rng.uniform(-1, 1, size=(n, k)) if cplx else X


class Case:
    """One fixture with its matrix, oracle, ||A||_inf and dense spectrum.  A name ending in _z: the fixture under the diagonal
    unitary similarity of test_gpu_pcg._phase_similarity, a complex Hermitian pair that the device accepts (herm_24_symm is
    complex SYMMETRIC in its couplings, F = E^T: the restatement runs on it, the device's Hermitian check refuses it)."""

    def __init__(self, name):
        from krylov_edges_util import csr_of
        from oracle import orc
        from util import load_hier

        self.name = name
        self.levels, self.d = load_hier(name[:-2] if name.endswith("_z") else name)
        self.A = csr_of(self.d)
        self.A.sort_indices()
        if name.endswith("_z"):
            from test_gpu_pcg import _phase_similarity

            self.levels, self.A, _ = _phase_similarity(self.levels, self.A)
        self.O = orc.Oracle(self.levels)
        self.cplx = np.iscomplexobj(self.A.data) or self.O.dtype.kind == "c"
        self.anorm = norm_inf(self.A)
        self.n = self.A.shape[0]
        self.eig = np.linalg.eigvalsh(self.A.toarray())
        self.Q = np.linalg.qr(self.d["V"])[0] if "V" in self.d else None


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


# (name, fixture, k, nev, tol, with the fixture's null-space basis installed, restated steps, seed of the start block): tol
# (from 1e-8 and its neighbours) and seed chosen by test_lobpcg_host.py so that decisions_ok holds and the step count is STABLE:
# six restatements with one rounding of noise per element (lobpcg_restated's `noise`) stop where the plain one does.  That is
# not a formality: with nev = k = 15 or 16 on p2d_32_symm (double eigenvalues, no guard columns, the last columns converge at
# the rate of the gap behind the block) most (tol, seed) give counts that move by one or two steps under such noise, and the
# eigenvectors inside a double eigenvalue are rotated by whatever eigensolver runs: no device can be held to such a count.  The
# wide blocks therefore want nev = 11 of 15 and 13 of 16 (both end between two eigenvalue clusters); FULL_BLOCKS are run as
# well and held to everything but the count.
CASES = (
    ("p32_k1", "p2d_32_symm", 1, 1, 1e-8, False, 8, 83),
    ("p32_k2", "p2d_32_symm", 2, 2, 1e-8, False, 11, 83),
    ("p32_k5", "p2d_32_symm", 5, 5, 2e-8, False, 14, 83),
    ("p32_k15", "p2d_32_symm", 15, 11, 1e-8, False, 11, 83),
    ("p32_k16", "p2d_32_symm", 16, 13, 2e-8, False, 12, 83),
    ("p32_k16_nev1", "p2d_32_symm", 16, 1, 1e-8, False, 5, 83),
    ("herm_k6", "herm_24_symm", 6, 6, 2e-8, False, 34, 83),
    ("herm_k16_nev8", "herm_24_symm", 16, 8, 1e-8, False, 20, 83),
    ("neu_k5", "neu2d_32_symm", 5, 5, 1e-8, False, 20, 83),
    ("neu_k5_basis", "neu2d_32_symm", 5, 5, 1e-8, True, 18, 83),
    ("twobody_k4", "twobody_symm", 4, 4, 1e-8, False, 17, 83),
    ("p32z_k5", "p2d_32_symm_z", 5, 5, 2e-8, False, 14, 83),
)
NOISE_SEEDS = (5, 6, 7, 8, 9, 10)
# fixture, k = nev, tol, seed, restated steps: (tol, seed) that pass decisions_ok and the noise test like CASES; the device is
# held to the count within FULL_SPREAD, the spread the restatement's own count shows under that noise at neighbouring (tol, seed)
FULL_BLOCKS = (("p2d_32_symm", 15, 1e-8, 84, 20), ("p2d_32_symm", 16, 2e-8, 85, 19))
FULL_SPREAD = 2
REFUSED_ON_DEVICE = ("herm_k6", "herm_k16_nev8")  # not a Hermitian hierarchy (F != E^H): the device refuses what PCG refuses
INDEFINITE = ("shift2d_32_symm", 4, 4, 1e-8, 40)  # fixture, k, nev, tol, maxit: flag 2


def inputs(name):
    """-> (Case, solve, X0, k, nev, tol, Q)"""
    _, fixture, k, nev, tol, basis, _, seed = next(c for c in CASES if c[0] == name)
    Cs = case(fixture)
    Q = Cs.Q if basis else None
    solve = Filtered(Cs.O, Q) if basis else Cs.O
    return Cs, solve, start_block(Cs.n, k, seed=seed, cplx=Cs.cplx), k, nev, tol, Q


_REF = {}


def reference(name, maxit=MAXIT):
    """-> (inputs(name), (lam, X, res, flags, steps, rank), trace), restated once per process"""
    if (name, maxit) not in _REF:
        inp = inputs(name)
        Cs, solve, X0, k, nev, tol, Q = inp
        tr = []
        _REF[name, maxit] = (inp, lobpcg_restated(solve, Cs.A, X0, nev, tol, maxit, Q=Q, trace=tr), tr)
    return _REF[name, maxit]


def diagonal_case(n, seed=91):
    """M^{-1} = I and A = diag(1 .. n shuffled): eigenvectors are unit vectors -> (levels, A, a)"""
    rng = np.random.default_rng(seed)
    a = rng.permutation(np.arange(1.0, n + 1.0))
    A = sp.csr_matrix(sp.diags(a))
    A.sort_indices()
    return diagonal_levels(np.ones(n)), A, a
