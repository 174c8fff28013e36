"""GPU (-m gpu): the null-space search (hifamd_nsp_find, HIF.find_nullspace / nsp_basis) on the three singular fixtures
of tests/golden/make_golden_nsp.py (a pure-Neumann Laplacian, two floating bodies with a null space of dimension 2, a
nonsymmetric periodic convection-diffusion matrix with different left and right null vectors), on two nonsingular
ones, on the complex twin of a symmetric one, and on the 1M-row Neumann Laplacian where the compiled reference
travelled.  Nothing here hands the library a null vector: what it finds is compared with the fixture's.

Tolerances: rtol = 1e-10 and tol = 1e-8 on the 1k-row fixtures (the bound rtol sqrt(n) = 3.2e-9 of include/hifir_amd.h
lies below tol); orthonormality 1e-12 (the project's apply tolerance); the subspace bound is derived, not chosen:
for any unit q, ||(I - P_null) q|| <= ||A q|| / sigma_min+(A), because A acts on the part of q outside null(A) with at
least its smallest nonzero singular value -- sigma_min+ comes from a dense SVD (closed form at 1M rows), ||A q|| is
recomputed in numpy, plus 1e-12 ||A||_inf for its rounding.  Krylov results after install agree with the same call
after set_nsp_basis(fixture V) within 10 times the driver's rtol, the bound tests/test_gpu_nsp_basis.py uses."""
import numpy as np
import pytest
import scipy.sparse as sp

import hifir_amd
from oracle import ref
from test_gpu_pcg import _phase_similarity
from test_nsp_find_host import _probe_numpy
from util import load_hier, relerr

pytestmark = pytest.mark.gpu

RTOL, TOL = 1e-10, 1e-8
NAMES = ["neu2d_32_symm", "twobody_symm", "pcd2d_32"]
SYMM = ["neu2d_32_symm", "twobody_symm"]
NULLITY = {"neu2d_32_symm": 1, "twobody_symm": 2, "pcd2d_32": 1}


def _matrix(d):
    n = len(d["b"])
    return sp.csr_matrix((d["A_vals"], d["A_indices"], d["A_indptr"]), shape=(n, n))


def _orth(V):
    return np.linalg.qr(V.reshape(V.shape[0], -1))[0]


def _norm_inf(A):
    return float(abs(A).sum(axis=1).max())


def _sigma_min_plus(A, k):
    """smallest nonzero singular value of a matrix of nullity k (dense SVD)"""
    s = np.linalg.svd(A.toarray(), compute_uv=False)
    assert s[-k] <= 1e-13 * s[0] < s[-k - 1]
    return float(s[-k - 1])


_CACHE = {}


def _fixture(name):
    """(levels, data, handle with the matrix and NO filter, A)"""
    if name not in _CACHE:
        levels, d = load_hier(name)
        M = hifir_amd.HIF.from_levels(levels, max_nrhs=64)
        M.set_matrix(d["A_indptr"], d["A_indices"], d["A_vals"])
        _CACHE[name] = (levels, d, M, _matrix(d))
    M = _CACHE[name][2]
    M.set_nsp_basis(None)
    M.set_nsp_basis(None, trans=True)
    M.set_nsp_const(1, 0)
    M.set_nsp_const(1, 0, trans=True)
    return _CACHE[name]


def _check_basis(tag, A, Q, resid, found, QV, sigma):
    """Everything the search promises about its result, recomputed in numpy.  A: the matrix whose null space was sought
    (A^H for trans), QV: orthonormal basis of the expected null space."""
    na = _norm_inf(A)
    assert Q.shape == (A.shape[0], found)
    assert np.all(resid[:found] <= TOL), (tag, resid)
    assert np.all(resid[found:] > TOL), (tag, resid)
    aq = np.linalg.norm(A @ Q, axis=0)
    orth = np.abs(Q.conj().T @ Q - np.eye(found)).max()
    out = np.linalg.norm(Q - QV @ (QV.conj().T @ Q), axis=0)
    bound = (aq + 1e-12 * na) / sigma
    print(tag, "found", found, "resid", resid[:found], "smallest other", resid[found:].min(), "|A q|/|A|inf", aq / na,
          "|Q^H Q - I|", orth, "sin to fixture", out, "bound", bound)
    assert np.all(aq <= TOL * na), (tag, aq / na)
    assert np.all(np.abs(aq / na - resid[:found]) <= 1e-12 + 1e-6 * resid[:found]), (tag, aq / na, resid[:found])
    assert orth <= 1e-12, (tag, orth)
    assert np.all(out <= bound), (tag, out, bound)


# ---- 1. what is found, against the fixture ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_finds_the_fixtures_null_space(name):
    levels, d, M, A = _fixture(name)
    k = NULLITY[name]
    Q, resid, info = M.find_nullspace(tol=TOL, rtol=RTOL, install=False)
    print(name, info)
    assert Q.shape[1] == k and info["nonfinite"] == 0 and info["unconverged"] == 0 and info["maybe_more"] == 0
    assert 1 <= info["iters"] <= 60
    _check_basis(name, A, Q, resid, k, _orth(d["V"]), _sigma_min_plus(A, k))
    assert M.nsp_dim() == 0 and M.nsp_basis() is None  # install=False
    # full rank of the dense level as well
    Q2, resid2, info2 = M.find_nullspace(tol=TOL, rtol=RTOL, install=False, full_rank=True)
    _check_basis(name + " full_rank", A, Q2, resid2, k, _orth(d["V"]), _sigma_min_plus(A, k))


def test_left_null_space():
    levels, d, M, A = _fixture("pcd2d_32")
    AH = A.conj().T.tocsr()
    Q, resid, info = M.find_nullspace(tol=TOL, rtol=RTOL, trans=True, install=False)
    assert Q.shape[1] == 1 and info["nonfinite"] == 0 and info["unconverged"] == 0
    _check_basis("pcd2d_32 trans", AH, Q, resid, 1, _orth(d["VL"]), _sigma_min_plus(AH, 1))
    # the left null vector is not the right one: the check above could tell them apart
    assert np.linalg.norm(Q - _orth(d["V"]) @ (_orth(d["V"]).T @ Q)) > 1e-2
    assert M.nsp_dim(trans=True) == 0 and M.nsp_dim() == 0


@pytest.mark.parametrize("name", SYMM)
def test_left_is_right_for_a_symmetric_matrix(name):
    levels, d, M, A = _fixture(name)
    k = NULLITY[name]
    Q, resid, info = M.find_nullspace(tol=TOL, rtol=RTOL, trans=True, install=False)
    assert Q.shape[1] == k
    _check_basis(name + " trans", A, Q, resid, k, _orth(d["V"]), _sigma_min_plus(A, k))


# ---- 2. bits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_bits_probe_generator_repeatability_and_suspension(name):
    levels, d, M, A = _fixture(name)
    n = len(d["b"])
    for seed in (0, 12345):
        Q0, r0, i0 = M.find_nullspace(tol=TOL, rtol=RTOL, install=False, seed=seed)
        Q1, r1, i1 = M.find_nullspace(tol=TOL, rtol=RTOL, install=False, seed=seed, X0=_probe_numpy(n, seed, False))
        assert np.array_equal(Q0, Q1) and np.array_equal(r0, r1) and i0 == i1, seed  # the device generator IS the formula
        Q2, r2, i2 = M.find_nullspace(tol=TOL, rtol=RTOL, install=False, seed=seed)
        assert np.array_equal(Q0, Q2) and np.array_equal(r0, r2) and i0 == i2, seed
    Qa, ra, _ = M.find_nullspace(tol=TOL, rtol=RTOL, install=False, seed=0)
    Qb, rb, _ = M.find_nullspace(tol=TOL, rtol=RTOL, install=False, seed=12345)
    assert not np.array_equal(Qa, Qb)  # (another seed, other probes: the comparisons above mean something)
    b = d["b"]
    x_plain = M.solve(b)
    # a basis filter in force (a vector that is NOT a null vector: the search must not see it)
    W = np.random.default_rng(5).uniform(-1, 1, size=(n, 3))
    M.set_nsp_basis(W)
    x_w = M.solve(b)
    assert not np.array_equal(x_w, x_plain)
    Qw, rw, _ = M.find_nullspace(tol=TOL, rtol=RTOL, install=False, seed=0)
    assert np.array_equal(Qw, Qa) and np.array_equal(rw, ra)
    assert M.nsp_dim() == 3 and np.array_equal(M.solve(b), x_w)  # still in force, same bits
    assert np.array_equal(M.nsp_basis(), M.nsp_basis()) and relerr(M.nsp_basis(), _orth(W) * np.sign(np.sum(_orth(W) * M.nsp_basis(), axis=0))) <= 1e-12
    # a constant-mode filter in force
    M.set_nsp_const(0, -1)
    x_c = M.solve(b)
    assert M.nsp_dim() == 0 and not np.array_equal(x_c, x_plain)
    Qc, rc, _ = M.find_nullspace(tol=TOL, rtol=RTOL, install=False, seed=0)
    assert np.array_equal(Qc, Qa) and np.array_equal(rc, ra)
    assert M.nsp_dim() == 0 and M.nsp_basis() is None and np.array_equal(M.solve(b), x_c)
    # the other op's filter is not touched either
    M.set_nsp_const(1, 0)
    M.set_nsp_basis(W, trans=True)
    xt_w = M.solve(b, trans=True)
    M.find_nullspace(tol=TOL, rtol=RTOL, install=True, seed=0)
    assert M.nsp_dim(trans=True) == 3 and np.array_equal(M.solve(b, trans=True), xt_w)


# ---- 3. install, and the payoff: no user-supplied vector anywhere ---------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_install_and_read_back(name):
    levels, d, M, A = _fixture(name)
    n = len(d["b"])
    k = NULLITY[name]
    assert M.stats_ext()["nsp_basis_bytes"] == 0.0
    M.set_nsp_const(0, -1)  # (replaced by the installed basis: one filter per op)
    Q, resid, info = M.find_nullspace(tol=TOL, rtol=RTOL)
    assert Q.shape[1] == k and M.nsp_dim() == k
    assert np.array_equal(M.nsp_basis(), Q)
    assert M.nsp_basis(trans=True) is None
    assert M.stats_ext()["nsp_basis_bytes"] == n * 8 * {1: 1, 2: 2}[k]
    # the filter in force is x - Q (Q^H x)
    X = np.random.default_rng(3).uniform(-1, 1, size=(n, 5))
    assert relerr(M.nsp_filter(X.copy()), X - Q @ (Q.T @ X)) <= 1e-12
    # a second search replaces it by the same bits; kmax below the nullity installs the leading vectors
    Q2, _, _ = M.find_nullspace(tol=TOL, rtol=RTOL)
    assert np.array_equal(Q2, Q) and np.array_equal(M.nsp_basis(), Q)
    M.set_nsp_basis(None)
    assert M.nsp_dim() == 0 and M.nsp_basis() is None and M.stats_ext()["nsp_basis_bytes"] == 0.0


@pytest.mark.parametrize("name", SYMM)
def test_projected_pcg_after_find_equals_pcg_after_set_basis(name):
    levels, d, M, A = _fixture(name)
    rtol = 1e-6
    B = np.stack([d["b"], d["bstar"]], axis=1)
    Q, _, _ = M.find_nullspace(tol=TOL, rtol=RTOL)
    X, fl, it = M.pcg(B, rtol=rtol, maxit=300)
    M.set_nsp_basis(d["V"])
    Xv, fv, iv = M.pcg(B, rtol=rtol, maxit=300)
    print(name, "pcg after find", fl, it, "after set_nsp_basis", fv, iv, "difference", [relerr(X[:, c], Xv[:, c]) for c in (0, 1)])
    assert fl.tolist() == [0, 0] and fv.tolist() == [0, 0]
    for c in (0, 1):
        assert relerr(X[:, c], Xv[:, c]) <= 10 * rtol, c
    QV = _orth(d["V"])
    PB = B - QV @ (QV.T @ B)
    assert (np.linalg.norm(A @ X - PB, axis=0) / np.linalg.norm(PB, axis=0)).max() <= 10 * rtol


def test_bicgstab_and_gmres_after_find_equal_the_calls_after_set_basis():
    """pcd2d_32: the fixture's b is not in range(A), and BiCGSTAB / GMRES take the right-hand side as it is -- it is made
    consistent with the LEFT null vector, found (first run) or the fixture's (second run); the right one filters the
    applies.  No vector of the first run comes from the caller."""
    levels, d, M, A = _fixture("pcd2d_32")
    rtol = 1e-6
    b = d["b"]
    QL, _, _ = M.find_nullspace(tol=TOL, rtol=RTOL, trans=True, install=False)
    Q, _, _ = M.find_nullspace(tol=TOL, rtol=RTOL)
    assert QL.shape[1] == 1 and Q.shape[1] == 1 and M.nsp_dim() == 1
    bc = b - QL @ (QL.T @ b)
    xb, fb, ib = M.bicgstab(bc, rtol=rtol, maxit=400)
    xg, fg, ig = M.gmres(bc, restart=30, rtol=rtol, maxit=500)
    M.set_nsp_basis(d["V"])
    QLv = _orth(d["VL"])
    bv = b - QLv @ (QLv.T @ b)
    xbv, fbv, ibv = M.bicgstab(bv, rtol=rtol, maxit=400)
    xgv, fgv, igv = M.gmres(bv, restart=30, rtol=rtol, maxit=500)
    print("bicgstab", (fb, ib), (fbv, ibv), relerr(xb, xbv), "gmres", (fg, ig), (fgv, igv), relerr(xg, xgv))
    assert (fb, fbv, fg, fgv) == (0, 0, 0, 0)
    assert relerr(xb, xbv) <= 10 * rtol and relerr(xg, xgv) <= 10 * rtol
    for x in (xb, xg):
        assert np.linalg.norm(A @ x - bv) / np.linalg.norm(bv) <= 10 * rtol


# ---- 4. nothing to find; kmax ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p2d_30", "cd2d_48"])
def test_nonsingular_matrix_has_no_null_space(name):
    levels, d, M, A = _fixture(name)
    n = len(d["b"])
    W = np.random.default_rng(7).uniform(-1, 1, size=(n, 2))
    M.set_nsp_basis(W)
    x_w = M.solve(d["b"])
    Qw = M.nsp_basis()
    for trans in (False, True):
        Q, resid, info = M.find_nullspace(tol=TOL, rtol=RTOL, trans=trans)  # (success: no exception)
        print(name, "trans", trans, info, "smallest resid", resid.min())
        assert Q.shape == (n, 0) and info["nonfinite"] == 0 and info["maybe_more"] == 0
        assert np.all(resid > TOL)
    assert M.nsp_dim() == 2 and np.array_equal(M.nsp_basis(), Qw) and np.array_equal(M.solve(d["b"]), x_w)  # untouched
    assert M.nsp_dim(trans=True) == 0


def test_kmax_below_and_above_the_nullity():
    levels, d, M, A = _fixture("twobody_symm")
    Q16, r16, i16 = M.find_nullspace(kmax=16, tol=TOL, rtol=RTOL, install=False)
    assert Q16.shape[1] == 2 and i16["maybe_more"] == 0
    Q1, r1, i1 = M.find_nullspace(kmax=1, tol=TOL, rtol=RTOL)
    assert Q1.shape[1] == 1 and i1["maybe_more"] == 1
    assert np.array_equal(Q1[:, 0], Q16[:, 0]) and np.array_equal(r1, r16)  # the leading column; all 16 residuals
    assert M.nsp_dim() == 1 and np.array_equal(M.nsp_basis(), Q1)
    Q2, _, i2 = M.find_nullspace(kmax=2, tol=TOL, rtol=RTOL)
    assert np.array_equal(Q2, Q16) and i2["maybe_more"] == 0 and M.nsp_dim() == 2


def test_nonfinite_probes_find_nothing():
    levels, d, M, A = _fixture("neu2d_32_symm")
    n = len(d["b"])
    W = np.random.default_rng(9).uniform(-1, 1, size=(n, 1))
    M.set_nsp_basis(W)
    X0 = _probe_numpy(n, 0, False).copy()
    X0[17, 3] = np.nan
    Q, resid, info = M.find_nullspace(tol=TOL, rtol=RTOL, X0=X0, maxit=40)
    assert Q.shape == (n, 0) and info["nonfinite"] == 1
    assert M.nsp_dim() == 1  # the filter in force is put back


# ---- 5. complex -------------------------------------------------------------------------------------------------------
def test_complex_twin():
    """A' = Phi A Phi^H, M'^{-1} = Phi M^{-1} Phi^H (tests/test_gpu_pcg.py _phase_similarity): null(A') = Phi null(A)."""
    levels, d, M, A = _fixture("twobody_symm")
    lz, Az, phi = _phase_similarity(levels, A)
    Az = sp.csr_matrix(Az)
    Az.sort_indices()
    n = A.shape[0]
    Mz = hifir_amd.HIF.from_levels(lz, max_nrhs=64)
    Mz.set_matrix(Az.indptr, Az.indices, Az.data)
    Q, resid, info = Mz.find_nullspace(tol=TOL, rtol=RTOL)
    assert Q.dtype == np.complex128 and Q.shape[1] == 2 and info["nonfinite"] == 0 and info["unconverged"] == 0
    _check_basis("twobody_symm complex", Az, Q, resid, 2, _orth(phi[:, None] * d["V"]), _sigma_min_plus(A, 2))
    assert np.abs(Q.imag).max() > 1e-3  # (complex data: the imaginary parts carry the phases)
    assert Mz.nsp_dim() == 2 and np.array_equal(Mz.nsp_basis(), Q)
    # explicit complex probes restate the device generator here as well
    Q1, r1, _ = Mz.find_nullspace(tol=TOL, rtol=RTOL, X0=_probe_numpy(n, 0, True), install=False)
    assert np.array_equal(Q1, Q) and np.array_equal(r1, resid)
    # the left null space of a Hermitian matrix is the right one
    QT, rT, _ = Mz.find_nullspace(tol=TOL, rtol=RTOL, trans=True, install=False)
    _check_basis("twobody_symm complex trans", Az, QT, rT, 2, _orth(phi[:, None] * d["V"]), _sigma_min_plus(A, 2))


# ---- 6. 1M rows ---------------------------------------------------------------------------------------------------
def _neumann2d(nx):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx), format="lil")
    T[0, 0] = 1.0
    T[nx - 1, nx - 1] = 1.0
    T = T.tocsr()
    I = sp.identity(nx, format="csr")
    A = (sp.kron(I, T) + sp.kron(T, I)).tocsr()
    A.sort_indices()
    return A


@pytest.mark.skipif(not ref.available(), reason="compiled reference not present")
def test_1m_neumann_null_space_is_the_constants():
    """The 1000^2 pure-Neumann Laplacian factorized with is_symm by the compiled reference, with the defaults
    rtol = 1e-10, tol = 1e-7, maxit = 500.  sigma_min+ = 2 - 2 cos(pi / 1000) (closed form: the smallest nonzero
    eigenvalue of the 1-D Neumann matrix plus the zero eigenvalue of the other direction)."""
    A = _neumann2d(1000)
    n = A.shape[0]
    R = ref.RefHIF(A.indptr, A.indices, A.data, ref.make_params(is_symm=1))
    M = hifir_amd.HIF.from_levels(R.levels(), max_nrhs=16)
    M.set_matrix(A.indptr, A.indices, A.data)
    Q, resid, info = M.find_nullspace()
    print("1M find_nullspace", info, "resid[0]", resid[0], "smallest other", resid[1:].min())
    assert Q.shape[1] == 1 and info["unconverged"] == 0 and info["nonfinite"] == 0
    assert resid[0] <= 1e-7 and np.all(resid[1:] > 1e-7)
    q = Q[:, 0]
    sigma = 2.0 - 2.0 * np.cos(np.pi / 1000)
    aq = np.linalg.norm(A @ q)
    dev = np.linalg.norm(q - q.mean())
    print("1M |A q|", aq, "|q - mean(q)|", dev, "bound", (aq + 1e-12 * 8.0) / sigma, "| |q| - 1 |", abs(np.linalg.norm(q) - 1.0))
    assert abs(np.linalg.norm(q) - 1.0) <= 1e-12
    assert dev <= (aq + 1e-12 * 8.0) / sigma
    assert M.nsp_dim() == 1
