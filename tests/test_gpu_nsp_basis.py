"""GPU (-m gpu): the basis mode of the null-space filter (hifamd_set_nsp_basis, HIF.set_nsp_basis / nsp_filter) and the
drivers that run through it, on three singular fixtures (tests/golden/make_golden_nsp.py: a pure-Neumann Laplacian,
two floating bodies with a non-constant null space of dimension 2, a nonsymmetric periodic convection-diffusion matrix
with different left and right null vectors): the filter and the filtered applies against numpy x - Q (Q^H x) around
the unfiltered device result, batch-width independence of the bits, the adjoint filter, projected PCG, BiCGSTAB, GMRES
and fixed-sweep refinement against numpy restatements around the oracle's apply, and the 1M-row Neumann Laplacian
where the compiled reference travelled.  Tolerances are the project's own: 1e-12 for applies, 1e-8 and 10 rtol for
Krylov results."""
import numpy as np
import pytest
import scipy.sparse as sp

import hifir_amd
from oracle import orc, ref
from test_gpu_pcg import _phase_similarity
from util import load_hier, relerr

pytestmark = pytest.mark.gpu

BAD_PREC = 3
NAMES = ["neu2d_32_symm", "twobody_symm", "pcd2d_32"]
SYMM = ["neu2d_32_symm", "twobody_symm"]
WIDTHS = [1, 5, 64, 70]


def _matrix(d):
    n = len(d["b"])
    return sp.csr_matrix((d["A_vals"], d["A_indices"], d["A_indptr"]), shape=(n, n))


def _orth(V):
    return np.linalg.qr(V.reshape(V.shape[0], -1))[0]


def _proj(Q, X):
    return X - Q @ (Q.conj().T @ X)


_CACHE = {}


def _fixture(name):
    """(levels, data, handle with the matrix and NO filter, oracle, A, Q of the right null space)"""
    if name not in _CACHE:
        levels, d = load_hier(name)
        M = hifir_amd.HIF.from_levels(levels, max_nrhs=64)
        M.set_matrix(d["A_indptr"], d["A_indices"], d["A_vals"])
        _CACHE[name] = (levels, d, M, orc.Oracle(levels), _matrix(d), _orth(d["V"]))
    M = _CACHE[name][2]
    M.set_nsp_basis(None)
    M.set_nsp_basis(None, trans=True)
    M.set_nsp_const(1, 0)
    return _CACHE[name]


def _qnorm(Q, X):
    """|Q^H x| / ||x|| per column"""
    X = X.reshape(X.shape[0], -1)
    return np.linalg.norm(Q.conj().T @ X, axis=0) / np.linalg.norm(X, axis=0)


# ---- 3. the filter and the filtered applies -----------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_filter_and_filtered_apply_vs_numpy(name):
    levels, d, M, O, A, Q = _fixture(name)
    n = len(d["b"])
    rng = np.random.default_rng(41)
    for w in WIDTHS:
        B = rng.uniform(-1, 1, size=(n, w))
        X0 = M.solve_mrhs(B)  # unfiltered
        assert M.nsp_dim() == 0
        assert np.array_equal(M.nsp_filter(X0.copy()), X0)  # no filter set: the block is left as it is
        M.set_nsp_basis(d["V"])
        assert M.nsp_dim() == d["V"].shape[1]
        want = _proj(Q, X0)
        Xf = M.solve_mrhs(B)
        assert relerr(Xf, want) <= 1e-12, (name, w, relerr(Xf, want))
        assert np.abs(Q.conj().T @ Xf).max() <= 1e-12 * np.abs(Xf).max()
        Y = X0.copy()
        assert M.nsp_filter(Y) is Y
        assert relerr(Y, want) <= 1e-12
        assert np.abs(Q.conj().T @ Y).max() <= 1e-12 * np.abs(Y).max()
        Y2 = M.nsp_filter(Y.copy())  # a second time moves nothing
        assert relerr(Y2, Y) <= 1e-12
        # a right-hand side (entries of order 1, a large component along Q) as well
        Bf = M.nsp_filter(B.copy())
        assert relerr(Bf, _proj(Q, B)) <= 1e-12
        if w == 1:
            x = M.solve(B[:, 0].copy())
            assert np.array_equal(x, Xf[:, 0])
            y = M.nsp_filter(X0[:, 0].copy())
            assert y.ndim == 1 and np.array_equal(y, Y[:, 0])
        M.set_nsp_basis(None)
        assert M.nsp_dim() == 0
        assert np.array_equal(M.solve_mrhs(B), X0)  # the unfiltered bits, exactly
    assert M.stats_ext()["nsp_basis_bytes"] == 0.0
    M.set_nsp_basis(d["V"])
    assert M.stats_ext()["nsp_basis_bytes"] == n * 8 * {1: 1, 2: 2}[d["V"].shape[1]]


def test_ones_basis_is_the_reference_constant_filter():
    levels, d, M, O, A, Q = _fixture("neu2d_32_symm")
    M.set_nsp_basis(np.ones(len(d["b"])))  # (n,) is one vector
    assert M.nsp_dim() == 1
    x = M.solve(d["b"])
    assert relerr(x, d["x_nspc"]) <= 1e-12, relerr(x, d["x_nspc"])


@pytest.mark.parametrize("k", [3, 16])
def test_random_basis_real_and_complex(k):
    levels, d, M, O, A, Q1 = _fixture("neu2d_32_symm")
    n = len(d["b"])
    rng = np.random.default_rng(100 + k)
    V = rng.uniform(-1, 1, size=(n, k))
    Q = _orth(V)
    B = rng.uniform(-1, 1, size=(n, 70))
    X0 = M.solve_mrhs(B)
    M.set_nsp_basis(V)
    assert M.nsp_dim() == k
    Xf = M.solve_mrhs(B)
    assert relerr(Xf, _proj(Q, X0)) <= 1e-12
    assert np.abs(Q.T @ Xf).max() <= 1e-12 * np.abs(Xf).max()
    # the complex hierarchy (a diagonal unitary similarity of the real one), V transformed alike plus an imaginary part
    lz, Az, phi = _phase_similarity(levels, A)
    Mz = hifir_amd.HIF.from_levels(lz, max_nrhs=64)
    Vz = phi[:, None] * (V + 1j * rng.uniform(-1, 1, size=(n, k)))
    Qz = _orth(Vz)
    Bz = rng.uniform(-1, 1, size=(n, 70)) + 1j * rng.uniform(-1, 1, size=(n, 70))
    Z0 = Mz.solve_mrhs(Bz)
    Mz.set_nsp_basis(Vz)
    assert Mz.nsp_dim() == k
    Zf = Mz.solve_mrhs(Bz)
    assert relerr(Zf, _proj(Qz, Z0)) <= 1e-12
    assert np.abs(Qz.conj().T @ Zf).max() <= 1e-12 * np.abs(Zf).max()
    Y = Mz.nsp_filter(Z0.copy())
    assert relerr(Y, _proj(Qz, Z0)) <= 1e-12
    assert relerr(Mz.nsp_filter(Y.copy()), Y) <= 1e-12
    # M'^{-1} = Phi M^{-1} Phi^H and Q' = Phi Q: the real filter is the complex one on transformed data
    Mz.set_nsp_basis(phi[:, None] * V)
    assert relerr(Mz.solve_mrhs(phi[:, None] * B), phi[:, None] * Xf) <= 1e-12
    for c in (0, 69):
        assert np.array_equal(Mz.solve(Bz[:, c].copy()), Mz.solve_mrhs(Bz)[:, c])


def test_dependent_zero_and_nonfinite_vectors_are_refused():
    levels, d, M, O, A, Q = _fixture("twobody_symm")
    V = d["V"]
    X0 = M.solve(d["b"])
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.set_nsp_basis(np.column_stack([V, V.sum(axis=1)]))
    assert e.value.code == BAD_PREC and "vector 2" in e.value.msg and "depend" in e.value.msg
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.set_nsp_basis(np.column_stack([V[:, 0], np.zeros(len(V))]))
    assert e.value.code == BAD_PREC and "vector 1" in e.value.msg
    Vn = V.copy()
    Vn[5, 0] = np.nan
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.set_nsp_basis(Vn)
    assert e.value.code == BAD_PREC and "vector 0" in e.value.msg
    assert M.nsp_dim() == 0 and np.array_equal(M.solve(d["b"]), X0)  # a refused basis leaves no filter behind
    # ... and does not disturb one that is in force
    M.set_nsp_basis(V)
    Xf = M.solve(d["b"])
    with pytest.raises(hifir_amd.HifAmdError):
        M.set_nsp_basis(Vn)
    assert M.nsp_dim() == 2 and np.array_equal(M.solve(d["b"]), Xf)


# ---- 4. bits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_filtered_bits_do_not_depend_on_the_batch(name):
    import torch

    levels, d, M, O, A, Q = _fixture(name)
    M.set_nsp_basis(d["V"])
    n = len(d["b"])
    B = np.random.default_rng(43).uniform(-1, 1, size=(n, 70))
    X70 = M.solve_mrhs(B)
    X64 = M.solve_mrhs(np.ascontiguousarray(B[:, :64]))
    X5 = M.solve_mrhs(np.ascontiguousarray(B[:, :5]))
    assert np.array_equal(X64, X70[:, :64]) and np.array_equal(X5, X70[:, :5])
    for c in (0, 3, 63, 64, 69):
        assert np.array_equal(M.solve(B[:, c].copy()), X70[:, c]), c
    F70 = M.nsp_filter(B.copy())
    assert np.array_equal(M.nsp_filter(np.ascontiguousarray(B[:, :64])), F70[:, :64])
    assert np.array_equal(M.nsp_filter(np.ascontiguousarray(B[:, :5])), F70[:, :5])
    for c in (0, 4, 63, 64, 69):
        assert np.array_equal(M.nsp_filter(B[:, c].copy()), F70[:, c]), c
    # the torch-device entries give the host entries' bits; a block with a row stride of its own as well
    for w in (5, 64, 70):
        Bd = torch.from_numpy(np.ascontiguousarray(B[:, :w])).cuda()
        Xd, Fd = M.solve_mrhs(Bd), M.nsp_filter(Bd.clone())
        M.sync()  # (the device entries enqueue on the handle's stream and do not wait)
        assert np.array_equal(Xd.cpu().numpy(), X70[:, :w])
        assert np.array_equal(Fd.cpu().numpy(), F70[:, :w])
    b3, b4 = torch.from_numpy(B[:, 3].copy()).cuda(), torch.from_numpy(B[:, 4].copy()).cuda()  # (kept alive until the sync)
    xd, fd = M.solve(b3), M.nsp_filter(b4)
    M.sync()
    assert np.array_equal(xd.cpu().numpy(), X70[:, 3])
    assert np.array_equal(fd.cpu().numpy(), F70[:, 4])
    wide = torch.from_numpy(B).cuda()
    view = wide[:, 10:15]  # row stride 70, 5 columns
    M.nsp_filter(view)
    M.sync()
    got = wide.cpu().numpy()
    assert np.array_equal(got[:, 10:15], F70[:, 10:15]) and np.array_equal(got[:, :10], B[:, :10])
    assert np.array_equal(got[:, 15:], B[:, 15:])


# ---- 5. the adjoint filter; one filter per op -----------------------------------------------------------------------
def test_adjoint_filter_and_replacement():
    levels, d, M, O, A, Q = _fixture("pcd2d_32")
    n = len(d["b"])
    QL = _orth(d["VL"])
    B = np.random.default_rng(47).uniform(-1, 1, size=(n, 5))
    X0, XT0 = M.solve_mrhs(B), M.solve_mrhs(B, trans=True)
    M.set_nsp_basis(d["V"])
    assert (M.nsp_dim(), M.nsp_dim(trans=True)) == (1, 0)
    assert np.array_equal(M.solve_mrhs(B, trans=True), XT0)  # the filter of HIFAMD_S does not touch HIFAMD_SH
    M.set_nsp_basis(d["VL"], trans=True)
    assert (M.nsp_dim(), M.nsp_dim(trans=True)) == (1, 1)
    XT = M.solve_mrhs(B, trans=True)
    assert relerr(XT, _proj(QL, XT0)) <= 1e-12
    assert np.abs(QL.T @ XT).max() <= 1e-12 * np.abs(XT).max()
    assert np.array_equal(M.solve(B[:, 2].copy(), trans=True), XT[:, 2])
    assert relerr(M.nsp_filter(XT0.copy(), trans=True), _proj(QL, XT0)) <= 1e-12
    Xf = M.solve_mrhs(B)  # HIFAMD_S keeps its own filter
    assert relerr(Xf, _proj(Q, X0)) <= 1e-12
    assert relerr(_proj(QL, X0), Xf) > 1e-3  # (the two filters differ: the test above could tell them apart)
    M.set_nsp_basis(None, trans=True)
    assert M.nsp_dim(trans=True) == 0 and np.array_equal(M.solve_mrhs(B, trans=True), XT0)
    assert np.array_equal(M.solve_mrhs(B), Xf)
    # a basis replaces a constant-mode filter on the same op, and the other way round
    M.set_nsp_basis(None)
    M.set_nsp_const(0, -1)
    Xc = M.solve_mrhs(B)
    assert relerr(Xc, X0 - X0.mean(axis=0)) <= 1e-12
    M.set_nsp_basis(d["V"])
    assert M.nsp_dim() == 1 and np.array_equal(M.solve_mrhs(B), Xf)
    M.set_nsp_const(0, -1)
    assert M.nsp_dim() == 0 and np.array_equal(M.solve_mrhs(B), Xc)
    M.set_nsp_const(1, 0)
    assert np.array_equal(M.solve_mrhs(B), X0)


# ---- 6. projected PCG -----------------------------------------------------------------------------------------------
def _bad(v):
    return not (np.isfinite(v) and np.real(v) > 0.0)


def pcg_restated(O, A, B, Q, rtol, maxit):
    """tests/test_gpu_pcg.py pcg_restated on the complement of span(Q): r0 = P b, ||b|| := ||P b||, every z = P M^{-1} r."""
    B = B.reshape(B.shape[0], -1)
    X = np.zeros_like(B)
    flags = np.zeros(B.shape[1], dtype=np.int32)
    iters = np.zeros(B.shape[1], dtype=np.int32)
    for c in range(B.shape[1]):
        r = _proj(Q, B[:, c])
        bn = np.linalg.norm(r)
        if bn == 0.0:
            continue
        x = np.zeros_like(r)
        z = _proj(Q, O.solve(r.copy()))
        p = z.copy()
        rho = np.vdot(r, z)
        flag, it = 1, 0
        if not _bad(rho):
            for k in range(maxit):
                q = A @ p
                sigma = np.vdot(p, q)
                if _bad(sigma):
                    flag, it = 1, k
                    break
                alpha = rho / sigma
                x = x + alpha * p
                r = r - alpha * q
                if np.linalg.norm(r) / bn <= rtol:
                    flag, it = 0, k + 1
                    break
                if k + 1 >= maxit:
                    flag, it = 2, maxit
                    break
                z = _proj(Q, O.solve(r.copy()))
                rho1 = np.vdot(r, z)
                if _bad(rho1):
                    flag, it = 1, k + 1
                    break
                p = z + (rho1 / rho) * p
                rho = rho1
        X[:, c], flags[c], iters[c] = x, flag, it
    return X, flags, iters


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", SYMM)
def test_projected_pcg_vs_restatement(name, rtol):
    levels, d, M, O, A, Q = _fixture(name)
    assert M.is_hermitian()
    M.set_nsp_basis(d["V"])
    n = len(d["b"])
    k = Q.shape[1]
    xs = d["xstar"]
    want = _proj(Q, xs)
    B = np.stack([d["bstar"], d["bstar"] + Q @ np.ones(k), np.zeros(n), d["b"]], axis=1)  # consistent, inconsistent, zero
    X, fl, it = M.pcg(B, rtol=rtol, maxit=300)
    Xo, fo, io = pcg_restated(O, A, B, Q, rtol, 300)
    print(name, rtol, "flags", fl, "iters", it, "restated", fo, io)
    assert fl.tolist() == fo.tolist() and it.tolist() == io.tolist(), (fl, fo, it, io)
    assert fl.tolist() == [0, 0, 0, 0] and it[2] == 0 and not np.any(X[:, 2])
    assert it[0] == it[1] and it[0] > 1  # the inconsistent part of b changes nothing
    PB = _proj(Q, B)
    for c in (0, 1, 3):
        res = np.linalg.norm(A @ X[:, c] - PB[:, c]) / np.linalg.norm(PB[:, c])
        print("  column", c, "vs restatement", relerr(X[:, c], Xo[:, c]), "residual", res, "|Q^H x|/|x|", _qnorm(Q, X[:, c])[0])
        assert relerr(X[:, c], Xo[:, c]) <= 1e-8, c
        assert res <= 10 * rtol, c
        assert _qnorm(Q, X[:, c])[0] <= 1e-12, c
    if rtol == 1e-10:
        for c in (0, 1):
            print("  column", c, "vs x* - Q Q^H x*", relerr(X[:, c], want))
            assert relerr(X[:, c], want) <= 1e-7, c
    # one column through the vector entry
    x, f, i = M.pcg(d["bstar"], rtol=rtol, maxit=300)
    assert np.array_equal(x, X[:, 0]) and (f, i) == (fl[0], it[0])


@pytest.mark.parametrize("name", SYMM)
def test_projected_pcg_bits_do_not_depend_on_the_batch(name):
    import torch

    levels, d, M, O, A, Q = _fixture(name)
    M.set_nsp_basis(d["V"])
    n = len(d["b"])
    B = np.random.default_rng(53).uniform(-1, 1, size=(n, 70))
    B[:, 9] = 0.0
    X70, f70, i70 = M.pcg(B, rtol=1e-9, maxit=300)
    X64, f64, i64 = M.pcg(np.ascontiguousarray(B[:, :64]), rtol=1e-9, maxit=300)
    X5, f5, i5 = M.pcg(np.ascontiguousarray(B[:, :5]), rtol=1e-9, maxit=300)
    assert np.array_equal(X64, X70[:, :64]) and np.array_equal(f64, f70[:64]) and np.array_equal(i64, i70[:64])
    assert np.array_equal(X5, X70[:, :5]) and np.array_equal(f5, f70[:5]) and np.array_equal(i5, i70[:5])
    for c in (0, 3, 9, 63, 64, 69):
        x, f, i = M.pcg(B[:, c].copy(), rtol=1e-9, maxit=300)
        assert np.array_equal(x, X70[:, c]) and (f, i) == (f70[c], i70[c]), c
    assert f70.tolist() == [0] * 70 and i70[9] == 0
    Xd, fd, idv = M.pcg(torch.from_numpy(np.ascontiguousarray(B[:, :5])).cuda(), rtol=1e-9, maxit=300)
    assert np.array_equal(Xd.cpu().numpy(), X5) and np.array_equal(fd, f5) and np.array_equal(idv, i5)
    xd, f, i = M.pcg(torch.from_numpy(B[:, 3].copy()).cuda(), rtol=1e-9, maxit=300)
    assert np.array_equal(xd.cpu().numpy(), X70[:, 3]) and (f, i) == (f70[3], i70[3])


def test_pcg_refusals_with_filters():
    levels, d, M, O, A, Q = _fixture("neu2d_32_symm")
    # a constant-mode filter is still refused, message and code unchanged
    M.set_nsp_const(0, -1)
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.pcg(d["bstar"])
    assert e.value.code == BAD_PREC and "null-space" in e.value.msg and "hifamd_set_nsp_const" in e.value.msg
    M.set_nsp_basis(d["V"])  # replaces it: PCG runs
    x, f, i = M.pcg(d["bstar"], rtol=1e-8, maxit=300)
    assert f == 0
    # a hierarchy that is not Hermitian is still refused with a basis set
    lp, dp, Mp, Op, Ap, Qp = _fixture("pcd2d_32")
    Mp.set_nsp_basis(dp["V"])
    with pytest.raises(hifir_amd.HifAmdError) as e:
        Mp.pcg(dp["bstar"])
    assert e.value.code == BAD_PREC and "Hermitian" in e.value.msg


# ---- 7. BiCGSTAB, GMRES and refinement with the basis ---------------------------------------------------------------
def _bs_bad(v):
    return v == 0 or not np.isfinite(v)


def bicgstab_restated(O, A, B, rtol, maxit, Q=None):
    """tests/test_gpu_bicgstab.py bicgstab_restated with a basis: every M^{-1} apply is followed by v - Q (Q^H v);
    b, r^ and ||b|| are taken as they are."""
    B = B.reshape(B.shape[0], -1)
    X = np.zeros_like(B)
    flags = np.zeros(B.shape[1], dtype=np.int32)
    iters = np.zeros(B.shape[1], dtype=np.int32)

    def prec(u):
        y = O.solve(u.copy())
        return y if Q is None else _proj(Q, y)

    for c in range(B.shape[1]):
        b = B[:, c]
        bn = np.linalg.norm(b)
        if bn == 0.0:
            continue
        x = np.zeros_like(b)
        r = b.copy()
        rh = b.copy()
        rho = np.vdot(rh, r)
        p = r.copy()
        flag, steps = 1, 0
        while not _bs_bad(rho):
            y = prec(p)
            v = A @ y
            steps += 1
            rv = np.vdot(rh, v)
            if _bs_bad(rv):
                break
            alpha = rho / rv
            x = x + alpha * y
            r = r - alpha * v
            if np.linalg.norm(r) / bn <= rtol:
                flag = 0
                break
            if steps >= maxit:
                flag = 2
                break
            y = prec(r)
            t = A @ y
            steps += 1
            tt = np.vdot(t, t)
            if _bs_bad(tt):
                break
            omega = np.vdot(t, r) / tt
            if _bs_bad(omega):
                break
            x = x + omega * y
            r = r - omega * t
            if np.linalg.norm(r) / bn <= rtol:
                flag = 0
                break
            if steps >= maxit:
                flag = 2
                break
            rho1 = np.vdot(rh, r)
            if _bs_bad(rho1):
                break
            beta = (rho1 / rho) * (alpha / omega)
            rho = rho1
            p = r + beta * (p - omega * v)
        X[:, c], flags[c], iters[c] = x, flag, steps
    return X, flags, iters


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", NAMES)
def test_bicgstab_with_basis_vs_restatement(name, rtol):
    levels, d, M, O, A, Q = _fixture(name)
    M.set_nsp_basis(d["V"])
    n = len(d["b"])
    B = np.stack([d["bstar"], np.zeros(n), A @ np.random.default_rng(59).uniform(-1, 1, n)], axis=1)
    X, fl, it = M.bicgstab(B, rtol=rtol, maxit=400)
    Xo, fo, io = bicgstab_restated(O, A, B, rtol, 400, Q)
    print(name, rtol, "flags", fl, "steps", it, "restated", fo, io)
    assert fl.tolist() == fo.tolist() and it.tolist() == io.tolist(), (fl, fo, it, io)
    assert fl.tolist() == [0, 0, 0] and it[1] == 0 and not np.any(X[:, 1])
    for c in (0, 2):
        res = np.linalg.norm(A @ X[:, c] - B[:, c]) / np.linalg.norm(B[:, c])
        print("  column", c, "vs restatement", relerr(X[:, c], Xo[:, c]), "residual", res, "|Q^H x|/|x|", _qnorm(Q, X[:, c])[0])
        assert relerr(X[:, c], Xo[:, c]) <= 1e-8, c
        assert res <= 10 * rtol, c
        assert _qnorm(Q, X[:, c])[0] <= 1e-12, c


@pytest.mark.parametrize("name", NAMES)
def test_bicgstab_with_basis_bits_do_not_depend_on_the_batch(name):
    levels, d, M, O, A, Q = _fixture(name)
    M.set_nsp_basis(d["V"])
    n = len(d["b"])
    B = A @ np.random.default_rng(61).uniform(-1, 1, size=(n, 70))
    X70, f70, i70 = M.bicgstab(B, rtol=1e-9, maxit=400)
    X64, f64, i64 = M.bicgstab(np.ascontiguousarray(B[:, :64]), rtol=1e-9, maxit=400)
    X5, f5, i5 = M.bicgstab(np.ascontiguousarray(B[:, :5]), rtol=1e-9, maxit=400)
    assert np.array_equal(X64, X70[:, :64]) and np.array_equal(f64, f70[:64]) and np.array_equal(i64, i70[:64])
    assert np.array_equal(X5, X70[:, :5]) and np.array_equal(f5, f70[:5]) and np.array_equal(i5, i70[:5])
    for c in (0, 3, 63, 64, 69):
        x, f, i = M.bicgstab(B[:, c].copy(), rtol=1e-9, maxit=400)
        assert np.array_equal(x, X70[:, c]) and (f, i) == (f70[c], i70[c]), c
    assert f70.tolist() == [0] * 70


@pytest.mark.parametrize("name", NAMES)
def test_gmres_with_basis(name):
    levels, d, M, O, A, Q = _fixture(name)
    M.set_nsp_basis(d["V"])
    rtol = 1e-10
    x, flag, it = M.gmres(d["bstar"], restart=30, rtol=rtol, maxit=500)
    res = np.linalg.norm(A @ x - d["bstar"]) / np.linalg.norm(d["bstar"])
    want = _proj(Q, d["xstar"])
    print(name, "gmres flag", flag, "inner steps", it, "residual", res, "|Q^H x|/|x|", _qnorm(Q, x)[0], "vs x* - Q Q^H x*",
          relerr(x, want))
    assert flag == 0
    assert res <= 10 * rtol
    assert _qnorm(Q, x)[0] <= 1e-12
    assert relerr(x, want) <= 1e-7


@pytest.mark.parametrize("name", NAMES)
def test_fixed_sweep_refinement_with_basis(name):
    """hifir with four fixed sweeps: x = 0; four times xk = x, r = b - A xk (the first: b), x = P M^{-1} r + xk."""
    levels, d, M, O, A, Q = _fixture(name)
    M.set_nsp_basis(d["V"])
    n = len(d["b"])
    B = np.stack([d["bstar"], d["b"], np.random.default_rng(67).uniform(-1, 1, n)], axis=1)
    X = M.hifir(B, 4)
    for c in range(B.shape[1]):
        b = B[:, c]
        x = np.zeros(n)
        for i in range(4):
            xk = x
            r = b - A @ xk if i else b.copy()
            x = _proj(Q, O.solve(r.copy())) + xk
        print(name, "hifir column", c, relerr(X[:, c], x))
        assert relerr(X[:, c], x) <= 1e-10, c
    assert np.array_equal(M.hifir(B[:, 1].copy(), 4), X[:, 1])


# ---- 8. 1M rows ---------------------------------------------------------------------------------------------------
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
def test_1m_neumann_projected_pcg_and_bicgstab():
    """The 1000^2 pure-Neumann Laplacian factorized with is_symm by the compiled reference, null space = constants:
    four consistent columns A x* and four uniformly random (inconsistent) ones.  Unfiltered PCG breaks down on the
    latter (flag 1); that run is not repeated here."""
    A = _neumann2d(1000)
    n = A.shape[0]
    R = ref.RefHIF(A.indptr, A.indices, A.data, ref.make_params(is_symm=1))
    M = hifir_amd.HIF.from_levels(R.levels(), max_nrhs=8)
    assert M.is_hermitian()
    M.set_matrix(A.indptr, A.indices, A.data)
    M.set_nsp_basis(np.ones(n))
    Q = np.full((n, 1), 1.0 / np.sqrt(n))
    rng = np.random.default_rng(71)
    B = np.concatenate([A @ rng.uniform(-1, 1, size=(n, 4)), rng.uniform(-1, 1, size=(n, 4))], axis=1)
    PB = _proj(Q, B)
    X, fl, it = M.pcg(B, rtol=1e-8, maxit=1000)
    res = np.linalg.norm(A @ X - PB, axis=0) / np.linalg.norm(PB, axis=0)
    print("1M pcg flags", fl, "iters", it, "residual", res, "|Q^H x|/|x|", _qnorm(Q, X))
    assert fl.tolist() == [0] * 8, (fl, it)
    assert res.max() <= 1e-7, res
    assert _qnorm(Q, X).max() <= 1e-12
    # the same B, made consistent first, through BiCGSTAB with the basis on its applies
    Bf = M.nsp_filter(B.copy())
    assert relerr(Bf, PB) <= 1e-12
    X, fl, it = M.bicgstab(Bf, rtol=1e-8, maxit=1000)
    res = np.linalg.norm(A @ X - PB, axis=0) / np.linalg.norm(PB, axis=0)
    print("1M bicgstab flags", fl, "steps", it, "residual", res, "|Q^H x|/|x|", _qnorm(Q, X))
    assert fl.tolist() == [0] * 8, (fl, it)
    assert res.max() <= 1e-7, res
