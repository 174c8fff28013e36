"""GPU (-m gpu): the batched symmetric QMR driver (hifamd_sqmr_batch / HIF.sqmr) on Hermitian indefinite hierarchies against
the numpy restatement of the same recurrence around the oracle's apply (test_sqmr_host.sqmr_restated), where PCG breaks
down; its batch-width independence; a complex Hermitian indefinite hierarchy made from a real one by a diagonal unitary
similarity; its flags and refusals; the projected iteration under a basis null-space filter; and, since this file runs several
solvers on one handle, that the buffers they share carry nothing from one call into the next."""
import numpy as np
import pytest

import hifir_amd
from oracle import orc
from test_sqmr_host import (MAXIT, PROJ_RTOLS, RTOLS, columns, complex_case, fixture, projected_case, sqmr_restated)
from util import load_hier, relerr

pytestmark = pytest.mark.gpu

INDEFINITE = ("shift2d_32_symm", "kktr_24_symm")
_HANDLES = {}


def _handle(name):
    """the fixture's handle with its matrix (made once), next to test_sqmr_host.fixture(name)"""
    if name not in _HANDLES:
        levels, d, O, A = fixture(name)
        M = hifir_amd.HIF.from_levels(levels, max_nrhs=64)
        M.set_matrix(d["A_indptr"], d["A_indices"], d["A_vals"])
        assert M.is_hermitian()
        _HANDLES[name] = M
    return _HANDLES[name]


def _check_vs_restated(X, fl, it, Xo, fo, io, A, B, rtol):
    assert fl.tolist() == fo.tolist() and it.tolist() == io.tolist(), (fl, fo, it, io)
    for c in range(B.shape[1]):
        if not np.any(B[:, c]):
            assert it[c] == 0 and fl[c] == 0 and not np.any(X[:, c])
            continue
        assert relerr(X[:, c], Xo[:, c]) <= 1e-8, c
        if fl[c] == 0:
            assert np.linalg.norm(A @ X[:, c] - B[:, c]) / np.linalg.norm(B[:, c]) <= 10 * rtol


@pytest.mark.parametrize("rtol", RTOLS)
@pytest.mark.parametrize("name", INDEFINITE + ("p2d_32_symm",))
def test_sqmr_vs_restatement(name, rtol):
    levels, d, O, A = fixture(name)
    M = _handle(name)
    B = columns(d, A)
    X, fl, it = M.sqmr(B, rtol=rtol, maxit=MAXIT)
    Xo, fo, io = sqmr_restated(O.solve, A, B, rtol, MAXIT)
    print(name, rtol, "flags", fl, "iters", it, "restated", fo, io)
    _check_vs_restated(X, fl, it, Xo, fo, io, A, B, rtol)
    assert fl.tolist() == [0] * 5 and it[1] == 0 and not np.any(X[:, 1]) and min(it[[0, 2, 3, 4]]) > 1
    # one column through the vector entry
    x, f, i = M.sqmr(d["b"], rtol=rtol, maxit=MAXIT)
    assert np.array_equal(x, X[:, 2]) and (f, i) == (fl[2], it[2])


@pytest.mark.parametrize("name", INDEFINITE)
def test_pcg_breaks_down_and_sqmr_converges(name):
    levels, d, O, A = fixture(name)
    M = _handle(name)
    b = columns(d, A)[:, 0].copy()
    x, f, i = M.pcg(b, rtol=1e-6, maxit=MAXIT)
    assert f == 1, (f, i)
    x, f, i = M.sqmr(b, rtol=1e-6, maxit=MAXIT)
    assert f == 0 and np.linalg.norm(A @ x - b) / np.linalg.norm(b) <= 1e-5


def test_column_bits_do_not_depend_on_the_batch():
    import torch

    M = _handle("shift2d_32_symm")
    n = fixture("shift2d_32_symm")[3].shape[0]
    rng = np.random.default_rng(17)
    B = rng.uniform(-1, 1, size=(n, 70))
    B[:, 9] = 0.0
    X70, f70, i70 = M.sqmr(B, rtol=1e-9, maxit=MAXIT)
    X64, f64, i64 = M.sqmr(np.ascontiguousarray(B[:, :64]), rtol=1e-9, maxit=MAXIT)
    X5, f5, i5 = M.sqmr(np.ascontiguousarray(B[:, :5]), rtol=1e-9, maxit=MAXIT)
    assert np.array_equal(X64, X70[:, :64]) and np.array_equal(f64, f70[:64]) and np.array_equal(i64, i70[:64])
    assert np.array_equal(X5, X70[:, :5]) and np.array_equal(f5, f70[:5]) and np.array_equal(i5, i70[:5])
    for k in (0, 3, 9, 63, 64, 69):
        x, f, i = M.sqmr(B[:, k].copy(), rtol=1e-9, maxit=MAXIT)
        assert np.array_equal(x, X70[:, k]) and (f, i) == (f70[k], i70[k]), k
    assert f70.tolist() == [0] * 70 and i70[9] == 0 and not np.any(X70[:, 9])
    # the torch-device entry gives the host entry's bits, for a block and for a vector
    Xd, fd, idv = M.sqmr(torch.from_numpy(np.ascontiguousarray(B[:, :5])).cuda(), rtol=1e-9, maxit=MAXIT)
    assert np.array_equal(Xd.cpu().numpy(), X5) and np.array_equal(fd, f5) and np.array_equal(idv, i5)
    xd, f, i = M.sqmr(torch.from_numpy(B[:, 3].copy()).cuda(), rtol=1e-9, maxit=MAXIT)
    assert np.array_equal(xd.cpu().numpy(), X70[:, 3]) and (f, i) == (f70[3], i70[3])
    # a second call gives the same bits
    Xa, fa, ia = M.sqmr(B, rtol=1e-9, maxit=MAXIT)
    assert np.array_equal(Xa, X70) and np.array_equal(fa, f70) and np.array_equal(ia, i70)


def test_complex_hermitian_indefinite_hierarchy():
    M = _handle("shift2d_32_symm")
    lz, Az, phi, B, Bz = complex_case()
    Mz = hifir_amd.HIF.from_levels(lz, max_nrhs=8)
    assert Mz.is_hermitian()
    Mz.set_matrix(Az.indptr, Az.indices, Az.data)
    X, fl, it = M.sqmr(B, rtol=1e-10, maxit=MAXIT)
    Xz, flz, itz = Mz.sqmr(phi[:, None] * B, rtol=1e-10, maxit=MAXIT)
    assert flz.tolist() == fl.tolist() == [0, 0] and itz.tolist() == it.tolist()
    for c in range(2):
        assert np.linalg.norm(Xz[:, c] - phi * X[:, c]) / np.linalg.norm(X[:, c]) <= 1e-10
    # a genuinely complex b (and a zero column) against the restatement
    Xz, flz, itz = Mz.sqmr(Bz, rtol=1e-10, maxit=MAXIT)
    Xo, fo, io = sqmr_restated(orc.Oracle(lz).solve, Az, Bz, 1e-10, MAXIT)
    _check_vs_restated(Xz, flz, itz, Xo, fo, io, Az, Bz, 1e-10)
    assert flz.tolist() == [0, 0, 0]


def _mixed_batch(n, ncol, seed, cplx=False):
    """seeded uniform columns; the 70-wide ones hold a zero column and one scaled by 1e-8, so columns freeze at different steps"""
    rng = np.random.default_rng(seed)
    B = rng.uniform(-1, 1, size=(n, ncol))
    if cplx:
        B = B + 1j * rng.uniform(-1, 1, size=(n, ncol))
    if ncol == 70:
        B[:, 9] = 0.0
        B[:, 66] *= 1e-8
    return B


def _solvers_share_nothing(make, n, calls, cplx=False):
    """every call of the sequence on ONE handle gives the bits of the same call on a fresh handle that ran nothing else"""
    M = make()
    for k, (solver, ncol, kw) in enumerate(calls):
        B = _mixed_batch(n, ncol, 100 + k, cplx)
        b = B[:, 0].copy() if ncol == 1 else B
        X, fl, it = getattr(M, solver)(b, **kw)
        Xf, ff, itf = getattr(make(), solver)(b, **kw)
        print(k, solver, ncol, "flags", np.unique(fl), "iters", np.min(it), np.max(it))
        assert np.array_equal(X, Xf) and np.array_equal(fl, ff) and np.array_equal(it, itf), (k, solver, ncol)


def test_solvers_on_one_handle_leave_nothing_behind():
    """PCG, BiCGSTAB, symmetric QMR and GMRES share the work vectors, the state block and the pinned read-back buffer of a
    handle: no scalar, active mask or vector of one call (another solver, another width, another sizeof) reaches the next"""
    levels, d, O, A = fixture("p2d_32_symm")

    def make():
        M = hifir_amd.HIF.from_levels(levels, max_nrhs=64)
        M.set_matrix(d["A_indptr"], d["A_indices"], d["A_vals"])
        return M

    kw = dict(rtol=1e-8, maxit=MAXIT)
    _solvers_share_nothing(make, A.shape[0], [("sqmr", 70, kw), ("pcg", 5, kw), ("bicgstab", 64, kw),
                                              ("gmres", 3, dict(restart=5, rtol=1e-8, maxit=MAXIT)), ("pcg", 70, kw),
                                              ("sqmr", 1, kw)])
    lz, Az = complex_case()[:2]

    def make_z():
        Mz = hifir_amd.HIF.from_levels(lz, max_nrhs=64)
        Mz.set_matrix(Az.indptr, Az.indices, Az.data)
        return Mz

    _solvers_share_nothing(make_z, Az.shape[0], [("sqmr", 70, kw), ("bicgstab", 5, kw), ("sqmr", 64, kw)], cplx=True)


def test_flags_and_refusals():
    levels, d, O, A = fixture("shift2d_32_symm")
    M = _handle("shift2d_32_symm")
    b = d["b"]
    n = len(b)
    # maxit reached
    x, flag, it = M.sqmr(b, rtol=1e-14, maxit=3)
    xo, fo, io = sqmr_restated(O.solve, A, b, 1e-14, 3)
    assert (flag, it) == (2, 3) == (int(fo[0]), int(io[0])) and relerr(x, xo[:, 0]) <= 1e-8
    # the same pattern with all values zero: sigma = p^H A p is exactly zero at the first iteration
    Mn = hifir_amd.HIF.from_levels(levels, max_nrhs=4)
    Mn.set_matrix(d["A_indptr"], d["A_indices"], np.zeros_like(d["A_vals"]))
    X, fl, it = Mn.sqmr(np.stack([b, np.zeros_like(b)], axis=1), rtol=1e-8, maxit=50)
    assert fl.tolist() == [1, 0] and it.tolist() == [0, 0] and not np.any(X)
    # a column holding a NaN breaks down at the start and leaves its neighbour's bits alone
    rng = np.random.default_rng(31)
    good = rng.uniform(-1, 1, n)
    bad = rng.uniform(-1, 1, n)
    bad[n // 2] = np.nan
    X, fl, it = M.sqmr(np.stack([bad, good], axis=1), rtol=1e-8, maxit=MAXIT)
    x, f, i = M.sqmr(good.copy(), rtol=1e-8, maxit=MAXIT)
    assert fl.tolist() == [1, 0] and it[0] == 0 and (f, i) == (0, it[1])
    assert np.array_equal(X[:, 1], x)
    # arguments
    for kw in ({"rtol": 0.0}, {"rtol": -1.0}, {"maxit": 0}):
        with pytest.raises(hifir_amd.HifAmdError) as e:
            M.sqmr(b, **kw)
        assert e.value.code == 2
    # no matrix
    M0 = hifir_amd.HIF.from_levels(levels, max_nrhs=4)
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M0.sqmr(b)
    assert e.value.code == 3 and "hifamd_set_matrix" in e.value.msg
    # a constant-mode null-space filter on the solve is refused
    M0.set_matrix(d["A_indptr"], d["A_indices"], d["A_vals"])
    M0.set_nsp_const(0, -1)
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M0.sqmr(b)
    assert e.value.code == 3 and "null-space" in e.value.msg
    # not Hermitian: the QRCP last level of p2d_30 (its sparse level is mirrored bit for bit)
    l30, d30 = load_hier("p2d_30")
    M30 = hifir_amd.HIF.from_levels(l30, max_nrhs=4)
    M30.set_matrix(d30["A_indptr"], d30["A_indices"], d30["A_vals"])
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M30.sqmr(d30["b"])
    msg = e.value.msg
    assert e.value.code == 3 and "level 1" in msg and "dense" in msg and "is_symm" in msg
    assert "GMRES" in msg and "BiCGSTAB" in msg


@pytest.mark.parametrize("rtol", PROJ_RTOLS)
def test_projected_sqmr_vs_restatement(rtol):
    levels, d, A, Q, solve, PB = projected_case()
    M = hifir_amd.HIF.from_levels(levels, max_nrhs=4)
    M.set_matrix(d["A_indptr"], d["A_indices"], d["A_vals"])
    M.set_nsp_basis(d["V"])
    B = np.stack([d["bstar"], d["b"], np.zeros(len(d["b"]))], axis=1)
    X, fl, it = M.sqmr(B, rtol=rtol, maxit=MAXIT)
    Xo, fo, io = sqmr_restated(solve, A, PB, rtol, MAXIT)
    print(rtol, "flags", fl, "iters", it, "restated", fo, io)
    assert fl.tolist() == fo.tolist() + [0] and it.tolist() == io.tolist() + [0] and not np.any(X[:, 2])
    assert fl.tolist() == [0, 0, 0] and min(it[:2]) > 1
    for c in range(2):
        res = np.linalg.norm(A @ X[:, c] - PB[:, c]) / np.linalg.norm(PB[:, c])
        qx = np.abs(Q.conj().T @ X[:, c]).max() / np.linalg.norm(X[:, c])
        print("  column", c, "vs restatement", relerr(X[:, c], Xo[:, c]), "residual", res, "max|Q^H x|/|x|", qx)
        assert relerr(X[:, c], Xo[:, c]) <= 1e-8, c
        assert res <= 10 * rtol, c
        assert qx <= 1e-10, c
