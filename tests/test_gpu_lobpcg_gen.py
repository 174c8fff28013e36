"""GPU (-m gpu): the generalized LOBPCG driver (hifamd_lobpcg_gen / HIF.lobpcg_gen, A x = lambda B x with the mass matrix of
set_mass_matrix) against the numpy restatement of the same iteration around the oracle's apply
(lobpcg_gen_util.lobpcg_gen_restated; test_lobpcg_gen_host.py pins every input used here away from its decisions): flags, step
counts, eigenvalues, true backward errors, B-orthonormality and the spanned subspace; B = I given explicitly, which must
reproduce the standard driver bit for bit; diagonal pencils (the kernels' row tails, exact eigenvectors); the entry points
(maxit, the generated start, host arrays and CUDA tensors, strides, repeatability); the other solvers of the handle, whose
bits must not move; the refusals in the header's order; the C++ facade."""
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import hifir_amd
import lobpcg_gen_util as G
import lobpcg_util as U
from idrs_util import generated_P
from util import load_hier

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c[0] for c in G.GEN_CASES]


def _handle(levels, A, B=None, max_nrhs=64):
    M = hifir_amd.HIF.from_levels(levels, max_nrhs=max_nrhs)
    M.set_matrix(A.indptr, A.indices, A.data)
    if B is not None:
        M.set_mass_matrix(B.indptr, B.indices, B.data)
    return M


_HANDLES = {}


def _case_handle(name):
    """one handle per fixture, with the fixture's mass matrix, shared by the tests of this module"""
    Cs, solve, B, X0, k, nev, tol = G.inputs(name)
    if Cs.name not in _HANDLES:
        _HANDLES[Cs.name] = _handle(Cs.levels, Cs.A, B)
    return _HANDLES[Cs.name]


_CHOL = {}


def _chol(fixture, B):
    """lower Cholesky factor of the dense B, once per fixture: B = L L^H turns the pencil into the standard problem
    L^{-1} A L^{-H} y = lambda y, y = L^H x"""
    if fixture not in _CHOL:
        _CHOL[fixture] = np.linalg.cholesky(B.toarray())
    return _CHOL[fixture]


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name):
    (Cs, solve, B, X0, k, nev, tol), (lo, Xo, ro, fo, so, rank_o), tr = G.reference(name)
    M = _case_handle(name)
    assert M.is_hermitian()
    lam, X, res, fl, steps = M.lobpcg_gen(X0=X0, nev=nev, tol=tol, maxit=G.MAXIT)
    true = G.backward_errors(Cs.A, B, lam, X)
    print(name, "steps", steps, so, "info", M.last_lobpcg_info.tolist(), "rank restated", rank_o)
    print("  lam diff / ||A||", np.abs(lam - lo).max() / Cs.anorm, "res", res.max(), "true - res", np.abs(true - res).max())
    assert fl.tolist() == fo.tolist() and steps == so, (fl, fo, steps, so)
    assert M.last_lobpcg_info[0] == so and k <= M.last_lobpcg_info[1] <= 3 * k and 1 <= M.last_lobpcg_info[2] <= 12
    assert np.abs(lam - lo)[:nev].max() <= tol * Cs.anorm
    eig = G.pencil_eigenvalues(Cs.name)
    assert np.abs(lam[:nev] - eig[:nev]).max() <= tol * Cs.anorm
    conv = fl == 0
    assert (true[conv] <= tol + 100 * G.GEN_DRIFT).all() and (np.abs(true - res) <= 100 * G.GEN_DRIFT).all()
    orth = np.linalg.norm(X.conj().T @ (B @ X) - np.eye(k))
    print("  ||X^H B X - I||_F", orth)
    assert orth <= 1e-12
    # the spanned subspace in the B-inner product: with B = L L^H, Y = L^H X has orthonormal columns and is an approximate
    # invariant subspace of C = L^{-1} A L^{-H} with residual L^{-1} (A X - B X Lambda); for Y and the restatement's Yo alike
    # the angle to the invariant subspace of the nev smallest eigenvalues is at most ||residual||_F / gap (Davis-Kahan), gap
    # between the pencil's eigenvalues nev and nev + 1
    L = _chol(Cs.name, B)

    def reduced(lm, Z):
        R = Cs.A @ Z[:, :nev] - (B @ Z[:, :nev]) * lm[None, :nev]
        return np.linalg.norm(scipy.linalg.solve_triangular(L, R, lower=True))

    gap = eig[nev] - eig[nev - 1]
    bound = (reduced(lam, X) + reduced(lo, Xo)) / gap
    angle = U.principal_angle(L.conj().T @ X[:, :nev], L.conj().T @ Xo[:, :nev])
    print("  angle", angle, "bound", bound)
    assert angle <= bound + 1e-12, (angle, bound)


@pytest.mark.parametrize("name", G.BIT_EQUAL)
def test_explicit_identity_reproduces_the_standard_driver_bit_for_bit(name):
    """B = I as a CRS matrix: the SpMM returns its input exactly, BS is a bitwise copy of S, and the three-operand kernels keep
    their models' lane maps and orders of summation -- so through BIT_EQUAL_MAXIT steps, where neither stopping test has a
    converged column to lock (test_lobpcg_gen_host.py), lambda and X are the standard driver's bits.  A swapped operand or a
    changed order of summation shows here."""
    Cs, solve, B, X0, k, nev, tol = G.inputs(name)
    M = _handle(Cs.levels, Cs.A)
    I = sp.identity(Cs.n, format="csr", dtype=Cs.A.dtype)
    M.set_mass_matrix(I.indptr, I.indices, I.data)
    m = G.BIT_EQUAL_MAXIT
    std = M.lobpcg(X0=X0, nev=nev, tol=tol, maxit=m)
    gen = M.lobpcg_gen(X0=X0, nev=nev, tol=tol, maxit=m)
    assert std[4] == gen[4] == m and std[3].tolist() == gen[3].tolist() == [2] * k
    assert np.array_equal(std[0], gen[0]) and np.array_equal(std[1], gen[1])
    assert np.iscomplexobj(gen[1]) == Cs.cplx and np.isfinite(gen[1]).all() and np.abs(gen[1]).max() > 0
    # the residuals differ by the scale alone: ||A|| against (||A|| + |lambda| ||I||) ||x||
    scale = (Cs.anorm + np.abs(gen[0]) * 1.0) * np.linalg.norm(gen[1], axis=0) / Cs.anorm
    assert np.abs(gen[2] * scale - std[2]).max() <= 1e-12 * std[2].max()


@pytest.mark.parametrize("n", [37, 101])
def test_diagonal_pencils_and_exact_eigenvectors(n):
    levels, A, a = U.diagonal_case(n)
    B, b = G.diagonal_mass(n)
    M = _handle(levels, A, B, max_nrhs=16)
    q = a / b
    order = np.argsort(q, kind="stable")
    X0 = np.zeros((n, 3))
    X0[order[:3], [2, 0, 1]] = [2.0, -1.0, 0.5]
    lam, X, res, fl, steps = M.lobpcg_gen(X0=X0, tol=1e-10, maxit=50)
    assert steps == 0 and fl.tolist() == [0, 0, 0] and lam.tolist() == q[order[:3]].tolist() and not res.any()
    want = np.zeros((n, 3))
    want[order[:3], [0, 1, 2]] = 1.0 / np.sqrt(b[order[:3]])  # B-normalized unit vectors: powers of two, exact
    assert np.array_equal(np.abs(X), want)
    # a random block, two wanted of four, against the restatement with M^{-1} = I
    X0 = U.start_block(n, 4, seed=5)
    lo, Xo, ro, fo, so, rank_o = G.lobpcg_gen_restated(lambda r: r, A, B, X0, 2, 1e-9, 400)
    lam, X, res, fl, steps = M.lobpcg_gen(X0=X0, nev=2, tol=1e-9, maxit=400)
    print(n, "steps", steps, so, fl, fo)
    assert so == G.DIAGONAL_STEPS[n] and fl.tolist() == fo.tolist() and steps == so  # (n is no multiple of 16 or 4: the row tails)
    assert fl[:2].tolist() == [0, 0] and np.abs(lam[:2] - q[order[:2]]).max() <= 1e-9 * n
    true = G.backward_errors(A, B, lam, X)
    assert (true[:2] <= 1e-9 + 100 * G.GEN_DRIFT).all() and (np.abs(true - res) <= 100 * G.GEN_DRIFT).all()
    assert np.linalg.norm(X.T @ (B @ X) - np.eye(4)) <= 1e-12


def test_maxit_one_below_and_at_the_restated_count():
    (Cs, solve, B, X0, k, nev, tol), (lo, Xo, ro, fo, so, rank_o), tr = G.reference("p32_k5")
    M = _case_handle("p32_k5")
    lam, X, res, fl, steps = M.lobpcg_gen(X0=X0, tol=tol, maxit=so - 1)
    short = G.lobpcg_gen_restated(solve, Cs.A, B, X0, nev, tol, so - 1)
    assert steps == so - 1 and fl.tolist() == short[3].tolist() and 2 in fl.tolist()
    assert np.linalg.norm(X.T @ (B @ X) - np.eye(k)) <= 1e-12 and np.abs(lam - short[0]).max() <= tol * Cs.anorm
    lam, X, res, fl, steps = M.lobpcg_gen(X0=X0, tol=tol, maxit=so)
    assert steps == so and fl.tolist() == [0] * k


def test_generated_start_tensors_strides_and_repeatability():
    import torch

    (Cs, solve, B, X0, k, nev, tol), ref, tr = G.reference("p32_k5")
    M = _case_handle("p32_k5")
    # the generated start is the generator's numpy restatement
    G0 = generated_P(Cs.n, k, 11, False)
    gen = M.lobpcg_gen(k=k, seed=11, tol=tol, maxit=G.MAXIT)
    giv = M.lobpcg_gen(X0=G0, tol=tol, maxit=G.MAXIT)
    assert gen[3].tolist() == [0] * k and _same(gen[:4], giv[:4]) and gen[4] == giv[4]
    # host arrays and CUDA tensors give the same bits; two calls give the same bits
    first = M.lobpcg_gen(X0=X0, tol=tol, maxit=G.MAXIT)
    again = M.lobpcg_gen(X0=X0, tol=tol, maxit=G.MAXIT)
    dev = M.lobpcg_gen(X0=torch.from_numpy(X0).cuda(), tol=tol, maxit=G.MAXIT)
    assert dev[1].is_cuda and np.array_equal(dev[1].cpu().numpy(), first[1])
    assert _same(first[:4], again[:4]) and _same(first[:4], (dev[0], first[1], dev[2], dev[3]))
    assert first[4] == again[4] == dev[4] == ref[4]
    # strided device blocks through the C entry: X0 at column 2 and X at column 1 of their blocks, the padding untouched
    wide = torch.full((Cs.n, 11), 7.25, dtype=torch.float64, device="cuda")
    wide[:, 2:2 + k] = torch.from_numpy(X0).cuda()
    out = torch.full((Cs.n, 9), -3.5, dtype=torch.float64, device="cuda")
    xv0, xv = wide[:, 2:2 + k], out[:, 1:1 + k]
    lam, res = np.zeros(k), np.zeros(k)
    fl, info = np.full(k, -7, dtype=np.int32), np.full(3, -7, dtype=np.int32)
    st = hifir_amd.lib().hifamd_lobpcg_gen_dev(M._h, k, nev, xv0.data_ptr(), xv0.stride(0), 0, tol, G.DEFTOL, G.MAXIT, 0,
                                               lam.ctypes.data, xv.data_ptr(), xv.stride(0), res.ctypes.data, fl.ctypes.data,
                                               info.ctypes.data)
    torch.cuda.synchronize()
    assert st == 0
    o, w = out.cpu().numpy(), wide.cpu().numpy()
    assert np.array_equal(o[:, 1:1 + k], first[1]) and np.array_equal(lam, first[0]) and np.array_equal(fl, first[3])
    assert np.array_equal(res, first[2])
    assert (o[:, :1] == -3.5).all() and (o[:, 1 + k:] == -3.5).all() and info[0] == first[4]
    assert (w[:, :2] == 7.25).all() and (w[:, 2 + k:] == 7.25).all() and np.array_equal(w[:, 2:2 + k], X0)


def test_nothing_else_on_the_handle_changes():
    """lobpcg, pcg and bcg on one handle: before set_mass_matrix, after it, and after a lobpcg_gen call -- the same bits"""
    Cs, solve, B, X0, k, nev, tol = G.inputs("p32_k5")
    M = _handle(Cs.levels, Cs.A)

    def others():
        return (M.lobpcg(X0=X0, tol=tol, maxit=U.MAXIT), M.pcg(X0[:, :3].copy(), rtol=1e-9, maxit=100),
                M.bcg(X0.copy(), block=k, rtol=1e-9, maxit=100))

    before = others()
    assert before[0][3].tolist() == [0] * k
    M.set_mass_matrix(B.indptr, B.indices, B.data)
    with_b = others()
    gen = M.lobpcg_gen(X0=X0, tol=tol, maxit=G.MAXIT)
    assert gen[3].tolist() == [0] * k and gen[4] == G.reference("p32_k5")[1][4]
    after = others()
    for a, b, c in zip(before, with_b, after):
        assert _same(a, b) and _same(a, c)
    assert _same(gen[:4], M.lobpcg_gen(X0=X0, tol=tol, maxit=G.MAXIT)[:4])
    # a second mass matrix replaces the first: B scaled by 4 gives the eigenvalues over 4, and the same steps (the test is
    # the backward error: it does not depend on how B is scaled; powers of two keep every rounding)
    M.set_mass_matrix(B.indptr, B.indices, 4.0 * B.data)
    g4 = M.lobpcg_gen(X0=X0, tol=tol, maxit=G.MAXIT)
    assert g4[4] == gen[4] and g4[3].tolist() == gen[3].tolist() and np.array_equal(4.0 * g4[0], gen[0])
    assert np.array_equal(2.0 * g4[1], gen[1])


def test_refusals_in_the_order_of_the_header():
    Cs, solve, B, X0, k, nev, tol = G.inputs("p32_k5")
    M = _case_handle("p32_k5")

    def refused(code, word, handle=M, **kw):
        args = dict(X0=X0, tol=tol, maxit=10)
        args.update(kw)
        with pytest.raises(hifir_amd.HifAmdError) as e:
            handle.lobpcg_gen(**args)
        assert e.value.code == code and word in e.value.msg, (kw, e.value.code, e.value.msg)

    refused(2, "1 <= k <= 16", X0=None, k=17)
    refused(2, "1 <= nev <= k", nev=k + 1)
    refused(2, "tol > 0", tol=0.0)
    refused(2, "maxit >= 1", maxit=0)
    refused(2, "0 < deftol < 1", deftol=1.0)
    refused(2, "1 <= nev <= k", nev=0, tol=-1.0, maxit=0)  # the first of several
    lam = np.zeros(k)
    Xo = np.zeros((Cs.n, k))
    st = hifir_amd.lib().hifamd_lobpcg_gen(M._h, k, nev, X0.ctypes.data, k - 1, 0, tol, G.DEFTOL, 10, 0, lam.ctypes.data,
                                           Xo.ctypes.data, k, None, None, None)
    assert st == 2 and b"row stride" in hifir_amd.lib().hifamd_last_error()
    # no matrix; no mass matrix
    M0 = hifir_amd.HIF.from_levels(Cs.levels, max_nrhs=8)
    refused(3, "hifamd_set_matrix", handle=M0)
    M0.set_matrix(Cs.A.indptr, Cs.A.indices, Cs.A.data)
    refused(3, "hifamd_set_mass_matrix", handle=M0)
    refused(2, "1 <= k <= 16", handle=M0, X0=None, k=17)  # (arguments come first)
    # set_mass_matrix refuses what set_matrix refuses, with its codes
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M0.set_mass_matrix(B.indptr[:-1], B.indices, B.data)
    assert e.value.code == 2 and "matrix size differs" in e.value.msg
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M0.set_mass_matrix(B.indptr + 2, B.indices, B.data)
    assert e.value.code == 2 and "0- or 1-based" in e.value.msg
    far = B.indices.copy()
    far[5] = Cs.n
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M0.set_mass_matrix(B.indptr, far, B.data)
    assert e.value.code == 2 and "column index out of range" in e.value.msg
    refused(3, "hifamd_set_mass_matrix", handle=M0)  # (a refused matrix is not installed)
    M0.set_mass_matrix(B.indptr + 1, B.indices + 1, B.data)  # 1-based
    one_based = M0.lobpcg_gen(X0=X0, tol=tol, maxit=G.MAXIT)
    assert _same(one_based[:4], M.lobpcg_gen(X0=X0, tol=tol, maxit=G.MAXIT)[:4])
    # any null-space filter: a basis filter, then a constant-mode one
    M0.set_nsp_basis(np.ones(Cs.n))
    refused(3, "B-orthogonal projector", handle=M0)
    refused(3, "hifamd_set_nsp_basis", handle=M0)
    M0.set_nsp_basis(None)
    M0.set_nsp_const(0, -1)
    refused(3, "B-orthogonal projector", handle=M0)
    refused(3, "hifamd_set_nsp_const", handle=M0)
    M0.set_nsp_const(1, 0)
    assert M0.lobpcg_gen(X0=X0, tol=tol, maxit=G.MAXIT)[4] == one_based[4]
    # not Hermitian: the QRCP last level of p2d_30
    l30, d30 = load_hier("p2d_30")
    M30 = hifir_amd.HIF.from_levels(l30, max_nrhs=8)
    M30.set_matrix(d30["A_indptr"], d30["A_indices"], d30["A_vals"])
    B30 = G.mass2d(30)
    M30.set_mass_matrix(B30.indptr, B30.indices, B30.data)
    refused(3, "is_symm", handle=M30, X0=U.start_block(len(d30["b"]), 3))
    # the start block: B = -mass2d is not positive definite; a NaN; duplicate columns
    M0.set_mass_matrix(B.indptr, B.indices, -B.data)
    refused(3, "not positive definite", handle=M0)
    bad = X0.copy()
    bad[7, 2] = np.nan
    refused(3, "not finite", X0=bad)
    dup = X0.copy()
    dup[:, 3] = dup[:, 1]
    refused(3, "rank deficient", X0=dup)
    refused(3, "not positive definite", X0=dup)  # (the message names both causes)
    # the handles still work
    M0.set_mass_matrix(B.indptr, B.indices, B.data)
    assert M0.lobpcg_gen(X0=X0, tol=tol, maxit=G.MAXIT)[4] == one_based[4]
    assert M.lobpcg_gen(X0=X0, tol=tol, maxit=G.MAXIT)[4] == G.reference("p32_k5")[1][4]


def test_cpp_facade_lobpcg_gen(tmp_path):
    exe = str(tmp_path / "facade_lobpcg_gen_test")
    libdir = os.path.join(ROOT, "hifir_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_lobpcg_gen_test.cpp"), "-L", libdir, "-lhifir_amd",
                           "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FACADE LOBPCG GEN TEST OK" in out.stdout and "FAIL" not in out.stdout
