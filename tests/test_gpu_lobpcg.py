"""GPU (-m gpu): the LOBPCG driver (hifamd_lobpcg / HIF.lobpcg) against the numpy restatement of the same iteration around
the oracle's apply (lobpcg_util.lobpcg_restated; test_lobpcg_host.py pins every input used here away from its decisions):
flags, step counts, eigenvalues, true residuals, orthonormality and the spanned subspace; the edges (a diagonal hierarchy,
exact eigenvectors, maxit, the generated start, host arrays and CUDA tensors, strides, repeatability,
other solvers on the same handle); the refusals in the header's order; the basis filter; the C++ facade."""
import os
import subprocess

import numpy as np
import pytest

import hifir_amd
import lobpcg_util as U
from idrs_util import generated_P
from util import load_hier

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON_DEVICE = [c[0] for c in U.CASES if c[0] not in U.REFUSED_ON_DEVICE]


def _handle(levels, A, max_nrhs=64):
    M = hifir_amd.HIF.from_levels(levels, max_nrhs=max_nrhs)
    M.set_matrix(A.indptr, A.indices, A.data)
    return M


_HANDLES = {}


def _case_handle(name):
    """one handle per (fixture, basis installed), shared by the tests of this module"""
    Cs, solve, X0, k, nev, tol, Q = U.inputs(name)
    key = (Cs.name, Q is not None)
    if key not in _HANDLES:
        M = _handle(Cs.levels, Cs.A)
        if Q is not None:
            M.set_nsp_basis(Cs.d["V"])
        _HANDLES[key] = M
    return _HANDLES[key]


def _true_residuals(A, anorm, lam, X):
    return np.linalg.norm(A @ X - X * lam[None, :], axis=0) / anorm


@pytest.mark.parametrize("name", ON_DEVICE)
def test_against_the_restatement(name):
    (Cs, solve, X0, k, nev, tol, Q), (lo, Xo, ro, fo, so, rank_o), tr = U.reference(name)
    M = _case_handle(name)
    assert M.is_hermitian()
    lam, X, res, fl, steps = M.lobpcg(X0=X0, nev=nev, tol=tol, maxit=U.MAXIT)
    true = _true_residuals(Cs.A, Cs.anorm, lam, X)
    print(name, "steps", steps, so, "info", M.last_lobpcg_info.tolist(), "rank restated", rank_o)
    print("  lam diff / ||A||", np.abs(lam - lo).max() / Cs.anorm, "res", res.max(), "true - res", np.abs(true - res).max())
    assert fl.tolist() == fo.tolist() and steps == so, (fl, fo, steps, so)
    assert M.last_lobpcg_info[0] == so and k <= M.last_lobpcg_info[1] <= 3 * k and 1 <= M.last_lobpcg_info[2] <= 12
    assert np.abs(lam - lo)[:nev].max() <= tol * Cs.anorm
    eig = Cs.eig if Q is None else Cs.eig[Q.shape[1]:]
    assert np.abs(lam[:nev] - eig[:nev]).max() <= tol * Cs.anorm
    conv = fl == 0
    assert (true[conv] <= tol + 100 * U.DRIFT).all() and (np.abs(true - res) <= 100 * U.DRIFT).all()
    assert np.linalg.norm(X.conj().T @ X - np.eye(k)) <= 1e-12
    # the spanned subspace: for X and the restatement's Xo alike the angle to the invariant subspace of the nev smallest
    # eigenvalues is at most ||R|| / gap (Davis-Kahan), gap from eigvalsh between eigenvalue nev and nev + 1
    gap = (eig[nev] - eig[nev - 1]) / Cs.anorm
    bound = (np.linalg.norm(true[:nev]) + np.linalg.norm(ro[:nev])) / gap
    angle = U.principal_angle(X[:, :nev], Xo[:, :nev])
    print("  angle", angle, "bound", bound)
    assert angle <= bound + 1e-12, (angle, bound)


@pytest.mark.parametrize("fixture,k,tol,seed,want", U.FULL_BLOCKS)
def test_full_blocks_without_guard_columns(fixture, k, tol, seed, want):
    """nev = k = 15 and 16 on p2d_32_symm: held to everything, and to the restated step count within FULL_SPREAD = 2 -- inside
    a double eigenvalue the device's Jacobi method and LAPACK rotate the Ritz vectors differently, and the count follows
    (lobpcg_util.CASES says why).  Measured here: 21 against 20 steps at k = 15, 19 against 19 at k = 16."""
    Cs = U.case(fixture)
    X0 = U.start_block(Cs.n, k, seed=seed)
    lo, Xo, ro, fo, so, rank_o = U.lobpcg_restated(Cs.O, Cs.A, X0, k, tol, U.MAXIT)
    lam, X, res, fl, steps = _case_handle("p32_k16").lobpcg(X0=X0, tol=tol, maxit=U.MAXIT)
    true = _true_residuals(Cs.A, Cs.anorm, lam, X)
    print(k, "steps", steps, so, "info", _case_handle("p32_k16").last_lobpcg_info.tolist())
    assert fl.tolist() == fo.tolist() == [0] * k and so == want and abs(steps - so) <= U.FULL_SPREAD
    assert np.abs(lam - Cs.eig[:k]).max() <= tol * Cs.anorm and (true <= tol + 100 * U.DRIFT).all()
    assert np.linalg.norm(X.T @ X - np.eye(k)) <= 1e-12
    gap = (Cs.eig[k] - Cs.eig[k - 1]) / Cs.anorm
    assert U.principal_angle(X, Xo) <= (np.linalg.norm(true) + np.linalg.norm(ro)) / gap + 1e-12


@pytest.mark.parametrize("name", U.REFUSED_ON_DEVICE)
def test_complex_symmetric_fixture_is_refused_as_pcg_refuses_it(name):
    """herm_24_symm couples its levels with F = E^T, not E^H: its M^{-1} is not Hermitian, the Hermitian check that LOBPCG
    shares with PCG refuses it, and the restatement alone covers it (test_lobpcg_host.py); p32z_k5 is the complex pair here"""
    Cs, solve, X0, k, nev, tol, Q = U.inputs(name)
    M = _handle(Cs.levels, Cs.A)
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.lobpcg(X0=X0, nev=nev, tol=tol)
    assert e.value.code == 3 and "LOBPCG needs a Hermitian preconditioner" in e.value.msg and "F != E^H" in e.value.msg


@pytest.mark.parametrize("n", [37, 101])
def test_diagonal_hierarchy_and_exact_eigenvectors(n):
    levels, A, a = U.diagonal_case(n)
    M = _handle(levels, A, max_nrhs=16)
    order = np.argsort(a)
    X0 = np.zeros((n, 3))
    X0[order[:3], [2, 0, 1]] = [2.0, -1.0, 0.5]
    lam, X, res, fl, steps = M.lobpcg(X0=X0, tol=1e-10, maxit=50)
    assert steps == 0 and fl.tolist() == [0, 0, 0] and lam.tolist() == [1.0, 2.0, 3.0] and not res.any()
    assert np.array_equal(np.abs(X), np.eye(n)[:, order[:3]])
    # a random block, two wanted of four, against the restatement with M^{-1} = I
    X0 = U.start_block(n, 4, seed=5)
    lo, Xo, ro, fo, so, rank_o = U.lobpcg_restated(lambda r: r, A, X0, 2, 1e-9, 400)
    lam, X, res, fl, steps = M.lobpcg(X0=X0, nev=2, tol=1e-9, maxit=400)
    print(n, "steps", steps, so, fl, fo)
    assert fl.tolist() == fo.tolist() and steps == so  # (n is no multiple of 16 or 4: the kernels' row tails)
    assert fl[:2].tolist() == [0, 0] and np.abs(lam[:2] - [1.0, 2.0]).max() <= 1e-9 * n
    assert (_true_residuals(A, float(n), lam, X)[:2] <= 1e-9 + 100 * U.DRIFT).all()
    assert np.linalg.norm(X.T @ X - np.eye(4)) <= 1e-12


def test_maxit_one_below_and_at_the_restated_count():
    (Cs, solve, X0, k, nev, tol, Q), (lo, Xo, ro, fo, so, rank_o), tr = U.reference("p32_k5")
    M = _case_handle("p32_k5")
    lam, X, res, fl, steps = M.lobpcg(X0=X0, tol=tol, maxit=so - 1)
    short = U.lobpcg_restated(solve, Cs.A, X0, nev, tol, so - 1)
    assert steps == so - 1 and fl.tolist() == short[3].tolist() and 2 in fl.tolist()
    assert np.linalg.norm(X.T @ X - np.eye(k)) <= 1e-12 and np.abs(lam - short[0]).max() <= tol * Cs.anorm
    lam, X, res, fl, steps = M.lobpcg(X0=X0, tol=tol, maxit=so)
    assert steps == so and fl.tolist() == [0] * k


def test_generated_start_tensors_strides_and_repeatability():
    import torch

    (Cs, solve, X0, k, nev, tol, Q), ref, tr = U.reference("p32_k5")
    M = _case_handle("p32_k5")
    # the generated start is the generator's numpy restatement
    G0 = generated_P(Cs.n, k, 11, False)
    gen = M.lobpcg(k=k, seed=11, tol=tol, maxit=U.MAXIT)
    giv = M.lobpcg(X0=G0, tol=tol, maxit=U.MAXIT)
    assert gen[3].tolist() == [0] * k and all(np.array_equal(a, b) for a, b in zip(gen[:4], giv[:4])) and gen[4] == giv[4]
    # host arrays and CUDA tensors give the same bits; two calls give the same bits
    first = M.lobpcg(X0=X0, tol=tol, maxit=U.MAXIT)
    pcg0 = M.pcg(X0[:, :3].copy(), rtol=1e-9, maxit=100)
    bcg0 = M.bcg(X0.copy(), block=k, rtol=1e-9, maxit=100)
    again = M.lobpcg(X0=X0, tol=tol, maxit=U.MAXIT)
    dev = M.lobpcg(X0=torch.from_numpy(X0).cuda(), tol=tol, maxit=U.MAXIT)
    assert dev[1].is_cuda and np.array_equal(dev[1].cpu().numpy(), first[1])
    for a, b, c in zip(first[:4], again[:4], (dev[0], first[1], dev[2], dev[3])):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert first[4] == again[4] == dev[4] == ref[4]
    # a PCG and a block-CG call on the same handle before and after give unchanged bits of theirs
    pcg1 = M.pcg(X0[:, :3].copy(), rtol=1e-9, maxit=100)
    bcg1 = M.bcg(X0.copy(), block=k, rtol=1e-9, maxit=100)
    assert all(np.array_equal(a, b) for a, b in zip(pcg0, pcg1)) and all(np.array_equal(a, b) for a, b in zip(bcg0, bcg1))
    # strided device blocks through the C entry: X0 at column 2 and X at column 1 of their blocks, the padding untouched
    wide = torch.full((Cs.n, 11), 7.25, dtype=torch.float64, device="cuda")
    wide[:, 2:2 + k] = torch.from_numpy(X0).cuda()
    out = torch.full((Cs.n, 9), -3.5, dtype=torch.float64, device="cuda")
    xv0, xv = wide[:, 2:2 + k], out[:, 1:1 + k]
    lam, res = np.zeros(k), np.zeros(k)
    fl, info = np.full(k, -7, dtype=np.int32), np.full(3, -7, dtype=np.int32)
    st = hifir_amd.lib().hifamd_lobpcg_dev(M._h, k, nev, xv0.data_ptr(), xv0.stride(0), 0, tol, U.DEFTOL, U.MAXIT, 0,
                                           lam.ctypes.data, xv.data_ptr(), xv.stride(0), res.ctypes.data, fl.ctypes.data,
                                           info.ctypes.data)
    torch.cuda.synchronize()
    assert st == 0
    o, w = out.cpu().numpy(), wide.cpu().numpy()
    assert np.array_equal(o[:, 1:1 + k], first[1]) and np.array_equal(lam, first[0]) and np.array_equal(fl, first[3])
    assert (o[:, :1] == -3.5).all() and (o[:, 1 + k:] == -3.5).all() and info[0] == first[4]
    assert (w[:, :2] == 7.25).all() and (w[:, 2 + k:] == 7.25).all() and np.array_equal(w[:, 2:2 + k], X0)


def test_refusals_in_the_order_of_the_header():
    Cs, solve, X0, k, nev, tol, Q = U.inputs("p32_k5")
    M = _case_handle("p32_k5")

    def refused(code, word, handle=M, **kw):
        args = dict(X0=X0, tol=tol, maxit=10)
        args.update(kw)
        with pytest.raises(hifir_amd.HifAmdError) as e:
            handle.lobpcg(**args)
        assert e.value.code == code and word in e.value.msg, (kw, e.value.code, e.value.msg)

    refused(2, "1 <= k <= 16", X0=None, k=17)
    refused(2, "1 <= k <= 16", X0=None, k=0)
    refused(2, "1 <= nev <= k", nev=k + 1)
    refused(2, "1 <= nev <= k", nev=0)
    refused(2, "tol > 0", tol=0.0)
    refused(2, "maxit >= 1", maxit=0)
    refused(2, "0 < deftol < 1", deftol=1.0)
    refused(2, "1 <= k <= 16", X0=None, k=17, nev=18, tol=-1.0)  # the first of several
    refused(2, "1 <= nev <= k", nev=0, tol=-1.0, maxit=0)
    lam = np.zeros(k)
    Xo = np.zeros((Cs.n, k))
    st = hifir_amd.lib().hifamd_lobpcg(M._h, k, nev, X0.ctypes.data, k - 1, 0, tol, U.DEFTOL, 10, 0, lam.ctypes.data,
                                       Xo.ctypes.data, k, None, None, None)
    assert st == 2 and b"row stride" in hifir_amd.lib().hifamd_last_error()
    assert hifir_amd.lib().hifamd_lobpcg(None, k, nev, None, 0, 0, tol, U.DEFTOL, 10, 0, None, Xo.ctypes.data, k, None, None,
                                         None) == 1
    # no matrix; then a constant-mode filter
    M0 = hifir_amd.HIF.from_levels(Cs.levels, max_nrhs=8)
    refused(3, "hifamd_set_matrix", handle=M0)
    refused(2, "1 <= k <= 16", handle=M0, X0=None, k=17)  # (arguments come first)
    M0.set_matrix(Cs.A.indptr, Cs.A.indices, Cs.A.data)
    M0.set_nsp_const(0, -1)
    refused(3, "constant-mode null-space filter", handle=M0)
    # not Hermitian: the QRCP last level of p2d_30
    l30, d30 = load_hier("p2d_30")
    M30 = hifir_amd.HIF.from_levels(l30, max_nrhs=8)
    M30.set_matrix(d30["A_indptr"], d30["A_indices"], d30["A_vals"])
    refused(3, "is_symm", handle=M30, X0=U.start_block(len(d30["b"]), 3))
    # the start block: duplicate columns, a NaN
    dup = X0.copy()
    dup[:, 3] = dup[:, 1]
    refused(3, "rank deficient", X0=dup)
    bad = X0.copy()
    bad[7, 2] = np.nan
    refused(3, "not finite", X0=bad)
    # the handle still works
    assert M.lobpcg(X0=X0, tol=tol, maxit=U.MAXIT)[4] == U.reference("p32_k5")[1][4]


def test_basis_filter_returns_the_smallest_nonzero_eigenvalues():
    (Cs, solve, X0, k, nev, tol, Q), ref, tr = U.reference("neu_k5_basis")
    plain = _case_handle("neu_k5").lobpcg(X0=X0, tol=tol, maxit=U.MAXIT)
    assert plain[3].tolist() == [0] * k and abs(plain[0][0]) <= tol * Cs.anorm
    lam, X, res, fl, steps = _case_handle("neu_k5_basis").lobpcg(X0=X0, tol=tol, maxit=U.MAXIT)
    assert fl.tolist() == [0] * k and abs(lam[0] - Cs.eig[1]) <= tol * Cs.anorm and abs(lam[0] - 9.6305e-3) <= 5e-8
    assert np.linalg.norm(Q.conj().T @ X) <= 1e-12


def test_cpp_facade_lobpcg(tmp_path):
    exe = str(tmp_path / "facade_lobpcg_test")
    libdir = os.path.join(ROOT, "hifir_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_lobpcg_test.cpp"), "-L", libdir, "-lhifir_amd",
                           "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FACADE LOBPCG TEST OK" in out.stdout and "FAIL" not in out.stdout
