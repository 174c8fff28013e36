"""GPU (-m gpu): the breakdown-free block CG driver (hifamd_bcg_batch / HIF.bcg) against the numpy restatement of the same
recurrence around the oracle's apply (blockcg_util.bcg_restated; test_blockcg_host.py pins every input used here away from
its decisions): block widths and tile cuts, deflation at the start and inside the loop, excluded columns, flags and
refusals, repeatability, a complex Hermitian pair, the projected iteration and the C++ facade."""
import os
import subprocess

import numpy as np
import pytest

import blockcg_util as U
import hifir_amd
from krylov_edges_util import neighbours_replaced
from util import load_hier, relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, MAXIT = U.RTOL, U.MAXIT


def _handle(levels, A, max_nrhs=64):
    M = hifir_amd.HIF.from_levels(levels, max_nrhs=max_nrhs)
    M.set_matrix(A.indptr, A.indices, A.data)
    assert M.is_hermitian()
    return M


@pytest.fixture(scope="module")
def p32():
    P = U.p32()
    return P, _handle(P.levels, P.A)


def _hold(out, ref, A, B, rtol):
    """flags, iterations and ranks equal; x within 1e-8 of the restatement's per column; true residual of a converged column"""
    (X, fl, it, rk), (Xo, fo, io, ro) = out, ref
    assert fl.tolist() == fo.tolist() and it.tolist() == io.tolist() and rk.tolist() == ro.tolist(), (fl, fo, it, io, rk, ro)
    with np.errstate(all="ignore"):
        b2 = np.array([np.vdot(B[:, c], B[:, c]).real for c in range(B.shape[1])])
    for c in range(B.shape[1]):
        if b2[c] == 0.0 or not np.isfinite(b2[c]):
            assert it[c] == 0 and not np.any(X[:, c]), c
            continue
        assert relerr(X[:, c], Xo[:, c]) <= 1e-8, (c, relerr(X[:, c], Xo[:, c]))
        if fl[c] == 0:
            assert np.linalg.norm(A @ X[:, c] - B[:, c]) / np.sqrt(b2[c]) <= 10 * rtol, c


@pytest.mark.parametrize("width", U.WIDTHS)
def test_block_widths(p32, width):
    P, M = p32
    (solve, A, B, block, rtol, maxit), ref = U.reference("width%d" % width)
    out = M.bcg(B, block=width, rtol=RTOL, maxit=MAXIT)
    _hold(out, ref, P.A, B, RTOL)
    assert out[1].tolist() == [0] * width and out[3].tolist() == [width, width]


@pytest.mark.parametrize("nrhs,block", U.CUTS)
def test_tile_cuts(p32, nrhs, block):
    P, M = p32
    B, ref = U.reference("cut%d_%d" % (nrhs, block))[0][2], U.reference("cut%d_%d" % (nrhs, block))[1]
    out = M.bcg(B, block=block, rtol=RTOL, maxit=MAXIT)
    _hold(out, ref, P.A, B, RTOL)
    last = nrhs - (nrhs - 1) // block * block
    assert out[1].tolist() == [0] * nrhs and out[3].tolist()[-2:] == [last, last] and len(out[3]) == 2 * (-(-nrhs // block))
    # the tiles are independent of each other: the last one alone gives the same bits
    alone = M.bcg(np.ascontiguousarray(B[:, nrhs - last:]), block=block, rtol=RTOL, maxit=MAXIT)
    assert np.array_equal(alone[0], out[0][:, nrhs - last:]) and np.array_equal(alone[2], out[2][nrhs - last:])


def test_deflation_at_the_start(p32):
    P, M = p32
    B, ref = U.reference("deflation")[0][2], U.reference("deflation")[1]
    out = M.bcg(B, block=8, rtol=RTOL, maxit=MAXIT)
    _hold(out, ref, P.A, B, RTOL)
    assert out[1].tolist() == [0] * 8 and out[3].tolist() == [5, 5] and out[2][4] == 0


def test_rank_loss_inside_the_loop():
    levels, A, B = U.rank_loss_case()
    M = _handle(levels, A, max_nrhs=8)
    out = M.bcg(B, block=5, rtol=RTOL, maxit=MAXIT)
    _hold(out, U.reference("rank_loss")[1], A, B, RTOL)
    assert out[1].tolist() == [0] * 5 and out[3].tolist() == [5, 3]


def test_fewer_rows_than_columns():
    levels, A, B = U.tiny_case()
    M = _handle(levels, A, max_nrhs=8)
    out = M.bcg(B, block=5, rtol=RTOL, maxit=MAXIT)
    _hold(out, U.reference("tiny")[1], A, B, RTOL)
    assert out[1].tolist() == [0] * 5 and out[3].tolist() == [3, 3]


@pytest.mark.parametrize("how", ["nan", "inf", "big"])
def test_excluded_columns_do_not_touch_their_neighbour(p32, how):
    P, M = p32
    B = U.columns(P.A.shape[0], 5)
    keep = 2
    X0, f0, i0, r0 = M.bcg(neighbours_replaced(B, keep, "zero"), block=5, rtol=RTOL, maxit=MAXIT)
    X, fl, it, rk = M.bcg(neighbours_replaced(B, keep, how), block=5, rtol=RTOL, maxit=MAXIT)
    assert np.array_equal(X[:, keep], X0[:, keep]) and (fl[keep], it[keep]) == (f0[keep], i0[keep]) == (0, i0[keep])
    others = np.arange(5) != keep
    assert (fl[others] == 1).all() and not it[others].any() and not X[:, others].any()
    assert not f0[others].any() and not i0[others].any() and rk.tolist() == r0.tolist() == [1, 1]
    _hold((X0, f0, i0, r0), U.reference("excluded")[1], P.A, neighbours_replaced(B, keep, "zero"), RTOL)


def test_flags_and_refusals(p32):
    P, M = p32
    n = P.A.shape[0]
    B = U.columns(n, 16)
    # maxit reached
    out = M.bcg(B, block=16, rtol=RTOL, maxit=3)
    _hold(out, U.reference("maxit3")[1], P.A, B, RTOL)
    assert out[1].tolist() == [2] * 16 and out[2].tolist() == [3] * 16
    # (-A, M): P^H A P is negative definite, breakdown at the first step's Cholesky
    Mn = hifir_amd.HIF.from_levels(P.levels, max_nrhs=4)
    Mn.set_matrix(P.A.indptr, P.A.indices, -P.A.data)
    Bn = np.stack([B[:, 0], np.zeros(n), B[:, 1]], axis=1)
    X, fl, it, rk = Mn.bcg(Bn, block=3, rtol=RTOL, maxit=50)
    assert fl.tolist() == [1, 0, 1] and it.tolist() == [0, 0, 0]
    fo, io = U.bcg_restated(P.apply, -P.A, Bn, 3, RTOL, 50)[1:3]
    assert fo.tolist() == fl.tolist() and io.tolist() == it.tolist()
    # arguments
    for kw in ({"rtol": 0.0}, {"rtol": -1.0}, {"maxit": 0}, {"block": 0}, {"block": 65}, {"deftol": 0.0}, {"deftol": 1.0}):
        with pytest.raises(hifir_amd.HifAmdError) as e:
            M.bcg(B, **kw)
        assert e.value.code == 2, kw
    # no matrix
    M0 = hifir_amd.HIF.from_levels(P.levels, max_nrhs=4)
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M0.bcg(B[:, :2])
    assert e.value.code == 3 and "hifamd_set_matrix" in e.value.msg
    # a constant-mode null-space filter on the solve is out of scope
    M0.set_matrix(P.A.indptr, P.A.indices, P.A.data)
    M0.set_nsp_const(0, -1)
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M0.bcg(B[:, :2])
    assert e.value.code == 3 and "null-space" in e.value.msg
    # not Hermitian: the QRCP last level of p2d_30
    l30, d30 = load_hier("p2d_30")
    M30 = hifir_amd.HIF.from_levels(l30, max_nrhs=4)
    M30.set_matrix(d30["A_indptr"], d30["A_indices"], d30["A_vals"])
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M30.bcg(d30["b"])
    assert e.value.code == 3 and "level 1" in e.value.msg and "dense" in e.value.msg and "is_symm" in e.value.msg


def test_same_inputs_same_bits(p32):
    import torch

    P, M = p32
    n = P.A.shape[0]
    B = U.columns(n, 40)
    first = M.bcg(B, block=16, rtol=RTOL, maxit=MAXIT)
    _hold(first, U.reference("same_bits")[1], P.A, B, RTOL)
    M.pcg(B[:, :5].copy(), rtol=RTOL, maxit=MAXIT)  # the pool's vectors go to another solver and come back
    again = M.bcg(B, block=16, rtol=RTOL, maxit=MAXIT)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    # the torch-device entry gives the host entry's bits, also on a strided block
    Xd, fd, idv, rd = M.bcg(torch.from_numpy(B).cuda(), block=16, rtol=RTOL, maxit=MAXIT)
    assert np.array_equal(Xd.cpu().numpy(), first[0]) and all(np.array_equal(a, b) for a, b in zip((fd, idv, rd), first[1:]))
    # ldb, ldx > nrhs through the C entry: b at column 2 and x at column 1 of their blocks, the padding of both untouched
    wide = torch.full((n, 47), 7.25, dtype=torch.float64, device="cuda")
    wide[:, 2:42] = torch.from_numpy(B).cuda()
    out = torch.full((n, 45), -3.5, dtype=torch.float64, device="cuda")
    Bv, xv = wide[:, 2:42], out[:, 1:41]
    fs, its, rs = np.full(40, -7, dtype=np.int32), np.full(40, -7, dtype=np.int32), np.full(6, -7, dtype=np.int32)
    st = hifir_amd.lib().hifamd_bcg_batch_dev(M._h, Bv.data_ptr(), Bv.stride(0), xv.data_ptr(), xv.stride(0), 40, 16, RTOL,
                                              U.DEFTOL, MAXIT, 0, fs.ctypes.data, its.ctypes.data, rs.ctypes.data)
    torch.cuda.synchronize()
    assert st == 0
    o, w = out.cpu().numpy(), wide.cpu().numpy()
    assert np.array_equal(o[:, 1:41], first[0]) and all(np.array_equal(a, b) for a, b in zip((fs, its, rs), first[1:]))
    assert (o[:, :1] == -3.5).all() and (o[:, 41:] == -3.5).all()
    assert (w[:, :2] == 7.25).all() and (w[:, 42:] == 7.25).all() and np.array_equal(w[:, 2:42], B)
    # a vector: block 1
    x, f, i, r = M.bcg(B[:, 3].copy(), block=1, rtol=RTOL, maxit=MAXIT)
    x2, f2, i2, r2 = M.bcg(B[:, 3:4].copy(), block=64, rtol=RTOL, maxit=MAXIT)
    _hold((x[:, None], np.array([f]), np.array([i]), r), U.reference("vector")[1], P.A, B[:, 3:4], RTOL)
    assert np.array_equal(x, x2[:, 0]) and (f, i) == (int(f2[0]), int(i2[0])) and r.tolist() == r2.tolist() == [1, 1]


def test_complex_hermitian_pair(p32):
    P, M = p32
    lz, Az, phi = U.complex_pair()
    Mz = _handle(lz, Az, max_nrhs=8)
    B = U.columns(P.A.shape[0], 5)
    X, fl, it, rk = M.bcg(B, block=5, rtol=RTOL, maxit=MAXIT)
    Xz, flz, itz, rkz = Mz.bcg(phi[:, None] * B, block=5, rtol=RTOL, maxit=MAXIT)
    assert flz.tolist() == fl.tolist() == [0] * 5 and itz.tolist() == it.tolist() and rkz.tolist() == rk.tolist()
    for c in range(5):
        assert np.linalg.norm(Xz[:, c] - phi * X[:, c]) / np.linalg.norm(X[:, c]) <= 1e-10, c
    Bz = U.columns(P.A.shape[0], 5, seed=59, cplx=True)
    Bz[:, 3] = 0.0
    out = Mz.bcg(Bz, block=5, rtol=RTOL, maxit=MAXIT)
    _hold(out, U.reference("complex")[1], Az, Bz, RTOL)
    _hold((Xz, flz, itz, rkz), U.reference("complex_similar")[1], Az, phi[:, None] * B, RTOL)
    assert out[3].tolist() == [4, 4]


def test_projected_under_a_basis_filter():
    P = U.projected_pair()
    M = _handle(P.levels, P.A)
    M.set_nsp_basis(P.d["V"])
    B = U.columns(P.A.shape[0], 33, seed=67)
    out = M.bcg(B, block=33, rtol=P.rtol, maxit=MAXIT)
    _hold(out, U.reference("projected")[1], P.A, P.apply.proj(B), P.rtol)
    assert out[1].tolist() == [0] * 33


def test_cpp_facade_bcg(tmp_path):
    exe = str(tmp_path / "facade_bcg_test")
    libdir = os.path.join(ROOT, "hifir_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_bcg_test.cpp"), "-L", libdir, "-lhifir_amd",
                           "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FACADE BCG TEST OK" in out.stdout and "FAIL" not in out.stdout
