"""GPU (-m gpu): the restarted block GCR driver (hifamd_bgcr_batch / HIF.bgcr) against the numpy restatement of the same
recurrence around the oracle's apply (blockgcr_util.bgcr_restated; test_blockgcr_host.py pins every input used here away
from its decisions): block widths and tile cuts, restart and maxit edges, deflation at the start and rank loss inside a
cycle, stagnation, excluded columns, refusals, a hierarchy PCG refuses, repeatability, a complex pair, a filtered apply and
the C++ facade."""
import os
import subprocess

import numpy as np
import pytest

import blockgcr_util as U
import hifir_amd
from krylov_edges_util import neighbours_replaced
from util import load_hier, relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXIT = U.MAXIT


def _handle(levels, A, max_nrhs=64):
    M = hifir_amd.HIF.from_levels(levels, max_nrhs=max_nrhs)
    M.set_matrix(A.indptr, A.indices, A.data)
    return M


@pytest.fixture(scope="module")
def cd48():
    P = U.cd48()
    return P, _handle(P.levels, P.A)


def _hold(out, ref, A, B, rtol):
    """flags, steps and ranks equal; x within 1e-8 of the restatement's per column; the true residual of a flag-0 column
    <= 2 rtol (the flag was decided on a true residual; test_blockgcr_host.py bounds what the two computations differ by)"""
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
            assert np.linalg.norm(B[:, c] - A @ X[:, c]) / np.sqrt(b2[c]) <= 2 * rtol, c


def _against(M, name, **kw):
    (solve, A, B, block, restart, rtol, maxit), ref = U.reference(name)
    out = M.bgcr(B, block=block, restart=restart, rtol=rtol, maxit=maxit, **kw)
    _hold(out, ref, A, B, rtol)
    return out, B


@pytest.mark.parametrize("width", U.WIDTHS)
def test_block_widths(cd48, width):
    out, B = _against(cd48[1], "width%d" % width)
    assert out[1].tolist() == [0] * width and out[3].tolist()[0] == width


@pytest.mark.parametrize("nrhs,block", U.CUTS)
def test_tile_cuts(cd48, nrhs, block):
    P, M = cd48
    out, B = _against(M, "cut%d_%d" % (nrhs, block))
    last = nrhs - (nrhs - 1) // block * block
    assert out[1].tolist() == [0] * nrhs and out[3].tolist()[-2] == last and len(out[3]) == 2 * (-(-nrhs // block))
    # the tiles are independent of each other: the last one alone gives the same bits
    alone = M.bgcr(np.ascontiguousarray(B[:, nrhs - last:]), block=block, restart=U.RESTART, rtol=P.rtol, maxit=MAXIT)
    assert np.array_equal(alone[0], out[0][:, nrhs - last:]) and np.array_equal(alone[2], out[2][nrhs - last:])


@pytest.mark.parametrize("name", ["restart1", "restart2", "restart3", "restart_long", "restart_exact"])
def test_restart_edges(cd48, name):
    out, B = _against(cd48[1], name)
    assert out[1].tolist() == [2 if name == "restart1" else 0] * 17


@pytest.mark.parametrize("maxit", [10, 11, 3])
def test_maxit_at_the_edges_of_a_cycle(cd48, maxit):
    out, B = _against(cd48[1], "maxit%d" % maxit)
    assert out[1].tolist() == [2] * 16 and out[2].tolist() == [maxit] * 16


def test_deflation_at_the_start(cd48):
    out, B = _against(cd48[1], "deflation")
    assert out[1].tolist() == [0] * 8 and out[3].tolist() == [5, 5] and out[2][4] == 0


def test_rank_loss_inside_a_cycle():
    levels, A, B = U.nonsym_rank_loss_case()
    M = _handle(levels, A, max_nrhs=8)
    out, B = _against(M, "rank_loss")
    assert out[1].tolist() == [0] * 5 and out[3].tolist() == [5, 3]


def test_fewer_rows_than_columns():
    levels, A, B = U.tiny_case()
    M = _handle(levels, A, max_nrhs=8)
    out, B = _against(M, "tiny")
    assert out[1].tolist() == [0] * 5 and out[3].tolist() == [3, 3]


def test_stagnation(cd48):
    """an rtol below what the pair can attain: flag 1 everywhere.  The cycle in which the largest true residual stops
    falling hangs on a rounding (test_blockgcr_host.py), so the count is held to the restatement's plus one cycle."""
    P, M = cd48
    (solve, A, B, block, restart, rtol, maxit), (Xo, fo, io, ro) = U.reference("stagnation")
    X, fl, it, rk = M.bgcr(B, block=block, restart=restart, rtol=rtol, maxit=maxit)
    assert fl.tolist() == fo.tolist() == [1] * 16 and (it == it[0]).all() and 0 < it[0] <= io[0] + restart
    assert np.linalg.norm(B - A @ X) <= 1e-8 * np.linalg.norm(B)  # (it stagnated at the level of the rounding, not before)


@pytest.mark.parametrize("how", ["nan", "inf", "big"])
def test_excluded_columns_do_not_touch_their_neighbour(cd48, how):
    P, M = cd48
    B = U.columns(P.A.shape[0], 5)
    keep = 2
    kw = dict(block=5, restart=U.RESTART, rtol=P.rtol, maxit=MAXIT)
    X0, f0, i0, r0 = M.bgcr(neighbours_replaced(B, keep, "zero"), **kw)
    X, fl, it, rk = M.bgcr(neighbours_replaced(B, keep, how), **kw)
    assert np.array_equal(X[:, keep], X0[:, keep]) and (fl[keep], it[keep]) == (f0[keep], i0[keep]) == (0, i0[keep])
    others = np.arange(5) != keep
    assert (fl[others] == 1).all() and not it[others].any() and not X[:, others].any()
    assert not f0[others].any() and not i0[others].any() and rk.tolist() == r0.tolist() == [1, 1]
    _hold((X0, f0, i0, r0), U.reference("excluded")[1], P.A, neighbours_replaced(B, keep, "zero"), P.rtol)


def test_refusals(cd48):
    P, M = cd48
    B = U.columns(P.A.shape[0], 4)
    for kw in ({"rtol": 0.0}, {"rtol": -1.0}, {"maxit": 0}, {"block": 0}, {"block": 65}, {"restart": 0}, {"restart": 65},
               {"deftol": 0.0}, {"deftol": 1.0}):
        with pytest.raises(hifir_amd.HifAmdError) as e:
            M.bgcr(B, **kw)
        assert e.value.code == 2, kw
    M0 = hifir_amd.HIF.from_levels(P.levels, max_nrhs=4)
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M0.bgcr(B[:, :2])
    assert e.value.code == 3 and "hifamd_set_matrix" in e.value.msg


def test_a_hierarchy_pcg_refuses_is_accepted():
    l30, d30 = load_hier("p2d_30")
    M30 = hifir_amd.HIF.from_levels(l30, max_nrhs=8)
    M30.set_matrix(d30["A_indptr"], d30["A_indices"], d30["A_vals"])
    assert not M30.is_hermitian()
    with pytest.raises(hifir_amd.HifAmdError):
        M30.pcg(d30["b"])
    out, B = _against(M30, "qrcp")
    assert out[1].tolist() == [0] * 5


def test_same_inputs_same_bits(cd48):
    import torch

    P, M = cd48
    n = P.A.shape[0]
    kw = dict(block=16, restart=U.RESTART, rtol=P.rtol, maxit=MAXIT)
    first, B = _against(M, "same_bits")
    M.bicgstab(B[:, :5].copy(), rtol=P.rtol, maxit=MAXIT)  # the pool's vectors go to another solver and come back
    M.gmres(B[:, :3].copy())  # (and the basis buffers to GMRES)
    again = M.bgcr(B, **kw)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    # the torch-device entry gives the host entry's bits
    Xd, fd, idv, rd = M.bgcr(torch.from_numpy(B).cuda(), **kw)
    assert np.array_equal(Xd.cpu().numpy(), first[0]) and all(np.array_equal(a, b) for a, b in zip((fd, idv, rd), first[1:]))
    # ldb, ldx > nrhs through the C entry: b at column 2 and x at column 1 of their blocks, the padding of both untouched
    wide = torch.full((n, 47), 7.25, dtype=torch.float64, device="cuda")
    wide[:, 2:42] = torch.from_numpy(B).cuda()
    out = torch.full((n, 45), -3.5, dtype=torch.float64, device="cuda")
    Bv, xv = wide[:, 2:42], out[:, 1:41]
    fs, its, rs = np.full(40, -7, dtype=np.int32), np.full(40, -7, dtype=np.int32), np.full(6, -7, dtype=np.int32)
    st = hifir_amd.lib().hifamd_bgcr_batch_dev(M._h, Bv.data_ptr(), Bv.stride(0), xv.data_ptr(), xv.stride(0), 40, 16,
                                               U.RESTART, P.rtol, U.DEFTOL, MAXIT, 0, fs.ctypes.data, its.ctypes.data,
                                               rs.ctypes.data)
    torch.cuda.synchronize()
    assert st == 0
    o, w = out.cpu().numpy(), wide.cpu().numpy()
    assert np.array_equal(o[:, 1:41], first[0]) and all(np.array_equal(a, b) for a, b in zip((fs, its, rs), first[1:]))
    assert (o[:, :1] == -3.5).all() and (o[:, 41:] == -3.5).all()
    assert (w[:, :2] == 7.25).all() and (w[:, 42:] == 7.25).all() and np.array_equal(w[:, 2:42], B)
    # NULL flags, iters and ranks
    st = hifir_amd.lib().hifamd_bgcr_batch_dev(M._h, Bv.data_ptr(), Bv.stride(0), xv.data_ptr(), xv.stride(0), 40, 16,
                                               U.RESTART, P.rtol, U.DEFTOL, MAXIT, 0, None, None, None)
    torch.cuda.synchronize()
    assert st == 0 and np.array_equal(out.cpu().numpy()[:, 1:41], first[0])
    # a vector: block 1 against block 64
    kv = dict(restart=U.RESTART, rtol=P.rtol, maxit=MAXIT)
    x, f, i, r = M.bgcr(B[:, 3].copy(), block=1, **kv)
    x2, f2, i2, r2 = M.bgcr(B[:, 3:4].copy(), block=64, **kv)
    _hold((x[:, None], np.array([f]), np.array([i]), r), U.reference("vector")[1], P.A, B[:, 3:4], P.rtol)
    assert np.array_equal(x, x2[:, 0]) and (f, i) == (int(f2[0]), int(i2[0])) and r.tolist() == r2.tolist() == [1, 1]


@pytest.mark.parametrize("name", ["complex5", "complex33"])
def test_complex_pair(name):
    Y = U.young()
    M = _handle(Y.levels, Y.A)
    out, B = _against(M, name)
    assert not any(out[1]) and out[3].tolist()[0] == (4 if name == "complex5" else 33)


def test_filtered_apply():
    P = U.filtered_pair()
    M = _handle(P.levels, P.A)
    M.set_nsp_basis(P.d["V"])
    (solve, A, B, block, restart, rtol, maxit), ref = U.reference("filtered")  # (B = P b: consistent)
    out = M.bgcr(B, block=block, restart=restart, rtol=rtol, maxit=maxit)
    _hold(out, ref, A, B, rtol)
    assert out[1].tolist() == [0] * 33


def test_cpp_facade_bgcr(tmp_path):
    exe = str(tmp_path / "facade_bgcr_test")
    libdir = os.path.join(ROOT, "hifir_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_bgcr_test.cpp"), "-L", libdir, "-lhifir_amd",
                           "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FACADE BGCR TEST OK" in out.stdout and "FAIL" not in out.stdout
