"""GPU (-m gpu): the batched right-preconditioned BiCGSTAB driver (hifamd_bicgstab_batch / HIF.bicgstab) against a
numpy restatement of the same recursion around the oracle's apply (orc.Oracle.solve as M^{-1}), its batch-width
independence, the half-step exit and an exact breakdown on a synthetic M^{-1} = I hierarchy, maxit and NaN columns,
refusals, the null-space filter, and the 1M-row default Poisson hierarchy where the compiled reference travelled."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import hifir_amd
from hifir_amd._lib import lib
from lockstep_edges_util import bicgstab_restated
from oracle import orc, ref
from util import load_hier, poisson2d, relerr

pytestmark = pytest.mark.gpu

NULL_OBJ, MISMATCHED_SIZES, BAD_PREC = 1, 2, 3


def _matrix(d):
    n = len(d["b"])
    return sp.csr_matrix((d["A_vals"], d["A_indices"], d["A_indptr"]), shape=(n, n))


_CACHE = {}


def _fixture(name, max_nrhs=64):
    if (name, max_nrhs) not in _CACHE:
        levels, d = load_hier(name)
        M = hifir_amd.HIF.from_levels(levels, max_nrhs=max_nrhs)
        M.set_matrix(d["A_indptr"], d["A_indices"], d["A_vals"])
        _CACHE[(name, max_nrhs)] = (levels, d, M, orc.Oracle(levels), _matrix(d))
    return _CACHE[(name, max_nrhs)]


def _columns(d, A):
    n = len(d["b"])
    rng = np.random.default_rng(5)
    cols = [rng.uniform(-1, 1, n), np.zeros(n), d["b"], A @ np.ones(n), 1e-30 * rng.uniform(-1, 1, n)]
    if np.iscomplexobj(d["b"]) or np.iscomplexobj(A.data):
        cols[0] = cols[0] + 1j * rng.uniform(-1, 1, n)
    return np.stack(cols, axis=1).astype(np.result_type(d["b"], A.data))


def _check_vs_restated(X, fl, it, Xo, fo, io, A, B, rtol):
    assert fl.tolist() == fo.tolist() and it.tolist() == io.tolist(), (fl, fo, it, io)
    for c in range(B.shape[1]):
        if not np.any(B[:, c]):
            assert it[c] == 0 and fl[c] == 0 and not np.any(X[:, c])
            continue
        assert relerr(X[:, c], Xo[:, c]) <= 1e-8, c
        if fl[c] == 0:
            assert np.linalg.norm(A @ X[:, c] - B[:, c]) / np.linalg.norm(B[:, c]) <= 10 * rtol, c


# Every fixture below converges to both tolerances within MAXIT steps (flag 0 on every nonzero column; asserted).
MAXIT = 400


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", ["cd2d_48", "p2d_30", "p2d_30_lup", "p2d_64_deep", "young1c", "kkt_26"])
def test_bicgstab_vs_restatement(name, rtol):
    levels, d, M, O, A = _fixture(name)
    x, flag, it = M.bicgstab(d["b"], rtol=rtol, maxit=MAXIT)
    xo, fo, io = bicgstab_restated(O, A, d["b"], rtol, MAXIT)
    assert (flag, it) == (int(fo[0]), int(io[0]))
    assert relerr(x, xo[:, 0]) <= 1e-8
    B = _columns(d, A)
    X, fl, it = M.bicgstab(B, rtol=rtol, maxit=MAXIT)
    Xo, fo, io = bicgstab_restated(O, A, B, rtol, MAXIT)
    _check_vs_restated(X, fl, it, Xo, fo, io, A, B, rtol)
    assert fl.tolist() == [0] * 5 and it[1] == 0, (fl, it)


def test_column_bits_do_not_depend_on_the_batch():
    import torch

    levels, d, M, O, A = _fixture("cd2d_48")
    n = len(d["b"])
    rng = np.random.default_rng(17)
    B = rng.uniform(-1, 1, size=(n, 70))
    B[:, 9] = 0.0
    kw = dict(rtol=1e-9, maxit=MAXIT)
    X70, f70, i70 = M.bicgstab(B, **kw)
    X64, f64, i64 = M.bicgstab(np.ascontiguousarray(B[:, :64]), **kw)
    X5, f5, i5 = M.bicgstab(np.ascontiguousarray(B[:, :5]), **kw)
    assert np.array_equal(X64, X70[:, :64]) and np.array_equal(f64, f70[:64]) and np.array_equal(i64, i70[:64])
    assert np.array_equal(X5, X70[:, :5]) and np.array_equal(f5, f70[:5]) and np.array_equal(i5, i70[:5])
    for k in (0, 3, 9, 63, 64, 69):
        x, f, i = M.bicgstab(B[:, k].copy(), **kw)
        assert np.array_equal(x, X70[:, k]) and (f, i) == (f70[k], i70[k]), k
    assert f70.tolist() == [0] * 70 and i70[9] == 0
    # the torch-device entry gives the host entry's bits
    Xd, fd, idv = M.bicgstab(torch.from_numpy(np.ascontiguousarray(B[:, :5])).cuda(), **kw)
    assert np.array_equal(Xd.cpu().numpy(), X5) and np.array_equal(fd, f5) and np.array_equal(idv, i5)
    xd, f, i = M.bicgstab(torch.from_numpy(B[:, 3].copy()).cuda(), **kw)
    assert np.array_equal(xd.cpu().numpy(), X70[:, 3]) and (f, i) == (f70[3], i70[3])
    Xd, fd, idv = M.bicgstab(torch.from_numpy(B).cuda(), **kw)
    assert np.array_equal(Xd.cpu().numpy(), X70) and np.array_equal(fd, f70) and np.array_equal(idv, i70)


def _identity_hierarchy(n, A, max_nrhs=8):
    """One level with m = n, L = U = 0, d = s = t = 1, p = q = identity, no Schur complement: M^{-1} = I."""
    lv = dict(m=n, n=n)
    for k, ncols in (("L", n), ("U", n), ("E", n), ("F", 0)):  # empty CCS blocks (E: 0 x n, F: n x 0)
        lv[k + "_colptr"], lv[k + "_rowind"], lv[k + "_vals"] = np.zeros(ncols + 1, np.int64), np.zeros(0, np.int32), np.zeros(0)
    lv["d"], lv["s"], lv["t"] = np.ones(n), np.ones(n), np.ones(n)
    for k in ("p", "q", "p_inv", "q_inv"):
        lv[k] = np.arange(n, dtype=np.int32)
    M = hifir_amd.HIF.from_levels([lv], max_nrhs=max_nrhs)
    A = sp.csr_matrix(A)
    A.sort_indices()
    M.set_matrix(A.indptr, A.indices, A.data)
    return M


def test_half_step_exit_and_exact_breakdown():
    n = 1000
    rng = np.random.default_rng(3)
    B = rng.integers(-4, 5, size=(n, 3)).astype(np.float64)
    B[0, :] = 1.0  # no zero column
    # A = 2I: alpha = 1/2 exactly, r = 0 after the first half step
    M2 = _identity_hierarchy(n, 2.0 * sp.identity(n))
    X, fl, it = M2.bicgstab(B, rtol=1e-12, maxit=50)
    assert fl.tolist() == [0, 0, 0] and it.tolist() == [1, 1, 1]
    assert np.array_equal(X, B / 2)
    # skew-symmetric A (2x2 blocks [[0, 1], [-1, 0]]), small integers: (r^, v) = b^T A b is exactly 0 in any order
    K = sp.kron(sp.identity(n // 2), sp.csr_matrix(np.array([[0.0, 1.0], [-1.0, 0.0]]))).tocsr()
    K.eliminate_zeros()
    Mk = _identity_hierarchy(n, K)
    X, fl, it = Mk.bicgstab(B, rtol=1e-12, maxit=50)
    assert fl.tolist() == [1, 1, 1] and it.tolist() == [1, 1, 1]
    assert not np.any(X)


def test_maxit_and_nan_columns():
    levels, d, M, O, A = _fixture("cd2d_48")
    b = d["b"]
    for maxit in (1, 2):
        x, flag, it = M.bicgstab(b, rtol=1e-14, maxit=maxit)
        xo, fo, io = bicgstab_restated(O, A, b, 1e-14, maxit)
        assert (flag, it) == (2, maxit) == (int(fo[0]), int(io[0]))
        assert relerr(x, xo[:, 0]) <= 1e-8
    rng = np.random.default_rng(31)
    B = np.stack([b, rng.uniform(-1, 1, len(b)), np.full(len(b), np.nan), d["b2"]], axis=1)
    B[7, 2] = 1.0
    X, fl, it = M.bicgstab(B, rtol=1e-10, maxit=MAXIT)
    assert fl[2] == 1 and it[2] == 0
    keep = [0, 1, 3]
    Xk, fk, ik = M.bicgstab(np.ascontiguousarray(B[:, keep]), rtol=1e-10, maxit=MAXIT)
    assert np.array_equal(X[:, keep], Xk) and fl[keep].tolist() == fk.tolist() == [0, 0, 0]
    assert it[keep].tolist() == ik.tolist()


def _raw(M, dev, B, X, nrhs, rtol=1e-6, maxit=10):
    fl = np.zeros(max(nrhs, 1), dtype=np.int32)
    it = np.zeros(max(nrhs, 1), dtype=np.int32)
    fn = lib().hifamd_bicgstab_batch_dev if dev else lib().hifamd_bicgstab_batch
    if dev:
        pb, px, ldb, ldx = B.data_ptr(), X.data_ptr(), B.stride(0), X.stride(0)
    else:
        pb, px, ldb, ldx = B.ctypes.data, X.ctypes.data, B.shape[1], X.shape[1]
    return fn(M._h, pb, ldb, px, ldx, nrhs, float(rtol), int(maxit), 0, fl.ctypes.data, it.ctypes.data)


@pytest.mark.parametrize("dev", [False, True])
def test_refusals(dev):
    import torch

    levels, d, M, O, A = _fixture("cd2d_48")
    n = len(d["b"])

    def blk(k):
        B = np.random.default_rng(k).uniform(-1, 1, size=(n, k))
        return torch.from_numpy(B).cuda() if dev else B

    B, X = blk(2), blk(2)
    assert _raw(M, dev, B, X, 2) == 0
    assert _raw(M, dev, B, X, 2, rtol=0.0) == MISMATCHED_SIZES
    assert _raw(M, dev, B, X, 2, rtol=-1.0) == MISMATCHED_SIZES
    assert _raw(M, dev, B, X, 2, maxit=0) == MISMATCHED_SIZES
    assert _raw(M, dev, B, B, 2) == BAD_PREC  # aliased b and x
    st = (lib().hifamd_bicgstab_batch_dev if dev else lib().hifamd_bicgstab_batch)(None, 0, 1, 0, 1, 1, 1e-6, 10, 0,
                                                                                    None, None)
    assert st == NULL_OBJ
    # no matrix
    M0 = hifir_amd.HIF.from_levels(levels, max_nrhs=4)
    assert _raw(M0, dev, B, X, 2) == BAD_PREC
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M0.bicgstab(B)
    assert e.value.code == BAD_PREC and "hifamd_set_matrix" in e.value.msg
    # a batch wider than the handle was finalized for (tile width 4)
    os.environ["HIFIR_AMD_MIN_LOGR"] = "0"
    try:
        M4 = hifir_amd.HIF.from_levels(levels, max_nrhs=4)
    finally:
        os.environ.pop("HIFIR_AMD_MIN_LOGR", None)
    M4.set_matrix(d["A_indptr"], d["A_indices"], d["A_vals"])
    B8, X8 = blk(8), blk(8)
    assert _raw(M4, dev, B8, X8, 8) == MISMATCHED_SIZES
    assert _raw(M4, dev, B, X, 2) == 0
    # the Python entry refuses the same arguments
    for kw in ({"rtol": 0.0}, {"maxit": 0}):
        with pytest.raises(hifir_amd.HifAmdError) as e:
            M.bicgstab(B, **kw)
        assert e.value.code == MISMATCHED_SIZES


def test_null_space_filter_is_honoured():
    levels, d = load_hier("cd2d_48")
    M = hifir_amd.HIF.from_levels(levels, max_nrhs=8)
    M.set_matrix(d["A_indptr"], d["A_indices"], d["A_vals"])
    M.set_nsp_const(0, -1)
    O, A = orc.Oracle(levels), _matrix(d)
    B = np.stack([d["b"], d["b2"], np.random.default_rng(41).uniform(-1, 1, len(d["b"]))], axis=1)
    # (only the first steps: on this nonsingular matrix the filtered M^{-1} makes the recursion amplify rounding, a
    # relative perturbation of 1e-15 per apply of the restatement moves its x by 1e-2 after 5 steps)
    for maxit in (1, 2):
        X, fl, it = M.bicgstab(B, rtol=1e-14, maxit=maxit)
        Xo, fo, io = bicgstab_restated(O, A, B, 1e-14, maxit, nsp=True)
        assert fl.tolist() == fo.tolist() == [2, 2, 2] and it.tolist() == io.tolist() == [maxit] * 3
        for c in range(3):
            assert relerr(X[:, c], Xo[:, c]) <= 1e-8, (maxit, c)
    # the filter changes the result
    Xf, _, _ = M.bicgstab(B, rtol=1e-14, maxit=2)
    Xu, _, _ = _fixture("cd2d_48")[2].bicgstab(B, rtol=1e-14, maxit=2)
    assert relerr(Xf, Xu) > 1e-6


@pytest.mark.skipif(not ref.available(), reason="compiled reference not present")
def test_1m_default_hierarchy_bicgstab():
    """The bench workload: the 1000^2 Poisson matrix factorized with default parameters by the compiled reference."""
    import torch

    A = poisson2d(1000)
    R = ref.RefHIF(A.indptr, A.indices, A.data)
    levels = R.levels()
    M = hifir_amd.HIF.from_levels(levels, max_nrhs=64)
    M.set_matrix(A.indptr, A.indices, A.data)
    n = A.shape[0]
    # device memory of the first call on 64 torch-device columns (work vectors, partials, state and X itself)
    Bd = torch.from_numpy(np.random.default_rng(37).uniform(-1, 1, size=(n, 64))).cuda()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    Xd, fl, it = M.bicgstab(Bd, rtol=1e-8, maxit=4)
    torch.cuda.synchronize()
    taken = free0 - torch.cuda.mem_get_info()[0]
    assert taken <= 7 * n * 64 * 8, taken
    assert fl.tolist() == [2] * 64 and it.tolist() == [4] * 64
    del Xd, Bd
    B = np.random.default_rng(29).uniform(-1, 1, size=(n, 8))
    X, fl, it = M.bicgstab(B, rtol=1e-8, maxit=1000)
    assert fl.tolist() == [0] * 8, (fl, it)
    res = np.linalg.norm(A @ X - B, axis=0) / np.linalg.norm(B, axis=0)
    assert res.max() <= 1e-7, res
