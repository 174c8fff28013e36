"""GPU (-m gpu): the extra-precise residual (k_crs_resid_dd through hifamd_residual_batch / _dev), iterative refinement and the
GMRES restarts under it, and GMRES-IR (Engine::gmres_ir_tile).  The kernel is held BIT FOR BIT against its numpy restatement
(xp_resid_util.resid_dd: the same IEEE operations in the same order, so no tolerance applies) at every lane map, 64 / R rows
per wave, a ragged second tile, strided blocks, real and complex, A and A^H; the drivers against the integer solutions of the
graded matrices (forward error 2 eps under the compensated residual, above 1e-10 without it: test_xp_resid_host.py pins that
margin) and against the rational residual on the fixtures."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import hifir_amd
import xp_resid_util as U
from hifir_amd._lib import lib
from krylov_edges_util import identity_levels

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 15, 16, 17, 33, 48, 49, 64, 65, 130)
WMAX = max(WIDTHS)
SIZES = (1, 63, 64, 65, 257, "rows")  # "rows": 320 rows, among them rows with 0, 1, 2 and 300 nonzeros
SENTINEL = 7.25


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _matrix(size, cplx):
    """a random sparse matrix of `size` rows, some of them empty (the last one too), values over twelve decades"""
    rng = np.random.default_rng(300 + (size if size != "rows" else 999) + 10000 * cplx)
    if size == "rows":
        n = 320
        nnz = [0, 1, 2, 300] + [int(k) for k in rng.integers(0, 9, n - 5)] + [0]
    else:
        n = size
        nnz = [int(k) for k in rng.integers(0, min(n, 12) + 1, n)]
        if n > 1:
            nnz[-1] = 0
    rows = [np.sort(rng.choice(n, k, replace=False)) for k in nnz]
    indptr = np.concatenate([[0], np.cumsum(nnz)]).astype(np.int64)
    indices = (np.concatenate(rows) if indptr[-1] else np.zeros(0)).astype(np.int32)
    draw = lambda: rng.normal(size=int(indptr[-1])) * 10.0 ** rng.integers(-6, 7, int(indptr[-1]))
    vals = draw() + 1j * draw() if cplx else draw()
    return n, indptr, indices, vals


def _vec(rng, shape, cplx):
    v = rng.normal(size=shape)
    return v + 1j * rng.normal(size=shape) if cplx else v


class KernelCase:
    """one matrix, a WMAX-wide batch and its restated residuals (computed once, never written to), a handle per lane-map rule"""

    def __init__(self, size, cplx):
        self.n, self.ip, self.ix, self.v = _matrix(size, cplx)
        self.cplx = cplx
        self.dtype = np.complex128 if cplx else np.float64
        rng = np.random.default_rng(17)
        self.X = _vec(rng, (self.n, WMAX), cplx).astype(self.dtype)
        A = sp.csr_matrix((self.v, self.ix, self.ip), shape=(self.n, self.n))
        # b = fl(A x) + a little: the residual is mostly cancellation
        self.B = np.ascontiguousarray(A @ self.X + 1e-9 * _vec(rng, (self.n, WMAX), cplx)).astype(self.dtype)
        self.R_dd = U.resid_dd(self.ip, self.ix, self.v, self.B, self.X)
        self.R_wk = U.resid_working(self.ip, self.ix, self.v, self.B, self.X)
        self.handles = {}
        self._adj = None

    def handle(self, min_logr=6):
        if min_logr not in self.handles:
            old = os.environ.get("HIFIR_AMD_MIN_LOGR")
            os.environ["HIFIR_AMD_MIN_LOGR"] = str(min_logr)  # (read when the handle is created)
            try:
                levels = identity_levels(self.n)
                M = hifir_amd.HIF.from_levels(levels, max_nrhs=64, dtype=self.dtype)
                M.set_matrix(self.ip, self.ix, self.v)
            finally:
                if old is None:
                    os.environ.pop("HIFIR_AMD_MIN_LOGR", None)
                else:
                    os.environ["HIFIR_AMD_MIN_LOGR"] = old
            self.handles[min_logr] = M
        return self.handles[min_logr]

    def adjoint(self):
        if self._adj is None:
            ip, ix, v = U.adjoint_crs(self.ip, self.ix, self.v, self.n)
            self._adj = (U.resid_dd(ip, ix, v, self.B[:, :17], self.X[:, :17]), U.resid_working(ip, ix, v, self.B[:, :17], self.X[:, :17]))
        return self._adj


@pytest.fixture(scope="module")
def kcases():
    made = {}

    def get(size, cplx):
        if (size, cplx) not in made:
            made[size, cplx] = KernelCase(size, cplx)
        return made[size, cplx]

    return get


def resid_call(M, B, X, trans=False, mode=1, pad=(0, 0, 0), dev=False):
    """hifamd_residual_batch (host blocks) or _dev (CUDA tensors) with row strides width + pad for B, X and R; the padding of R
    has to come back untouched; -> R (n, width)"""
    n, w = B.shape
    op = 1 if trans else 0
    blocks = []
    for src, p in ((B, pad[0]), (X, pad[1]), (None, pad[2])):
        blk = np.full((n, w + p), SENTINEL, dtype=B.dtype)
        if src is not None:
            blk[:, :w] = src
        blocks.append(blk)
    if dev:
        import torch

        tb, tx, tr = (torch.from_numpy(b).cuda() for b in blocks)
        hifir_amd.hif._check(lib().hifamd_residual_batch_dev(M._h, op, tb.data_ptr(), tb.stride(0), tx.data_ptr(), tx.stride(0),
                                                            tr.data_ptr(), tr.stride(0), w, mode, None))
        M.sync()
        out = tr.cpu().numpy()
    else:
        hifir_amd.hif._check(lib().hifamd_residual_batch(M._h, op, _p(blocks[0]), w + pad[0], _p(blocks[1]), w + pad[1],
                                                        _p(blocks[2]), w + pad[2], w, mode))
        out = blocks[2]
    assert np.all(out[:, w:] == SENTINEL), "the padding of R was written"
    return np.ascontiguousarray(out[:, :w])


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["d", "z"])
@pytest.mark.parametrize("size", SIZES)
def test_compensated_residual_equals_the_restatement_bit_for_bit(kcases, size, cplx):
    """every width (every logR under both lane-map rules, a second tile with a ragged end), host and device blocks; as every
    width is held against the same WMAX-wide restatement, a column's bits depend on no width either"""
    K = kcases(size, cplx)
    for min_logr in (6, 0):
        M = K.handle(min_logr)
        for w in WIDTHS:
            for dev in (False, True):
                R = resid_call(M, K.B[:, :w], K.X[:, :w], dev=dev)
                assert same_bits(R, K.R_dd[:, :w]), (size, cplx, min_logr, w, dev, int(np.sum(R != K.R_dd[:, :w])))


@pytest.mark.parametrize("cplx", [False, True], ids=["d", "z"])
def test_column_alone_equals_column_of_the_wide_call(kcases, cplx):
    K = kcases(257, cplx)
    M = K.handle()
    wide = resid_call(M, K.B, K.X, dev=True)
    for c in (0, 63, 64, 129):
        assert same_bits(resid_call(M, K.B[:, c:c + 1], K.X[:, c:c + 1], dev=True), wide[:, c:c + 1])


@pytest.mark.parametrize("cplx", [False, True], ids=["d", "z"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_row_strides_larger_than_the_width(kcases, cplx, dev):
    K = kcases(65, cplx)
    for min_logr in (6, 0):
        M = K.handle(min_logr)
        for w in (3, 17, 65):
            for pad in ((2, 0, 0), (0, 5, 0), (0, 0, 1), (3, 1, 7)):
                for mode, ref in ((1, K.R_dd), (0, K.R_wk)):
                    assert same_bits(resid_call(M, K.B[:, :w], K.X[:, :w], mode=mode, pad=pad, dev=dev), ref[:, :w]), (w, pad, mode)


@pytest.mark.parametrize("cplx", [False, True], ids=["d", "z"])
@pytest.mark.parametrize("size", (65, "rows"))
def test_adjoint_residual_equals_the_restatement_on_the_conjugate_transpose(kcases, size, cplx):
    K = kcases(size, cplx)
    dd, wk = K.adjoint()
    M = K.handle()
    assert same_bits(resid_call(M, K.B[:, :17], K.X[:, :17], trans=True), dd)
    assert same_bits(resid_call(M, K.B[:, :17], K.X[:, :17], trans=True, mode=0, dev=True), wk)


@pytest.mark.parametrize("cplx", [False, True], ids=["d", "z"])
@pytest.mark.parametrize("size", SIZES)
def test_working_precision_mode_returns_the_bits_of_its_restatement(kcases, size, cplx):
    K = kcases(size, cplx)
    M = K.handle()
    for w in (1, 17, 64, 130):
        assert same_bits(resid_call(M, K.B[:, :w], K.X[:, :w], mode=0), K.R_wk[:, :w])
    # mode -1 is the handle's
    assert M.residual_precision() == 0
    assert same_bits(resid_call(M, K.B[:, :17], K.X[:, :17], mode=-1), K.R_wk[:, :17])
    M.set_residual_precision(1)
    try:
        assert same_bits(resid_call(M, K.B[:, :17], K.X[:, :17], mode=-1), K.R_dd[:, :17])
        assert same_bits(M.residual(K.B[:, :17], K.X[:, :17]), K.R_dd[:, :17])
        assert same_bits(M.residual(K.B[:, :17], K.X[:, :17], precise=False), K.R_wk[:, :17])
    finally:
        M.set_residual_precision(0)


@pytest.mark.parametrize("cplx", [False, True], ids=["d", "z"])
def test_nan_and_inf_columns_change_no_bit_of_their_neighbours(kcases, cplx):
    K = kcases(257, cplx)
    for min_logr in (6, 0):
        M = K.handle(min_logr)
        for w in (17, 65):
            B, X = K.B[:, :w].copy(), K.X[:, :w].copy()
            X[:, 1] = np.nan
            B[:, 3] = np.inf
            X[5, w - 1] = -np.inf
            R = resid_call(M, B, X, dev=True)
            keep = [c for c in range(w) if c not in (1, 3, w - 1)]
            assert same_bits(np.ascontiguousarray(R[:, keep]), np.ascontiguousarray(K.R_dd[:, :w][:, keep]))
            assert not np.all(np.isfinite(R[:, [1, 3, w - 1]]))


def test_refusals(kcases):
    K = kcases(63, False)
    M = K.handle()
    n, L = K.n, lib()
    B, X = np.ascontiguousarray(K.B[:, :4]), np.ascontiguousarray(K.X[:, :4])
    R = np.zeros_like(B)
    call = lambda h, op, b, x, r, mode, ldr=4, nrhs=4: L.hifamd_residual_batch(h, op, _p(b), 4, _p(x), 4, _p(r), ldr, nrhs, mode)
    assert call(None, 0, B, X, R, 1) == 1  # NULL handle: HIFAMD_NULL_OBJ
    assert L.hifamd_residual_precision(None) == -1
    assert L.hifamd_set_residual_precision(None, 1) == 1
    assert call(M._h, 2, B, X, R, 1) == 2 and call(M._h, 3, B, X, R, 1) == 2  # HIFAMD_M / HIFAMD_MH: MISMATCHED_SIZES
    assert call(M._h, 0, B, X, R, 2) == 2 and call(M._h, 0, B, X, R, -2) == 2  # bad mode
    assert L.hifamd_set_residual_precision(M._h, 2) == 2 and L.hifamd_set_residual_precision(M._h, -1) == 2
    assert M.residual_precision() == 0
    assert call(M._h, 0, B, X, B, 1) == 3 and call(M._h, 0, B, X, X, 1) == 3  # R aliases B or X: BAD_PREC
    assert call(M._h, 0, B, X, R, 1, ldr=3) == 2 and call(M._h, 0, B, X, R, 1, nrhs=0) == 2
    assert L.hifamd_residual_batch(M._h, 0, None, 4, _p(X), 4, _p(R), 4, 4, 1) == 1
    # no matrix; not finalized (the mode can be set on either)
    N = hifir_amd.HIF.from_levels(identity_levels(n), max_nrhs=8)
    assert call(N._h, 0, B, X, R, 1) == 3 and call(N._h, 1, B, X, R, 1) == 3
    with pytest.raises(hifir_amd.hif.HifAmdError):
        N.gmres_ir(B)
    F = hifir_amd.HIF()
    F.add_level(identity_levels(n)[0])
    F.set_residual_precision(1)
    assert F.residual_precision() == 1
    assert call(F._h, 0, B, X, R, 1) == 3
    # GMRES-IR: gmres's refusals plus inner_rtol outside (0, 1) and max_outer < 1
    for kw in (dict(inner_rtol=0.0), dict(inner_rtol=1.0), dict(max_outer=0), dict(restart=0), dict(inner_maxit=0), dict(rtol=0.0)):
        with pytest.raises(hifir_amd.hif.HifAmdError) as e:
            M.gmres_ir(B, **kw)
        assert e.value.code == 2, kw


# ---- the drivers on the graded matrices ------------------------------------------------------------------------------------
CASES = [(w, z) for w in (0, 1) for z in (False, True)]
IDS = ["graded%d-%s" % (U.GRADED[w][0], "z" if z else "d") for w, z in CASES]


class Graded:
    def __init__(self, which, cplx):
        C = U.graded_case(which, cplx)
        self.C, self.n = C, C["n"]
        self.ip, self.ix, self.v = C["indptr"], C["indices"], C["vals"]
        self.XT = np.concatenate([C["XT"], np.zeros((self.n, 1), dtype=C["XT"].dtype)], axis=1)  # five columns and a zero one
        self.B = np.concatenate([C["B"], np.zeros((self.n, 1), dtype=C["B"].dtype)], axis=1)
        self.levels = U.one_level(C["A"])
        self.M = self.new_handle()

    def new_handle(self):
        M = hifir_amd.HIF.from_levels(self.levels, max_nrhs=64)
        M.set_matrix(self.ip, self.ix, self.v)
        return M

    def ok(self, X):
        return U.fwd_ok(X[:, :U.NCOLS], self.XT[:, :U.NCOLS]) and not np.any(X[:, U.NCOLS])


@pytest.fixture(scope="module")
def graded():
    made = {}

    def get(which, cplx):
        if (which, cplx) not in made:
            made[which, cplx] = Graded(which, cplx)
        return made[which, cplx]

    return get


@pytest.mark.parametrize("which,cplx", CASES, ids=IDS)
def test_refinement_reaches_the_integer_solution_only_under_the_compensated_residual(graded, which, cplx):
    G = graded(which, cplx)
    M = G.M
    assert M.residual_precision() == 0
    X0 = M.hifir(G.B, 8)
    err0 = min(U.fwd_err(X0[:, c], G.XT[:, c]) for c in range(U.NCOLS))
    print("mode 0: smallest forward error of a column %.3e" % err0)
    assert err0 > 1e-10
    M.set_residual_precision(1)
    try:
        X1 = M.hifir(G.B, 8)
        print("mode 1: forward error %.3e" % U.fwd_err(X1[:, :U.NCOLS], G.XT[:, :U.NCOLS]))
        assert G.ok(X1)
        Xb, it, fl = M.hifir(G.B, 30, betas=[1e-14, 1e3])
        print("mode 1, bounded: iterations", it, "flags", fl)
        assert not np.any(fl) and np.all(it[:U.NCOLS] <= 4) and it[U.NCOLS] == 0
    finally:
        M.set_residual_precision(0)
    assert same_bits(M.hifir(G.B, 8), X0)  # mode 1 and back: the mode-0 bits


@pytest.mark.parametrize("which,cplx", [(0, False), (0, True)], ids=["graded48-d", "graded48-z"])
def test_environment_variable_at_creation_equals_the_setter(graded, which, cplx):
    G = graded(which, cplx)
    G.M.set_residual_precision(1)
    try:
        X1 = G.M.hifir(G.B, 8)
    finally:
        G.M.set_residual_precision(0)
    os.environ["HIFIR_AMD_RESIDUAL"] = "1"
    try:
        E = G.new_handle()
    finally:
        os.environ.pop("HIFIR_AMD_RESIDUAL", None)
    assert E.residual_precision() == 1 and G.new_handle().residual_precision() == 0
    assert same_bits(E.hifir(G.B, 8), X1)


@pytest.mark.parametrize("which,cplx", CASES, ids=IDS)
def test_adjoint_refinement_follows_the_mode(graded, which, cplx):
    """hifamd_apply_batch(HIFAMD_SH, nirs = 8): the adjoint engine is built after the mode was set, or receives it later"""
    G = graded(which, cplx)
    ipt, ixt, vt = U.adjoint_crs(G.ip, G.ix, G.v, G.n)
    BH = U.exact_rhs(ipt, ixt, vt, G.XT)
    for set_first in (True, False):
        M = G.new_handle()
        if set_first:
            M.set_residual_precision(1)
        else:
            X0 = M.hifir(BH, 8, trans=True)  # builds the adjoint engine under mode 0
            assert min(U.fwd_err(X0[:, c], G.XT[:, c]) for c in range(U.NCOLS)) > 1e-10
            M.set_residual_precision(1)
        assert G.ok(M.hifir(BH, 8, trans=True)), set_first


@pytest.mark.parametrize("which,cplx", CASES, ids=IDS)
def test_gmres_ir_on_the_graded_cases(graded, which, cplx):
    G = graded(which, cplx)
    # rtol = eps / cond(A) (xp_resid_util.RTOL_FWD): b is exact, the iteration ends on xt itself
    X, fl, ou, it, rr = G.M.gmres_ir(G.B, rtol=U.RTOL_FWD, full_rank=True)
    print("flags", fl, "corrections", ou, "inner iterations", it, "relres", rr)
    assert not np.any(fl) and np.all(ou <= 4) and ou[U.NCOLS] == 0 and it[U.NCOLS] == 0
    assert G.ok(X)
    assert np.all(rr <= 1e-14)
    R = U.resid_dd(G.ip, G.ix, G.v, G.B, X)
    for c in range(U.NCOLS):
        want = np.linalg.norm(R[:, c]) / np.linalg.norm(G.B[:, c])
        assert abs(rr[c] - want) <= 1e-3 * want, (c, rr[c], want)
    # the default tolerance stops at a certified 1e-14
    X, fl, ou, it, rr = G.M.gmres_ir(G.B, full_rank=True)
    assert not np.any(fl) and np.all(ou <= 4) and np.all(rr <= 1e-14)
    R = U.resid_dd(G.ip, G.ix, G.v, G.B, X)
    for c in range(U.NCOLS):
        want = np.linalg.norm(R[:, c]) / np.linalg.norm(G.B[:, c])
        assert abs(rr[c] - want) <= 1e-3 * want, (c, rr[c], want)
    # a CUDA tensor takes the device-pointer entry
    import torch

    Xd, fld, oud, itd, rrd = G.M.gmres_ir(torch.from_numpy(G.B).cuda(), full_rank=True)
    assert same_bits(Xd.cpu().numpy(), X) and np.array_equal(fld, fl) and np.array_equal(oud, ou) and np.array_equal(rrd, rr)


def test_column_fates_in_one_tile(graded):
    G = graded(0, False)
    M, n = G.M, G.n
    rng = np.random.default_rng(3)
    # exact, exact, exact, zero, and fl(A y) for a y of order one: a solution of modest size that no vector of doubles hits
    base = np.concatenate([G.B[:, :3], np.zeros((n, 1)), (G.C["A"] @ rng.normal(size=n)).reshape(n, 1)], axis=1)
    kw = dict(rtol=1e-30, full_rank=True)
    X, fl, ou, it, rr = M.gmres_ir(base, **kw)
    print("flags", fl, "corrections", ou, "relres", rr)
    # the exact columns end on xt with the residual 0; the zero column never starts
    assert list(fl[:4]) == [0, 0, 0, 0] and U.fwd_ok(X[:, :3], G.XT[:, :3]) and np.all(rr[:4] == 0)
    assert ou[3] == 0 and it[3] == 0 and not np.any(X[:, 3])
    # the last column's residual stops falling near eps, far above 1e-30: flag 1, and x is the iterate whose certificate is
    # returned -- the restated residual of the returned x IS relres
    assert fl[4] == 1 and ou[4] >= 1 and rr[4] <= 1e-14
    want = np.linalg.norm(U.resid_dd(G.ip, G.ix, G.v, base[:, 4], X[:, 4])) / np.linalg.norm(base[:, 4])
    assert abs(rr[4] - want) <= 1e-3 * want, (rr[4], want)
    # a NaN column: flag 1 at once, its neighbours bitwise as beside a zero column
    bad = base.copy()
    bad[:, 3] = np.nan
    Xn, fln, oun, itn, rrn = M.gmres_ir(bad, **kw)
    keep = [0, 1, 2, 4]
    assert fln[3] == 1 and oun[3] == 0 and itn[3] == 0
    assert same_bits(np.ascontiguousarray(Xn[:, keep]), np.ascontiguousarray(X[:, keep]))
    assert np.array_equal(fln[keep], fl[keep]) and np.array_equal(oun[keep], ou[keep]) and np.array_equal(rrn[keep], rr[keep])
    # one NaN entry in a column that is otherwise solvable: the same
    bad = base.copy()
    bad[n // 2, 1] = np.nan
    Xn, fln, oun, itn, rrn = M.gmres_ir(bad, **kw)
    keep = [0, 2, 3, 4]
    assert fln[1] == 1 and oun[1] == 0
    assert same_bits(np.ascontiguousarray(Xn[:, keep]), np.ascontiguousarray(X[:, keep]))
    # max_outer = 1: one correction, then flag 2 (the zero column: still flag 0)
    X1, fl1, ou1, it1, rr1 = M.gmres_ir(base, max_outer=1, **kw)
    assert list(fl1) == [2, 2, 2, 0, 2] and list(ou1) == [1, 1, 1, 0, 1]
    assert np.all(rr1[[0, 1, 2, 4]] > 0) and np.all(rr1[[0, 1, 2, 4]] < 1e-10)


def test_one_handle_serves_gmres_refinement_and_gmres_ir_in_turn(graded):
    G = graded(0, True)
    kw = dict(rtol=U.RTOL_FWD, full_rank=True)
    fresh = G.new_handle()
    want6 = fresh.gmres_ir(G.B, **kw)
    want3 = G.new_handle().gmres_ir(G.B[:, :3], **kw)
    M = G.new_handle()
    xg = M.gmres(G.B, rtol=1e-8, full_rank=True)[0]
    xh = M.hifir(G.B, 3)
    for want, B in ((want6, G.B), (want3, np.ascontiguousarray(G.B[:, :3])), (want6, G.B)):
        got = M.gmres_ir(B, **kw)
        assert same_bits(got[0], want[0]) and all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:]))
        assert same_bits(M.gmres(G.B, rtol=1e-8, full_rank=True)[0], xg) and same_bits(M.hifir(G.B, 3), xh)
    assert same_bits(want6[0][:, :3].copy(), want3[0])  # (and a column's bits do not depend on the width)


# ---- GMRES-IR on the fixtures that carry their matrix ----------------------------------------------------------------------
@pytest.mark.parametrize("name", U.FIXTURES)
def test_gmres_ir_on_the_fixtures(name):
    C = U.fixture_case(name)
    M = hifir_amd.HIF.from_levels(C["levels"], max_nrhs=64)
    M.set_matrix(C["indptr"], C["indices"], C["vals"])
    B3 = C["B"]
    X, fl, ou, it, rr = M.gmres_ir(B3)
    print(name, "flags", fl, "corrections", ou, "inner iterations", it, "relres", rr)
    assert not np.any(fl)
    for c in range(3):
        true = U.exact_norm(U.resid_exact(C["indptr"], C["indices"], C["vals"], B3[:, c], X[:, c])) / np.linalg.norm(B3[:, c])
        assert true <= 2e-14, (c, true)
        assert abs(rr[c] - true) <= 1e-3 * true, (c, rr[c], true)
    # widths 1, 17, 64, 65: a column keeps its bits (the three columns repeated with small integer factors)
    wide = np.concatenate([B3 * (1 + k) for k in range(22)], axis=1)[:, :65]
    X65 = M.gmres_ir(wide)
    assert not np.any(X65[1])
    assert same_bits(np.ascontiguousarray(X65[0][:, :3]), X)
    for w in (1, 17, 64):
        Xw = M.gmres_ir(np.ascontiguousarray(wide[:, :w]))
        assert same_bits(Xw[0], np.ascontiguousarray(X65[0][:, :w])), w
        assert all(np.array_equal(a, b[:w]) for a, b in zip(Xw[1:], X65[1:])), w
