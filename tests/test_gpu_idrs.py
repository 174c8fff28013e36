"""GPU (-m gpu): the batched IDR(s) driver (hifamd_idrs_batch / _dev, HIF.idrs) against its single-column restatement
(idrs_util; test_idrs_host.py pins the inputs, the vetted columns and the tolerance table): flags and steps equal and x within
the table's bound on every vetted column at every width and s, equal bits wherever bits are claimed (a column alone and in any
batch, host and device entry, strided blocks, replays, after other solvers used the shared pool, beside NaN neighbours), maxit on
either side of a converging column, the exact constructions, the generated shadow block, the null-space filters, a system larger
than one trip of the row walk, the refusals in their order, and the reason for the solver: fewer steps than BiCGSTAB."""
import numpy as np
import pytest
import scipy.sparse as sp

import hifir_amd
import idrs_util as U
import lockstep_edges_util as L
from hifir_amd._lib import lib
from util import relerr

pytestmark = pytest.mark.gpu

WIDTH_CASES = [(name, s, w) for name, s in U.CASES for w in U.widths_of(name, s)]
NULL_OBJ, MISMATCHED_SIZES, BAD_PREC = 1, 2, 3


@pytest.fixture(scope="module")
def handles():
    """fixture name -> its handle with the perturbed matrix attached (one for every s); "exact" -> the diagonal hierarchy's"""
    made = {}

    def get(name):
        if name not in made:
            if name == "exact":
                E = U.exact_case()
                levels, A = E["levels"], E["A"]
            elif name == "p2d_32_symm":
                P = L.pair("pcg", name)
                levels, A = P.levels, P.A
            else:
                P = U.pair(name, 4)
                levels, A = P.levels, P.A
            M = hifir_amd.HIF.from_levels(levels, max_nrhs=64)
            M.set_matrix(A.indptr, A.indices, A.data)
            made[name] = M
        return made[name]

    yield get
    for M in made.values():
        M.close()


def run(M, P, B, maxit=U.MAXIT, **kw):
    if P.gen is None:
        kw.setdefault("P", P.P)
    else:
        kw.setdefault("seed", P.gen)
    return M.idrs(B, s=P.s, rtol=P.rtol, maxit=maxit, **kw)


def check_against_restatement(P, B, fates, cols, X, fl, it, maxit=U.MAXIT, kinds=None):
    """the columns `cols`: (flag, steps) of the restatement, x within the tolerance of the kind; -> largest error by kind"""
    worst = {}
    for c in cols:
        xo, fo, io, _ = P.restated(B[:, c], maxit=maxit)
        assert (int(fl[c]), int(it[c])) == (fo, io), (c, fates[c], (int(fl[c]), int(it[c])), (fo, io))
        if not xo.any():
            assert (fo, io) == (0, 0) and not X[:, c].any(), (c, fates[c])
            continue
        kind = kinds[c] if kinds else L.kind_of(fates[c])
        e = relerr(X[:, c], xo)
        worst[kind] = max(worst.get(kind, 0.0), e)
        assert e <= U.tolerance(P, kind), (c, fates[c], e, U.tolerance(P, kind))
    return worst


def check_scaled_copies(fates, X, fl, it):
    for c, f in enumerate(fates):
        if f in L.SCALED_COPY_OF:  # 2^-100 times the first hard column, 2^+100 times the first easy one: the same bits, scaled
            o = fates.index(L.SCALED_COPY_OF[f])
            assert (int(fl[c]), int(it[c])) == (int(fl[o]), int(it[o])), (c, f)
            assert np.array_equal(X[:, c], X[:, o] * (2.0 ** -100 if f == "tiny" else 2.0 ** 100)), (c, f)


def check_alone(M, P, B, X, fl, it, cols, maxit=U.MAXIT):
    for c in sorted(set(cols)):
        x, f, i = run(M, P, B[:, c].copy(), maxit)
        assert (f, i) == (int(fl[c]), int(it[c])), (c, (f, i), (int(fl[c]), int(it[c])))
        assert np.array_equal(x, X[:, c], equal_nan=True), c


def check_device_entry(M, P, B, X, fl, it, maxit=U.MAXIT):
    torch = pytest.importorskip("torch")
    Xd, fd, idv = run(M, P, torch.from_numpy(np.ascontiguousarray(B)).cuda(), maxit)
    assert np.array_equal(Xd.cpu().numpy(), X, equal_nan=True) and np.array_equal(fd, fl) and np.array_equal(idv, it)


def edge_columns(width):
    return [c for c in (0, 31, 32, 63, 64, width - 1) if c < width]


# ---- a. widths, s, mixed fates ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,s,width", WIDTH_CASES)
def test_mixed_fates_against_the_restatement(handles, name, s, width):
    P, M = U.pair(name, s), handles(name)
    B, fates = P.batch(width)
    X, fl, it = run(M, P, B)
    worst = check_against_restatement(P, B, fates, P.vetted(width), X, fl, it)
    assert not fl.any() and (it[[c for c in range(width) if B[:, c].any()]] > 0).all()  # the unvetted columns converge too
    check_scaled_copies(fates, X, fl, it)
    if width >= 33 and name != "pcd2d_32":  # the fates really leave the tile at different steps
        assert len({int(v) for v in it[:64]}) >= 3
    check_alone(M, P, B, X, fl, it, edge_columns(width))
    check_device_entry(M, P, B, X, fl, it)
    print(name, s, "width", width, "largest relerr by kind", {k: "%.1e" % v for k, v in worst.items()})


# ---- b. a column does not see its neighbours ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cd2d_48", "young1c"])
def test_column_does_not_see_its_neighbours(handles, name):
    P, M = U.pair(name, 4), handles(name)
    width = 33
    B, fates = P.batch(width)
    X0, fl0, it0 = run(M, P, B)
    for keep in (0, 32):
        assert fates[keep] == "hard"
        for how in ("zero", "nan", "inf", "big"):
            X, fl, it = run(M, P, L.neighbours_replaced(B, keep, how))
            assert np.array_equal(X[:, keep], X0[:, keep]) and (fl[keep], it[keep]) == (fl0[keep], it0[keep]), (keep, how)
            others = np.arange(width) != keep
            if how == "zero":
                assert not fl[others].any() and not it[others].any() and not X[:, others].any()
            else:
                assert (fl[others] == 1).all(), (how, fl)
            if how == "nan":  # a non-finite column: flag 1, 0 steps, x the zero it started from
                assert not it[others].any() and not X[:, others].any()
    # one NaN column inside the mixed batch: every other column keeps its bits
    Bn = B.copy()
    Bn[:, 5] = np.nan
    X, fl, it = run(M, P, Bn)
    others = np.arange(width) != 5
    assert (fl[5], it[5]) == (1, 0) and not X[:, 5].any()
    assert np.array_equal(X[:, others], X0[:, others]) and np.array_equal(fl[others], fl0[others]) and np.array_equal(it[others], it0[others])


# ---- c. bit independence ---------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_batch_or_the_entry(handles):
    torch = pytest.importorskip("torch")
    P, M = U.pair("cd2d_48", 4), handles("cd2d_48")
    B70, fates = P.batch(70)
    n = B70.shape[0]
    col = B70[:, 0].copy()
    x, f, i = run(M, P, col)
    assert f == 0 and i == P.restated(col)[2]
    for width in (5, 64, 70):
        B = P.batch(width)[0]
        assert np.array_equal(B[:, 0], col)
        X, fl, it = run(M, P, B)
        assert np.array_equal(X[:, 0], x) and (fl[0], it[0]) == (f, i), width
        check_device_entry(M, P, B, X, fl, it)
        assert all(np.array_equal(a, b) for a, b in zip(run(M, P, B), (X, fl, it))), width  # replay
    # a strided device block: b at column 2 and x at column 1 of wider blocks, paddings and b untouched
    X70, fl70, it70 = run(M, P, B70)
    stride = 80
    wide = torch.full((n, stride), 7.25, dtype=torch.float64, device="cuda")
    wide[:, 2:72] = torch.from_numpy(B70).cuda()
    Bv = wide[:, 2:72]
    out = torch.full((n, stride), -3.5, dtype=torch.float64, device="cuda")
    xv = out[:, 1:71]
    for fl, it in ((np.full(70, -7, dtype=np.int32), np.full(70, -7, dtype=np.int32)), (None, None)):  # (flags and iters NULL)
        out[:] = -3.5
        st = lib().hifamd_idrs_batch_dev(M._h, Bv.data_ptr(), Bv.stride(0), xv.data_ptr(), xv.stride(0), 70, 4, P.P.ctypes.data, 4,
                                         0, P.rtol, U.MAXIT, 0, None if fl is None else fl.ctypes.data,
                                         None if it is None else it.ctypes.data)
        torch.cuda.synchronize()
        assert st == 0
        o = out.cpu().numpy()
        assert (o[:, :1] == -3.5).all() and (o[:, 71:] == -3.5).all() and np.array_equal(o[:, 1:71], X70)
        assert fl is None or (np.array_equal(fl, fl70) and np.array_equal(it, it70))
    w = wide.cpu().numpy()
    assert (w[:, :2] == 7.25).all() and (w[:, 72:] == 7.25).all() and np.array_equal(w[:, 2:72], B70)
    # the host entry with flags and iters NULL
    Xh = np.empty_like(B70)
    st = lib().hifamd_idrs_batch(M._h, B70.ctypes.data, 70, Xh.ctypes.data, 70, 70, 4, P.P.ctypes.data, 4, 0, P.rtol, U.MAXIT, 0,
                                 None, None)
    assert st == 0 and np.array_equal(Xh, X70)
    # a shadow block with a row stride of its own
    Pw = np.full((n, 7), np.nan)
    Pw[:, :4] = P.P
    Xs = np.empty_like(B70)
    st = lib().hifamd_idrs_batch(M._h, B70.ctypes.data, 70, Xs.ctypes.data, 70, 70, 4, Pw.ctypes.data, 7, 0, P.rtol, U.MAXIT, 0,
                                 None, None)
    assert st == 0 and np.array_equal(Xs, X70)


def test_no_trace_of_other_solvers_in_the_shared_pool(handles):
    # kr_vec is laid out [n][nc] and never cleared, the state block and the pinned read-back are shared: a 70-column IDR(4) and an
    # IDR(8) solve give the same bits after PCG, BiCGSTAB, symmetric QMR, GMRES and refinement ran at other widths, one with NaNs
    Pc, M = L.pair("pcg", "p2d_32_symm"), handles("p2d_32_symm")
    B70, B33 = Pc.batch(70)[0], Pc.batch(33)[0]
    first = [M.idrs(B70, s=s, rtol=1e-9, maxit=200, seed=3) for s in (4, 8)]
    assert all(not r[1].any() and len({int(v) for v in r[2]}) >= 2 for r in first)
    M.sqmr(Pc.batch(3)[0], rtol=1e-9, maxit=100)
    out = M.bicgstab(L.neighbours_replaced(B33, 0, "nan"), rtol=1e-9, maxit=100)
    assert (out[1][1:] == 1).all()
    M.gmres(Pc.batch(65)[0], restart=12, rtol=1e-9, maxit=60)
    M.pcg(Pc.batch(5)[0], rtol=1e-9, maxit=100)
    M.idrs(B33, s=2, rtol=1e-9, maxit=100, seed=8)
    M.hifir(B33, 8, betas=(2e-3, 0.5))
    again = [M.idrs(B70, s=s, rtol=1e-9, maxit=200, seed=3) for s in (4, 8)]
    for r0, r1 in zip(first, again):
        assert all(np.array_equal(a, b) for a, b in zip(r0, r1))
    # and the other solvers after IDR(s): BiCGSTAB's bits with and without an IDR(8) call before it
    b0 = M.bicgstab(B70, rtol=1e-9, maxit=100)
    M.idrs(B33, s=8, rtol=1e-9, maxit=100, seed=1)
    assert all(np.array_equal(a, b) for a, b in zip(b0, M.bicgstab(B70, rtol=1e-9, maxit=100)))


# ---- d. maxit ----------------------------------------------------------------------------------------------------------------------
def test_maxit_beside_a_converging_column(handles):
    for name, s, m, spec in U.MAXIT_EDGES:
        P, M = U.pair(name, s), handles(name)
        B = U.maxit_columns(P, spec)
        X, fl, it = run(M, P, B, m)
        assert fl.tolist() == [0, 0, 2] and it.tolist() == [m - 1, m, m], (m, fl, it)
        kinds = ["ladder" if what == "pow" else "hard" for what, k in spec]
        worst = check_against_restatement(P, B, ["edge"] * 3, range(3), X, fl, it, maxit=m, kinds=kinds)
        check_alone(M, P, B, X, fl, it, range(3), m)
        print(name, s, "maxit", m, {k: "%.1e" % v for k, v in worst.items()})


@pytest.mark.parametrize("maxit", [1, 2, 5, 6])
def test_smallest_maxit(handles, maxit):
    # 1, 2: inside the first cycle; 5: the first omega step; 6: the first step of the second cycle
    P, M = U.pair("cd2d_48", 4), handles("cd2d_48")
    B, fates = P.batch(3)
    X, fl, it = run(M, P, B, maxit)
    assert fl.tolist() == [2, 0, 2] and it.tolist() == [maxit, 0, maxit]
    for c in (0, 2):
        xo, fo, io, _ = P.restated(B[:, c], maxit=maxit)
        assert (fo, io) == (2, maxit) and relerr(X[:, c], xo) <= U.tolerance(P, L.kind_of(fates[c])), (c, maxit)
    check_alone(M, P, B, X, fl, it, range(3), maxit)


# ---- e. exact constructions --------------------------------------------------------------------------------------------------------
def test_exact_constructions(handles):
    E, M = U.exact_case(), handles("exact")
    n = E["A"].shape[0]
    assert np.array_equal(M.solve_mrhs(np.eye(n)), np.eye(n))
    for nm, (b, P, exp, updates) in E["cases"].items():
        s = P.shape[1]
        Xo, fo, io = U.idrs_restated(lambda r: r, E["A"], b, P, 1e-10, 50)
        # the column alone, and between scaled copies of itself in a wider batch
        B = np.stack([b * 2.0 ** ((7 * c) % 41 - 20) for c in range(5)], axis=1)
        for rhs in (b, B):
            X, fl, it = M.idrs(rhs, s=s, rtol=1e-10, maxit=50, P=P)
            X, fl, it = np.reshape(X, (n, -1)), np.atleast_1d(fl), np.atleast_1d(it)
            for c in range(X.shape[1]):
                scale = 1.0 if rhs is b else 2.0 ** ((7 * c) % 41 - 20)
                assert (int(fl[c]), int(it[c])) == exp == (int(fo[0]), int(io[0])), (nm, c, fl, it)
                assert not X[b == 0, c].any() and bool(X[:, c].any()) == (updates > 0), (nm, c)
                if nm in ("half", "skew", "pzero0"):
                    assert np.array_equal(X[:, c], Xo[:, 0] * scale), (nm, c)  # (sums of a few small integers: exact on both sides)
                else:
                    assert relerr(X[:, c], Xo[:, 0] * scale) <= 1e-13, (nm, c)
    b, P = E["cases"]["half"][:2]
    assert np.array_equal(M.idrs(b, s=2, rtol=1e-10, maxit=50, P=P)[0], b / 2)  # beta = 1/2


# ---- f. the generated shadow block ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", U.GEN_CASES)
def test_generated_shadow_block(handles, key):
    P, M = U.pair(*key), handles(key[0])
    B, fates = P.batch(33)
    X, fl, it = run(M, P, B)
    assert all(np.array_equal(a, b) for a, b in zip(run(M, P, B), (X, fl, it)))  # same seed, same bits
    worst = check_against_restatement(P, B, fates, P.vetted(33), X, fl, it)
    check_alone(M, P, B, X, fl, it, (0, 32))
    check_device_entry(M, P, B, X, fl, it)
    # the twin handed over as an explicit block: the same bits
    X2, fl2, it2 = M.idrs(B, s=P.s, rtol=P.rtol, maxit=U.MAXIT, P=P.P)
    assert np.array_equal(X2, X) and np.array_equal(fl2, fl) and np.array_equal(it2, it)
    # another seed: other bits, and it still converges
    X3, fl3, it3 = M.idrs(B, s=P.s, rtol=P.rtol, maxit=U.MAXIT, seed=P.gen + 1)
    assert not fl3.any() and not np.array_equal(X3, X)
    for c in (0, 32):
        assert np.linalg.norm(B[:, c] - P.A @ X3[:, c]) / np.linalg.norm(B[:, c]) <= P.rtol * L.MARGIN
    print(key, {k: "%.1e" % v for k, v in worst.items()})


# ---- g. null-space filters --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["const", "basis"])
def test_null_space_filters_act_on_the_applies(mode):
    # a filter on HIFAMD_S filters every M^{-1} apply and nothing else (b is taken as it is).  Only the first steps: on this
    # nonsingular matrix the filtered M^{-1} makes the recursion amplify rounding (test_gpu_bicgstab.py), so the bound of a
    # column is 1000 times what one-ulp noise on the applies does to it at that maxit, floor 1e-12
    Pr = U.pair("cd2d_48", 2)
    n = Pr.A.shape[0]
    M = hifir_amd.HIF.from_levels(Pr.levels, max_nrhs=8)
    M.set_matrix(Pr.A.indptr, Pr.A.indices, Pr.A.data)
    V = np.random.default_rng(3).uniform(-1, 1, (n, 2))
    if mode == "const":
        M.set_nsp_const(0, -1)
        solve = lambda r: (lambda y: y - y.mean())(Pr.O.solve(r))  # noqa: E731
    else:
        M.set_nsp_basis(V)
        solve = L.Filtered(Pr.O, np.linalg.qr(V)[0]).solve
    B = np.stack([Pr.hard(0), Pr.d["b"], Pr.hard(1)], axis=1)
    for maxit in (1, 2, 3, 4):  # (3: the omega step of s = 2)
        X, fl, it = M.idrs(B, s=2, rtol=1e-14, maxit=maxit, P=Pr.P)
        Xo, fo, io = U.idrs_restated(solve, Pr.A, B, Pr.P, 1e-14, maxit)
        assert fl.tolist() == fo.tolist() == [2, 2, 2] and it.tolist() == io.tolist() == [maxit] * 3
        for c in range(3):
            rng = np.random.default_rng(5)
            noisy = lambda r: (lambda y: y * (1.0 + 2.0 ** -52 * rng.uniform(-1, 1, n)))(solve(r))  # noqa: E731
            Xn = U.idrs_restated(noisy, Pr.A, B[:, c], Pr.P, 1e-14, maxit)[0][:, 0]
            bound = max(1000.0 * relerr(Xn, Xo[:, c]), 1e-12)
            assert relerr(X[:, c], Xo[:, c]) <= bound, (mode, maxit, c, relerr(X[:, c], Xo[:, c]), bound)
    Xu = U.idrs_restated(Pr.O, Pr.A, B, Pr.P, 1e-14, 4)[0]
    assert relerr(X, Xu) > 1e-6  # the filter changes the result
    M.close()


# ---- h. more rows than one trip of the row walk ---------------------------------------------------------------------------------------
def test_more_rows_than_one_trip_of_the_row_walk():
    # n = 20,517 > 4 * 4096 + 4096: the four-rows-per-trip body of the P^H x pass and its tail both run, and every fused pass
    # walks more than one trip.  M^{-1} = I, A = a diagonal in [2, 3] plus a band of width 5 and size 0.3: no reference is needed,
    # the true residual is: the recurrence stops at ||r|| <= rtol ||b|| and its distance to b - A x after some twenty
    # well-conditioned steps is a few hundred roundings (1e-13), far below the 2 % granted here
    n, rtol = 20517, 1e-8
    rng = np.random.default_rng(12)
    A = sp.diags([rng.uniform(2, 3, n)] + [0.3 * rng.uniform(-1, 1, n - abs(k)) for k in (-5, -1, 1, 5)], [0, -5, -1, 1, 5]).tocsr()
    A.sort_indices()
    M = hifir_amd.HIF.from_levels(L.diagonal_levels(np.ones(n)), max_nrhs=64)
    M.set_matrix(A.indptr, A.indices, A.data)
    B = rng.uniform(-1, 1, (n, 9))
    B[:, 4] = 0.0
    for s in (3, 8):
        X, fl, it = M.idrs(B, s=s, rtol=rtol, maxit=200, seed=2)
        assert not fl.any() and it[4] == 0 and not X[:, 4].any()
        for c in (0, 1, 2, 3, 5, 6, 7, 8):
            assert 5 <= it[c] < 100 and np.linalg.norm(B[:, c] - A @ X[:, c]) / np.linalg.norm(B[:, c]) <= rtol * L.MARGIN, (s, c)
        x, f, i = M.idrs(B[:, 8].copy(), s=s, rtol=rtol, maxit=200, seed=2)
        assert np.array_equal(x, X[:, 8]) and (f, i) == (0, it[8])
        # the restatement on the twin of the generated block: both residuals are within rtol and the eigenvalues of A lie in
        # [0.8, 4.2] (Gershgorin), so the two x differ by at most 2 cond(A) rtol <= 10.5 rtol
        Xo, fo, io = U.idrs_restated(lambda r: r, A, B[:, 8], U.generated_P(n, s, 2, False), rtol, 200)
        assert fo[0] == 0 and relerr(x, Xo[:, 0]) <= 11 * rtol
    M.close()


# ---- i. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True])
def test_refusals_in_order(handles, dev):
    torch = pytest.importorskip("torch")
    P = U.pair("cd2d_48", 4)
    M = handles("cd2d_48")
    n = P.A.shape[0]
    fn = lib().hifamd_idrs_batch_dev if dev else lib().hifamd_idrs_batch
    Bh, Xh = np.ascontiguousarray(P.batch(3)[0]), np.zeros((n, 3))
    if dev:
        Bt, Xt = torch.from_numpy(Bh).cuda(), torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        pb, px = Bt.data_ptr(), Xt.data_ptr()
    else:
        pb, px = Bh.ctypes.data, Xh.ctypes.data
    Pn = P.P.copy()
    Pn[n - 1, 3] = np.inf
    good = dict(h=M._h, B=pb, ldb=3, X=px, ldx=3, nrhs=3, s=4, P=P.P.ctypes.data, ldp=4, seed=0, rtol=1e-8, maxit=50)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], a["B"], a["ldb"], a["X"], a["ldx"], a["nrhs"], a["s"], a["P"], a["ldp"], a["seed"], a["rtol"], a["maxit"],
                  0, None, None)

    bad_all = dict(B=None, nrhs=0, ldb=2, X=pb, maxit=0, s=0, P=Pn.ctypes.data)
    order = [("h", None, NULL_OBJ), ("B", None, NULL_OBJ), ("nrhs", 0, MISMATCHED_SIZES), ("ldb", 2, MISMATCHED_SIZES),
             ("X", pb, BAD_PREC), ("maxit", 0, MISMATCHED_SIZES), ("s", 0, MISMATCHED_SIZES), ("P", Pn.ctypes.data, BAD_PREC)]
    # everything wrong at once, then one error repaired after the other: the refusals come in the documented order
    wrong = dict(h=None, **bad_all)
    for key, _, code in order:
        assert call(**wrong) == code, (key, code)
        del wrong[key]
    assert call(**wrong) == 0
    for kw in (dict(s=9), dict(s=-1), dict(ldp=3), dict(rtol=0.0)):
        assert call(**kw) == MISMATCHED_SIZES, kw
    assert call(P=None, ldp=0) == 0 and call(s=3) == 0 and call(s=8, P=None) == 0  # (ldp is not looked at without P; ldp > s is a stride)
    # needs the matrix, as BiCGSTAB does
    M2 = hifir_amd.HIF.from_levels(P.levels, max_nrhs=4)
    assert call(h=M2._h, maxit=0, s=0) == BAD_PREC
    M2.close()
    for kw in ({"rtol": 0.0}, {"maxit": 0}, {"s": 0}, {"s": 9}):
        with pytest.raises(hifir_amd.HifAmdError) as e:
            M.idrs(Bh, **kw)
        assert e.value.code == MISMATCHED_SIZES


# ---- j. the reason for the solver -----------------------------------------------------------------------------------------------------
def test_idr4_needs_fewer_steps_than_bicgstab_on_pcd2d_32(handles):
    P, M = U.pair("pcd2d_32", 4), handles("pcd2d_32")
    B, fates = P.batch(65)
    cols = [c for c in P.vetted(65) if B[:, c].any()]
    X, fl, it = run(M, P, B)
    Xb, flb, itb = M.bicgstab(B, rtol=P.rtol, maxit=U.MAXIT)
    assert not fl[cols].any() and not flb[cols].any()
    print("pcd2d_32 on the device: mean steps IDR(4) %.1f, BiCGSTAB %.1f" % (it[cols].mean(), itb[cols].mean()))
    assert it[cols].mean() <= 0.9 * itb[cols].mean()
