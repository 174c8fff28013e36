"""GPU (-m gpu): PCG, BiCGSTAB and symmetric QMR -- the three solvers on the lock-step scaffold of engine.hip (kr_vec, krylov_state,
krylov_batch, cg_close_mode) -- at their batch, fate and stopping edges: every width at which the 64-column tile cut and the
lane = column mapping can go wrong, columns that leave one tile at different steps for different reasons, every finishing-kernel
mode an exact construction reaches, maxit on either side of a converging column, strided device blocks, reuse of one handle's
pool by other solvers and widths, non-finite neighbours, and the projected iteration.  Every column is held against its own
single-column restatement (lockstep_edges_util; test_lockstep_edges_host.py pins the inputs, the margins of every decision and
the tolerance table): (flag, iterations) equal, x within lockstep_edges_util.tolerance, and equal bits wherever bits are claimed
(a column alone against the same column in a batch, host entry against device entry, a power-of-two scaled copy)."""
import numpy as np
import pytest

import hifir_amd
import lockstep_edges_util as U
from util import relerr

pytestmark = pytest.mark.gpu

REAL_PAIRS = [("pcg", "p2d_32_symm"), ("sqmr", "shift2d_32_symm"), ("sqmr", "kktr_24_symm"), ("bicgstab", "cd2d_48")]
COMPLEX_PAIRS = [("pcg", "p2d_32_symm_z"), ("bicgstab", "young1c")]
ONE_PER_SOLVER = [("pcg", "p2d_32_symm"), ("sqmr", "shift2d_32_symm"), ("bicgstab", "cd2d_48")]
PROJECTED = [("pcg", "neu2d_32_symm"), ("sqmr", "neu2d_32_symm")]
WIDTH_CASES = [(s, n, w) for s, n in REAL_PAIRS + COMPLEX_PAIRS for w in U.CONFIG[s, n]["widths"]]


@pytest.fixture(scope="module")
def handles():
    """(solver, name) -> (the pair of lockstep_edges_util, its handle); "exact", solver -> (ExactCase, its handle)"""
    made = {}

    def get(solver, name):
        if (solver, name) not in made:
            if solver == "exact":
                P = U.ExactCase(name)
            else:
                P = U.pair(solver, name)
            M = hifir_amd.HIF.from_levels(P.levels, max_nrhs=64)
            M.set_matrix(P.A.indptr, P.A.indices, P.A.data)
            if solver != "exact" and P.cfg.get("proj"):
                M.set_nsp_basis(P.d["V"])
            made[solver, name] = (P, M)
        return made[solver, name]

    yield get
    for P, M in made.values():
        M.close()


def run(M, solver, B, rtol, maxit=U.MAXIT):
    return getattr(M, solver)(B, rtol=rtol, maxit=maxit)


def colerr(x, xo):
    return 0.0 if not xo.any() and not x.any() else relerr(x, xo)


def check_against_restatement(P, B, fates, X, fl, it, maxit=U.MAXIT, kinds=None):
    """every column: (flag, iterations) of its restatement, x within the tolerance of its kind; -> largest error by kind"""
    worst = {}
    for c, f in enumerate(fates):
        xo, fo, io, _ = P.restated(B[:, c], maxit=maxit)
        assert (int(fl[c]), int(it[c])) == (fo, io), (c, f, (int(fl[c]), int(it[c])), (fo, io))
        if not xo.any():
            assert (fo, io) == (0, 0) and not X[:, c].any(), (c, f)
            continue
        kind = kinds[c] if kinds else U.kind_of(f)
        e = colerr(X[:, c], xo)
        worst[kind] = max(worst.get(kind, 0.0), e)
        assert e <= U.tolerance(P, kind), (c, f, e, U.tolerance(P, kind))
    return worst


def check_scaled_copies(fates, X, fl, it):
    for c, f in enumerate(fates):
        if f in U.SCALED_COPY_OF:  # 2^-100 times the first hard column, 2^+100 times the first easy one: the same bits, scaled
            o = fates.index(U.SCALED_COPY_OF[f])
            assert (int(fl[c]), int(it[c])) == (int(fl[o]), int(it[o])), (c, f)
            assert np.array_equal(X[:, c], X[:, o] * (2.0 ** -100 if f == "tiny" else 2.0 ** 100)), (c, f)


def check_alone(M, solver, B, X, fl, it, cols, rtol, maxit=U.MAXIT):
    """the columns `cols` solved alone: the bits, flag and count they have in the batch"""
    for c in sorted(set(cols)):
        x, f, i = run(M, solver, B[:, c].copy(), rtol, maxit)
        assert (f, i) == (int(fl[c]), int(it[c])), (c, (f, i), (int(fl[c]), int(it[c])))
        assert np.array_equal(x, X[:, c], equal_nan=True), c


def check_device_entry(M, solver, B, X, fl, it, rtol, maxit=U.MAXIT):
    torch = pytest.importorskip("torch")
    Xd, fd, idv = run(M, solver, torch.from_numpy(np.ascontiguousarray(B)).cuda(), rtol, maxit)
    assert np.array_equal(Xd.cpu().numpy(), X, equal_nan=True) and np.array_equal(fd, fl) and np.array_equal(idv, it)


def edge_columns(width):
    return [c for c in (0, 31, 32, 63, 64, width - 1) if c < width]


# ---- a. widths, mixed fates -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,name,width", WIDTH_CASES)
def test_mixed_fates_at_every_width(handles, solver, name, width):
    P, M = handles(solver, name)
    B, fates = P.batch(width)
    X, fl, it = run(M, solver, B, P.rtol)
    worst = check_against_restatement(P, B, fates, X, fl, it)
    check_scaled_copies(fates, X, fl, it)
    if width >= 33:  # the fates really leave the tile at different steps
        assert len({int(v) for v in it[:64]}) >= 5
    check_alone(M, solver, B, X, fl, it, edge_columns(width), P.rtol)
    check_device_entry(M, solver, B, X, fl, it, P.rtol)
    print(solver, name, "width", width, "largest relerr by kind", {k: "%.1e" % v for k, v in worst.items()})


# ---- b. exact fates ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [5, 64, 65, 130])
@pytest.mark.parametrize("solver", list(U.EXACT_FATES))
def test_exact_fates(handles, solver, width):
    # every finishing-kernel mode an exact construction reaches, next to a column that runs 10 .. 35 steps longer; a frozen column
    # keeps its bits through all of them, and through the one frozen pass after a breakdown in the last mode
    E, M = handles("exact", solver)
    B, fates = E.batch(width)
    X, fl, it = run(M, solver, B, U.EXACT_RTOL, U.EXACT_MAXIT)
    got = [(int(f), int(i)) for f, i in zip(fl, it)]
    assert got == [E.expected(f) for f in fates], [(c, f, g, E.expected(f)) for c, (f, g) in enumerate(zip(fates, got)) if g != E.expected(f)]
    check_alone(M, solver, B, X, fl, it, range(width), U.EXACT_RTOL, U.EXACT_MAXIT)
    check_device_entry(M, solver, B, X, fl, it, U.EXACT_RTOL, U.EXACT_MAXIT)
    for c, f in enumerate(fates):
        if f != "hard" and E.expected(f)[0] == 0:
            xe = E.exact_x(f) * E.scale(c)
            assert np.abs(X[:, c] - xe).max() <= 1e-14 * np.abs(xe).max(), (c, f)
        if f in ("rho0", "sigma0", "nan", "skew"):  # stopped before the first update: x is the zero it started from
            assert not X[:, c].any(), (c, f)
        rows = np.ones(B.shape[0], dtype=bool)
        rows[E.rows[f]] = False
        assert not X[rows, c].any(), (c, f)  # nothing outside the column's own block


def test_diagonal_hierarchy_is_exact(handles):
    for solver in U.EXACT_FATES:
        E, M = handles("exact", solver)
        n = E.A.shape[0]
        assert np.array_equal(M.solve_mrhs(np.eye(n)), np.diag(E.sign))
        assert M.is_hermitian()


# ---- c. a column does not see its neighbours -----------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [33, 64])
@pytest.mark.parametrize("solver,name", ONE_PER_SOLVER)
def test_column_does_not_see_its_neighbours(handles, solver, name, width):
    P, M = handles(solver, name)
    B, fates = P.batch(width)
    for keep in sorted({0, 32, width - 1}):
        assert fates[keep] == "hard"
        x, f, i = run(M, solver, B[:, keep].copy(), P.rtol)
        assert f == 0
        for how in ("zero", "nan", "inf", "big"):
            X, fl, it = run(M, solver, U.neighbours_replaced(B, keep, how), P.rtol)
            assert np.array_equal(X[:, keep], x) and (int(fl[keep]), int(it[keep])) == (f, i), (keep, how)
            others = np.arange(width) != keep
            if how == "zero":
                assert not fl[others].any() and not it[others].any() and not X[:, others].any()
            else:
                assert (fl[others] == 1).all(), (how, fl)
            if how == "nan":  # broken down before the first update: no iteration, and x is the zero it started from
                assert not it[others].any() and not X[:, others].any(), how


# ---- d. maxit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", list(U.MAXIT_EDGES))
def test_maxit_beside_a_converging_column(handles, solver):
    # maxit = m on columns that need m - 1, m and m + 1: converged exactly at maxit is flag 0, one more is flag 2 with the
    # iterate of step m; BiCGSTAB with m odd (the half step, mode 2) and even (the full step, mode 4)
    for name, m, spec in U.MAXIT_EDGES[solver]:
        P, M = handles(solver, name)
        B = U.maxit_columns(P, spec)
        X, fl, it = run(M, solver, B, P.rtol, m)
        assert fl.tolist() == [0, 0, 2] and it.tolist() == [m - 1, m, m], (m, fl, it)
        kinds = ["ladder" if what == "pow" else "hard" for what, k in spec]
        worst = check_against_restatement(P, B, ["edge"] * 3, X, fl, it, maxit=m, kinds=kinds)
        check_alone(M, solver, B, X, fl, it, range(3), P.rtol, m)
        print(solver, name, "maxit", m, {k: "%.1e" % v for k, v in worst.items()})


@pytest.mark.parametrize("maxit", [1, 2, 3])
@pytest.mark.parametrize("solver,name", ONE_PER_SOLVER)
def test_smallest_maxit(handles, solver, name, maxit):
    P, M = handles(solver, name)
    B, fates = P.batch(3)
    X, fl, it = run(M, solver, B, P.rtol, maxit)
    assert fl.tolist() == [2, 0, 2] and it.tolist() == [maxit, 0, maxit]
    check_against_restatement(P, B, fates, X, fl, it, maxit=maxit)
    check_alone(M, solver, B, X, fl, it, range(3), P.rtol, maxit)


# ---- e. strided device blocks -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,stride", [(5, 9), (70, 80)])
@pytest.mark.parametrize("solver,name", ONE_PER_SOLVER)
def test_strided_device_blocks(handles, solver, name, width, stride):
    # ldb, ldx > nrhs, b at column 2 and x at column 1 of their blocks: the bits of the contiguous call, the padding of both
    # blocks untouched and b itself unchanged (BiCGSTAB reads its shadow residual from it in place, with stride ldb)
    torch = pytest.importorskip("torch")
    P, M = handles(solver, name)
    B, fates = P.batch(width)
    n = B.shape[0]
    Bd = torch.from_numpy(B).cuda()
    wide = torch.full((n, stride), 7.25, dtype=Bd.dtype, device="cuda")
    wide[:, 2:2 + width] = Bd
    Bv = wide[:, 2:2 + width]
    assert Bv.stride(0) == stride
    entry = getattr(hifir_amd.lib(), "hifamd_%s_batch_dev" % solver)

    def strided(fl, it):
        out = torch.full((n, stride), -3.5, dtype=Bd.dtype, device="cuda")
        x = out[:, 1:1 + width]
        st = entry(M._h, Bv.data_ptr(), Bv.stride(0), x.data_ptr(), x.stride(0), width, P.rtol, U.MAXIT, 0,
                   None if fl is None else fl.ctypes.data, None if it is None else it.ctypes.data)
        torch.cuda.synchronize()
        assert st == 0
        o = out.cpu().numpy()
        assert (o[:, :1] == -3.5).all() and (o[:, 1 + width:] == -3.5).all()
        return o[:, 1:1 + width]

    fl, it = np.full(width, -7, dtype=np.int32), np.full(width, -7, dtype=np.int32)
    Xs = strided(fl, it)
    Xc, flc, itc = run(M, solver, Bd, P.rtol)
    assert np.array_equal(Xs, Xc.cpu().numpy()) and np.array_equal(fl, flc) and np.array_equal(it, itc)
    check_against_restatement(P, B, fates, Xs, fl, it)
    if width == 70:  # no flags, no counts
        assert np.array_equal(strided(None, None), Xs)
    w = wide.cpu().numpy()
    assert (w[:, :2] == 7.25).all() and (w[:, 2 + width:] == 7.25).all() and np.array_equal(w[:, 2:2 + width], B)


# ---- f. no trace between calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,name", [("pcg", "p2d_32_symm"), ("sqmr", "shift2d_32_symm"), ("bicgstab", "p2d_32_symm")])
def test_no_trace_between_calls(handles, solver, name):
    # kr_vec is laid out [n][nc] and never cleared, the state block and the pinned read-back are shared: a 70-column solve gives
    # the same bits after other solvers ran at other widths (other layouts of the same bytes), one of them with NaN columns.
    # BiCGSTAB is recorded on the positive definite pair, whose hierarchy every interleaved solver accepts.
    P, M = handles("pcg" if solver == "bicgstab" else solver, name)
    B70, fates = P.batch(70)
    first = run(M, solver, B70, P.rtol)
    assert len({int(v) for v in first[2]}) >= 5
    B33 = P.batch(33)[0]
    run(M, "sqmr", P.batch(3)[0], P.rtol)
    out = run(M, "bicgstab", U.neighbours_replaced(B33, 0, "nan"), P.rtol)
    assert (out[1][1:] == 1).all()
    M.gmres(P.batch(65)[0], restart=12, rtol=1e-9, maxit=60)
    run(M, "pcg", P.batch(5)[0], P.rtol)
    M.hifir(B33, 8, betas=(2e-3, 0.5))
    again = run(M, solver, B70, P.rtol)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    check_scaled_copies(fates, *again)


# ---- g. projected -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [33, 65])
@pytest.mark.parametrize("solver,name", PROJECTED)
def test_projected_batches(handles, solver, name, width):
    # the basis filter installed: the restatement runs with P M^{-1} and P b.  One more column equal to the basis vector has
    # P b = rounding noise: whatever the iteration makes of it is finite and the other columns do not notice
    P, M = handles(solver, name)
    B, fates = P.batch(width)
    X, fl, it = run(M, solver, B, P.rtol)
    worst = check_against_restatement(P, B, fates, X, fl, it)
    for c in range(width):
        if X[:, c].any():
            assert np.abs(P.Q.conj().T @ X[:, c]).max() <= 1e-10 * np.linalg.norm(X[:, c]), c
    check_alone(M, solver, B, X, fl, it, edge_columns(width), P.rtol)
    X2, fl2, it2 = run(M, solver, np.column_stack([B, P.d["V"][:, 0]]), P.rtol)
    assert np.isfinite(X2[:, width]).all()
    assert np.array_equal(X2[:, :width], X) and np.array_equal(fl2[:width], fl) and np.array_equal(it2[:width], it)
    print(solver, name, "width", width, "largest relerr by kind", {k: "%.1e" % v for k, v in worst.items()})
