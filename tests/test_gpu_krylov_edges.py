"""GPU (-m gpu): the lock-step drivers around the apply -- GMRES and FGMRES (Engine::gmres_tile, the k_gm_* kernels) and iterative
refinement (Engine::hifir_dev, k_masked_add, k_colnorm2_partial) -- at their batch, restart and stopping edges: every width at
which the (row, column) thread mapping 256 / nc leaves lanes idle, columns of different fate in one tile, stagnation, the
multiple-of-restart return, restarts 1 .. 9 around kGmBlock = 4, strided device blocks, reuse of one handle's work buffers and
neighbours full of NaN.  Every column is held against its own single-column restatement (oracle.orc.gmres / fgmres,
krylov_edges_util.ir_restated; test_krylov_edges_host.py pins those and the inputs): (flag, iterations[, sweeps]) equal,
x to 1e-8 (GMRES, FGMRES) or 1e-11 (refinement), and equal bits where bits are claimed."""
import numpy as np
import pytest

import hifir_amd
from krylov_edges_util import (QUIRK, SCALED_COPY_OF, finishing_steps, ir_mixed_batch, ir_restated, mixed_batch, neighbours_replaced, perturbed,
                               stagnating_case)
from oracle import orc
from util import load_hier, relerr

pytestmark = pytest.mark.gpu

PERTURBED = {"cd2d_48": True, "young1c": False}  # fixture -> real diagonal (a real handle) or complex
GM = dict(restart=12, rtol=1e-9, maxit=300)
FGM = dict(restart=6, rtol=1e-9, maxit=100)
IR_N, IR_BOUNDED = 4, dict(nirs=8, betas=(2e-3, 0.5))
TOL_GM, TOL_IR = 1e-8, 1e-11


class Case:
    def __init__(self, levels, d, A):
        self.levels, self.d, self.A = levels, d, A
        self.M = hifir_amd.HIF.from_levels(levels, max_nrhs=64)
        self.M.set_matrix(A.indptr, A.indices, A.data)
        self.O = orc.Oracle(levels)
        self.ref, self.batches = {}, {}

    def batch(self, width, seed=11):
        if (width, seed) not in self.batches:
            self.batches[width, seed] = mixed_batch(self.O, self.d, self.A, width, seed)
        return self.batches[width, seed]

    def _cached(self, kind, b, kw, fn):
        key = (kind, b.tobytes(), tuple(sorted((k, str(v)) for k, v in kw.items())))
        if key not in self.ref:
            self.ref[key] = fn()
        return self.ref[key]

    def gmres(self, b, **kw):  # -> (x, flag, iters)
        A = self.A
        return self._cached("g", b, kw, lambda: orc.gmres(self.O, A.indptr, A.indices, A.data, b.copy(), **kw))

    def fgmres(self, b, **kw):  # -> (x, flag, iters, sweeps)
        A = self.A
        return self._cached("f", b, kw, lambda: orc.fgmres(self.O, A.indptr, A.indices, A.data, b.copy(), **kw))

    def ir(self, b, nirs, betas=None, trans=False):  # -> (x, iters, flag, ratios)
        def run():
            hist = []
            return ir_restated(self.O, self.A, b.copy(), nirs, betas, trans=trans, history=hist) + (hist,)

        return self._cached("i", b, dict(nirs=nirs, betas=betas, trans=trans), run)


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            if name == "stag":
                S = stagnating_case()
                made[name] = Case(S["levels"], S, S["A"])
            elif name == "irmix":
                S = ir_mixed_batch(width=130)
                made[name] = Case(S["levels"], S, S["A"])
            else:
                levels, d = load_hier(name)
                made[name] = Case(levels, d, perturbed(d, 0.05 if name in PERTURBED else 0.0, real=PERTURBED.get(name, True)))
        return made[name]

    yield get
    for c in made.values():
        c.M.close()


def colerr(x, xo):
    return 0.0 if not xo.any() and not x.any() else relerr(x, xo)


def check_gmres(C, B, X, fl, it, kw, fates=None):
    worst = 0.0
    for c in range(B.shape[1]):
        xo, fo, io = C.gmres(B[:, c], **kw)
        assert (int(fl[c]), int(it[c])) == (fo, io), (c, fates and fates[c])
        worst = max(worst, colerr(X[:, c], xo))
        assert colerr(X[:, c], xo) <= TOL_GM, (c, fates and fates[c])
    return worst


def check_fates(B, X, fl, it, fates):
    for c, f in enumerate(fates):
        if f == "zero":
            assert (int(fl[c]), int(it[c])) == (0, 0) and not X[:, c].any()
        if f in SCALED_COPY_OF:  # a copy scaled by 1e-30 / 1e+30 behaves like its original
            o = fates.index(SCALED_COPY_OF[f])
            assert (int(fl[c]), int(it[c])) == (int(fl[o]), int(it[o])), f


# ---- a. widths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 3, 33, 48, 63, 64, 65, 129])
@pytest.mark.parametrize("name", list(PERTURBED))
def test_gmres_widths(cases, name, width):
    C = cases(name)
    B, fates = C.batch(width)
    X, fl, it = C.M.gmres(B, **GM)
    worst = check_gmres(C, B, X, fl, it, GM, fates)
    check_fates(B, X, fl, it, fates)
    if width >= 33:  # the fates really differ inside the tile: two outer cycles, three finishing steps in one of them
        where = [finishing_steps(int(it[c]), GM["restart"]) for c in range(min(width, 64)) if fates[c] != "zero"]
        assert len({o for o, _ in where}) >= 2 and max(len({j for o, j in where if o == cyc}) for cyc in (0, 1)) >= 3
    print("gmres %s width %d: largest relerr %.2e" % (name, width, worst))


@pytest.mark.parametrize("width", [33, 64, 70])
@pytest.mark.parametrize("name", list(PERTURBED))
def test_fgmres_widths(cases, name, width):
    C = cases(name)
    B, fates = C.batch(width)
    X, fl, it, mv = C.M.fgmres(B, **FGM)
    worst = 0.0
    for c in range(width):
        xo, fo, io, mo = C.fgmres(B[:, c], **FGM)
        assert (int(fl[c]), int(it[c]), int(mv[c])) == (fo, io, mo), (c, fates[c])
        worst = max(worst, colerr(X[:, c], xo))
        assert colerr(X[:, c], xo) <= TOL_GM, (c, fates[c])
    check_fates(B, X, fl, it, fates)
    assert len({int(v) for v in it}) >= 3
    print("fgmres %s width %d: largest relerr %.2e" % (name, width, worst))


def check_ir(C, B, X, N, betas=None, its=None, fls=None, trans=False, fates=None):
    worst = 0.0
    for c in range(B.shape[1]):
        xo, io, fo, hist = C.ir(B[:, c], N, betas, trans)
        if betas is not None:
            # (the restated ratios are not within 1e-6 of a beta: device rounding cannot change the fate)
            assert all(abs(r / bt - 1.0) > 1e-6 for r in hist for bt in betas), (c, hist)
            assert (int(its[c]), int(fls[c])) == (io, fo), (c, fates and fates[c], hist)
        worst = max(worst, colerr(X[:, c], xo))
        assert colerr(X[:, c], xo) <= TOL_IR, (c, fates and fates[c])
    return worst


@pytest.mark.parametrize("width", [5, 63, 64, 65, 130])
@pytest.mark.parametrize("name", list(PERTURBED))
def test_refinement_widths(cases, name, width):
    C = cases(name)
    B, fates = C.batch(width)
    X = C.M.hifir(B, IR_N)
    w1 = check_ir(C, B, X, IR_N, fates=fates)
    Xb, its, fls = C.M.hifir(B, IR_BOUNDED["nirs"], betas=IR_BOUNDED["betas"])
    w2 = check_ir(C, B, Xb, IR_BOUNDED["nirs"], IR_BOUNDED["betas"], its, fls, fates=fates)
    for c, f in enumerate(fates):
        if f == "zero":
            assert (int(its[c]), int(fls[c])) == (0, 0) and not Xb[:, c].any() and not X[:, c].any()
        if f in SCALED_COPY_OF:
            o = fates.index(SCALED_COPY_OF[f])
            assert (int(its[c]), int(fls[c])) == (int(its[o]), int(fls[o]))
    if name == "cd2d_48" and width >= 63:
        assert {-1, 0, 1} <= {int(v) for v in fls}  # sweeps exhausted and divergence (the fixture's b) in one batch
    print("refinement %s width %d: largest relerr %.2e (N = 4), %.2e (bounded)" % (name, width, w1, w2))


@pytest.mark.parametrize("width", [5, 64, 65, 130])
def test_bounded_refinement_five_fates(cases, width):
    # zero, converged after 2 and after 3 .. 6 sweeps, sweeps exhausted, diverged at once: frozen columns (k_masked_add)
    # next to running ones, on both sides of column 64
    C = cases("irmix")
    S = C.d
    B = np.ascontiguousarray(S["B"][:, :width])
    X, its, fls = C.M.hifir(B, S["nirs"], betas=S["betas"])
    assert [(int(i), int(f)) for i, f in zip(its, fls)] == S["expected"][:width]
    check_ir(C, B, X, S["nirs"], S["betas"], its, fls, fates=S["fates"])


@pytest.mark.parametrize("width", [5, 130])
def test_bounded_refinement_five_fates_device_entry(cases, width):
    torch = pytest.importorskip("torch")
    C = cases("irmix")
    S = C.d
    B = np.ascontiguousarray(S["B"][:, :width])
    X, its, fls = C.M.hifir(B, S["nirs"], betas=S["betas"])
    Xd, its2, fls2 = C.M.hifir(torch.from_numpy(B).cuda(), S["nirs"], betas=S["betas"])
    assert np.array_equal(its2, its) and np.array_equal(fls2, fls) and np.array_equal(Xd.cpu().numpy(), X)


# ---- b. a column does not see its neighbours ---------------------------------------------------------------------------------
NB_GM = dict(restart=12, rtol=1e-9, maxit=40)
NB_FGM = dict(restart=6, rtol=1e-9, maxit=25)  # (not a multiple of the restart: a NaN column meets the maxit test)


def _solve(M, driver, B):
    """-> (X, status arrays ...) of one driver"""
    if driver == "gmres":
        return M.gmres(B, **NB_GM)
    if driver == "fgmres":
        return M.fgmres(B, **NB_FGM)
    if driver == "ir":
        return (M.hifir(B, IR_N),)
    return M.hifir(B, IR_BOUNDED["nirs"], betas=IR_BOUNDED["betas"])


@pytest.mark.parametrize("driver", ["gmres", "fgmres", "ir", "ir_bounded"])
@pytest.mark.parametrize("name,width", [("cd2d_48", 33), ("cd2d_48", 64), ("young1c", 33)])
def test_column_does_not_see_its_neighbours(cases, name, width, driver):
    # every reduction is per column with rows-per-pass a function of nc alone, and the apply's bits do not depend on the
    # other columns: the bits of a column are those it has next to zeros, NaN, inf and 1e300
    C = cases(name)
    B, fates = C.batch(width)
    base = _solve(C.M, driver, B)
    for keep in sorted({0, 32, width - 1}):
        assert fates[keep] == "hard"
        for how in ("zero", "nan", "inf", "big"):
            out = _solve(C.M, driver, neighbours_replaced(B, keep, how))
            for got, want in zip(out, base):
                assert np.array_equal(got[..., keep], want[..., keep]), (keep, how)
            other = 1
            if how == "nan" and driver == "gmres":  # a NaN column passes no test but maxit
                assert (int(out[1][other]), int(out[2][other])) == (2, NB_GM["maxit"])
            if how == "nan" and driver == "fgmres":
                assert (int(out[1][other]), int(out[2][other])) == (2, NB_FGM["maxit"])
            if how == "nan" and driver == "ir_bounded":
                assert (int(out[1][other]), int(out[2][other])) == (IR_BOUNDED["nirs"], -1)
            if how == "zero":
                assert not out[0][:, other].any()
    if driver == "gmres":
        assert int(base[1][0]) == 0 and int(base[2][0]) > NB_GM["restart"]  # the kept column crosses a restart


# ---- c. stopping rules -------------------------------------------------------------------------------------------------------
def test_identity_hierarchy_is_exact(cases):
    C = cases("stag")
    n = C.A.shape[0]
    assert np.array_equal(C.M.solve_mrhs(np.eye(n)), np.eye(n))


@pytest.mark.parametrize("width", [1, 5, 33])
def test_stagnation(cases, width):
    # flag 1 (gmres.hpp:90-93), at once, after one step and with the residual ratio equal to the bound (>=, not >), alone and
    # among columns that converge in 1, 2 and 3 steps
    C = cases("stag")
    cols, exp = C.d["columns"], C.d["expected"]
    kw = dict(restart=12, rtol=1e-9, maxit=40)
    if width == 1:
        for nm in ("now", "later", "edge"):
            x, fl, it = C.M.gmres(cols[nm], **kw)
            xo, fo, io = C.gmres(cols[nm], **kw)
            assert (fl, it) == (fo, io) == exp[nm] and colerr(x, xo) <= TOL_GM
        return
    names = [nm for nm in cols if nm != "edge"]
    pick = [names[(3 * c) % 5] for c in range(width)]  # now, conv2, later, conv3, conv1, ...
    pick[width - 1] = "edge"
    B = np.stack([cols[nm] * (1.0 if nm == "edge" else 1.0 + c) for c, nm in enumerate(pick)], axis=1)
    X, fl, it = C.M.gmres(B, **kw)
    assert [(int(f), int(i)) for f, i in zip(fl, it)] == [exp[nm] for nm in pick]
    check_gmres(C, B, X, fl, it, kw, pick)
    assert {1, 0} == {int(f) for f in fl}
    X, fl, it, mv = C.M.fgmres(B, **kw)
    assert [(int(f), int(i)) for f, i in zip(fl, it)] == [exp[nm] for nm in pick]
    for c in range(width):
        xo, fo, io, mo = C.fgmres(B[:, c], **kw)
        assert (int(fl[c]), int(it[c]), int(mv[c])) == (fo, io, mo), (c, pick[c])
        assert colerr(X[:, c], xo) <= TOL_GM, (c, pick[c])


def test_multiple_of_restart_returns_flag_0(cases):
    name, restart, maxit, rtol = QUIRK
    C = cases(name)
    B, fates = C.batch(5)
    B = np.column_stack([B, C.d["b"]])
    kw = dict(restart=restart, rtol=rtol, maxit=maxit)
    X, fl, it = C.M.gmres(B, **kw)
    check_gmres(C, B, X, fl, it, kw)
    assert (int(fl[5]), int(it[5])) == (0, maxit)
    assert np.linalg.norm(C.A @ X[:, 5] - B[:, 5]) / np.linalg.norm(B[:, 5]) > 100 * rtol
    X, fl, it, mv = C.M.fgmres(B, **kw)
    for c in range(6):
        xo, fo, io, mo = C.fgmres(B[:, c], **kw)
        assert (int(fl[c]), int(it[c]), int(mv[c])) == (fo, io, mo) and colerr(X[:, c], xo) <= TOL_GM


@pytest.mark.parametrize("restart,maxit", [(12, 1), (30, 7), (9, 10), (3, 2)])
def test_maxit_below_and_beside_restart(cases, restart, maxit):
    # maxit = 1, restart > maxit, maxit = restart + 1: flag 2 with iters == maxit wherever the restatement says so
    C = cases("cd2d_48")
    B, fates = C.batch(5)
    kw = dict(restart=restart, rtol=1e-9, maxit=maxit)
    X, fl, it = C.M.gmres(B, **kw)
    check_gmres(C, B, X, fl, it, kw, fates)
    assert (int(fl[0]), int(it[0])) == (2, maxit)
    assert (int(fl[1]), int(it[1])) == (0, 0)


# ---- d. restart ladder -------------------------------------------------------------------------------------------------------
# the restated GMRES(r) needs 12 ... 23 iterations on these five columns for every r of the ladder (printed below); maxit is an
# order of magnitude above, so that every column converges and none comes near the maxit test
LADDER_MAXIT = 300


@pytest.mark.parametrize("restart", [1, 2, 3, 4, 5, 8, 9])
def test_restart_ladder(cases, restart):
    # kGmBlock = 4: block sizes mn = 1 .. 4 in k_gm_block / k_gm_hblock, one and two blocks and a remainder; restart 1 has
    # no Q(:, 1) and a 1 x 1 R
    C = cases("cd2d_48")
    B, fates = C.batch(5)
    kw = dict(restart=restart, rtol=1e-8, maxit=LADDER_MAXIT)
    X, fl, it = C.M.gmres(B, **kw)
    worst = check_gmres(C, B, X, fl, it, kw, fates)
    check_fates(B, X, fl, it, fates)
    assert int(fl[0]) == 0 and int(it[0]) > restart
    print("gmres restart %d: iterations %s, largest relerr %.2e" % (restart, [int(v) for v in it], worst))


@pytest.mark.parametrize("restart", [1, 30])
def test_exact_preconditioner_takes_one_step(cases, restart):
    # p2d_5: M^-1 is A^-1 to rounding, the first step converges and leaves a breakdown-sized |v|; x and (flag, iters) only
    C = cases("p2d_5")
    n = C.A.shape[0]
    rng = np.random.default_rng(9)
    B = np.column_stack([C.d["b"], rng.uniform(-1, 1, (n, 3)), np.zeros(n)])
    kw = dict(restart=restart, rtol=1e-10, maxit=30)
    X, fl, it = C.M.gmres(B, **kw)
    check_gmres(C, B, X, fl, it, kw)
    assert [(int(f), int(i)) for f, i in zip(fl, it)] == [(0, 1)] * 4 + [(0, 0)]


# ---- e. strides ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,stride", [(5, 9), (70, 80)])
def test_strided_device_blocks(cases, width, stride):
    # the device entries with ldb, ldx > nrhs: same bits as the contiguous call, the padding keeps its fill value
    torch = pytest.importorskip("torch")
    C = cases("p2d_30")
    B, fates = C.batch(width)
    n = B.shape[0]
    Bd = torch.from_numpy(B).cuda()
    wide = torch.full((n, stride), 7.25, dtype=Bd.dtype, device="cuda")
    wide[:, 2:2 + width] = Bd
    Bv = wide[:, 2:2 + width]
    assert Bv.stride(0) == stride
    lib, M = hifir_amd.lib(), C.M

    def strided(call):
        out = torch.full((n, stride), -3.5, dtype=Bd.dtype, device="cuda")
        call(Bv, out[:, 1:1 + width])
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[:, :1] == -3.5).all() and (o[:, 1 + width:] == -3.5).all()
        return o[:, 1:1 + width]

    def p(a):
        return None if a is None else a.ctypes.data

    fl, it = np.zeros(width, dtype=np.int32), np.zeros(width, dtype=np.int32)
    Xs = strided(lambda b, x: hifir_amd.hif._check(lib.hifamd_gmres_batch_dev(
        M._h, b.data_ptr(), b.stride(0), x.data_ptr(), x.stride(0), width, GM["restart"], GM["rtol"], GM["maxit"], 0, p(fl), p(it))))
    Xc, flc, itc = M.gmres(Bd, **GM)
    assert np.array_equal(Xs, Xc.cpu().numpy()) and np.array_equal(fl, flc) and np.array_equal(it, itc)
    check_gmres(C, B, Xs, fl, it, GM, fates)
    for nirs, betas in ((IR_N, None), (IR_BOUNDED["nirs"], IR_BOUNDED["betas"])):
        bt = None if betas is None else np.ascontiguousarray(betas, dtype=np.float64)
        st = np.zeros(2 * width, dtype=np.int32)  # (iterations, flag) per column
        Xs = strided(lambda b, x: hifir_amd.hif._check(lib.hifamd_hifir_batch_dev(
            M._h, b.data_ptr(), b.stride(0), x.data_ptr(), x.stride(0), width, nirs, p(bt), -1, p(st))))
        ref = M.hifir(Bd, nirs, betas=betas)
        Xc = ref if betas is None else ref[0]
        assert np.array_equal(Xs, Xc.cpu().numpy())
        if betas is not None:
            assert np.array_equal(st[0::2], ref[1]) and np.array_equal(st[1::2], ref[2])
            check_ir(C, B, Xs, nirs, betas, st[0::2], st[1::2], fates=fates)
    w = wide.cpu().numpy()
    assert (w[:, :2] == 7.25).all() and (w[:, 2 + width:] == 7.25).all() and np.array_equal(w[:, 2:2 + width], B)


# ---- f. no trace between calls -----------------------------------------------------------------------------------------------
def test_no_trace_between_calls(cases):
    # gm_Q, gm_Z, ir_part, gm_red and gm_hb are never cleared and ir_part serves GMRES and the refinement's norms: a solve's
    # bits must not depend on what ran before it on the handle
    C = cases("cd2d_48")
    M = C.M
    B70, _ = C.batch(70)
    B3, _ = C.batch(3)
    B33, _ = C.batch(33)
    B65, _ = C.batch(65)
    first = M.gmres(B70, restart=30, rtol=1e-9, maxit=90)
    ir_first = (M.hifir(B65, IR_N),) + M.hifir(B65, IR_BOUNDED["nirs"], betas=IR_BOUNDED["betas"])
    M.gmres(B3, restart=5, rtol=1e-9, maxit=100)
    M.fgmres(B33, **FGM)
    M.hifir(B65, IR_BOUNDED["nirs"], betas=IR_BOUNDED["betas"])
    M.gmres(neighbours_replaced(B33, 0, "nan"), **NB_GM)
    again = M.gmres(B70, restart=30, rtol=1e-9, maxit=90)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    assert not first[1].any()
    # the refinement around a GMRES call (the last call above): ir_part held GMRES's partial sums
    ir_again = (M.hifir(B65, IR_N),) + M.hifir(B65, IR_BOUNDED["nirs"], betas=IR_BOUNDED["betas"])
    for a, b in zip(ir_first, ir_again):
        assert np.array_equal(a, b)


# ---- g. transposed refinement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [5, 65])
@pytest.mark.parametrize("name", list(PERTURBED))
def test_transposed_refinement(cases, name, width):
    C = cases(name)
    B, fates = C.batch(width)
    X = C.M.hifir(B, IR_N, trans=True)
    w1 = check_ir(C, B, X, IR_N, trans=True, fates=fates)
    Xb, its, fls = C.M.hifir(B, IR_BOUNDED["nirs"], betas=IR_BOUNDED["betas"], trans=True)
    w2 = check_ir(C, B, Xb, IR_BOUNDED["nirs"], IR_BOUNDED["betas"], its, fls, trans=True, fates=fates)
    z = fates.index("zero")
    assert (int(its[z]), int(fls[z])) == (0, 0) and not Xb[:, z].any()
    print("transposed refinement %s width %d: largest relerr %.2e (N = 4), %.2e (bounded)" % (name, width, w1, w2))
