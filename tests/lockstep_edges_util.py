"""Inputs and restatements for the batch, fate and stopping edges of the three lock-step solvers that sit on the Krylov
scaffold: PCG, BiCGSTAB and symmetric QMR (test_lockstep_edges_host.py pins everything here on the CPU,
test_gpu_lockstep_edges.py holds the drivers against it).  numpy / scipy only.

The restatements are column by column around a solve(r) callback (M^{-1} r; an object with a .solve method serves as
well), in the order of operations of Engine::pcg_tile / bicgstab_tile / sqmr_tile.  trace (a list) receives one dict per
column: mode and step at which the column stopped, numbered as the comments of k_cg_finish / k_bs_finish / k_qm_finish
number them (step is the kernel's k), `ratios` = every residual ratio a stopping test looked at, and `scalars` =
(name, k, value / scale) of every scalar a breakdown test looked at, each divided by its natural scale."""
import numpy as np
import scipy.sparse as sp

from krylov_edges_util import EASY_POWER, SCALED_COPY_OF, csr_of, mixed_batch, mixed_fates, neighbours_replaced, perturbed  # noqa: F401

MARGIN = 1.02  # (test_sqmr_host.MARGIN; the host test asserts they agree)


def _solver(solve):
    return getattr(solve, "solve", solve)


def _norm2(v):
    return float(np.vdot(v, v).real)


def _over(v, scale):
    """v / scale for the trace; a zero or non-finite scale gives v itself (the column is breaking down anyway)"""
    with np.errstate(all="ignore"):
        return v / scale if (scale != 0 and np.isfinite(scale)) else v


class _Trace:
    def __init__(self, trace):
        self.t = None
        if trace is not None:
            self.t = dict(mode=0, step=0, ratios=[], scalars=[])
            trace.append(self.t)

    def ratio(self, v):
        if self.t is not None:
            self.t["ratios"].append(float(v))

    def scalar(self, name, k, v, scale):
        if self.t is not None:
            self.t["scalars"].append((name, k, _over(v, scale)))

    def stop(self, mode, step):
        if self.t is not None:
            self.t["mode"], self.t["step"] = mode, step


def _pcg_bad(v):
    return not (np.isfinite(v) and np.real(v) > 0.0)


def pcg_restated(solve, A, B, rtol, maxit, trace=None):
    """Column by column: x0 = 0, r = b, z = M^{-1} r, p = z, rho = r^H z; per step q = A p, alpha = rho / p^H q,
    x += alpha p, r -= alpha q, stop on |r| / |b| <= rtol (flag 0) or after maxit steps (flag 2), z = M^{-1} r,
    rho' = r^H z, p = z + (rho' / rho) p.  A non-positive or non-finite p^H A p or r^H z is a breakdown (flag 1).
    trace scales: rho / |r|^2, sigma / p^H p."""
    solve = _solver(solve)
    B = B.reshape(B.shape[0], -1)
    X = np.zeros_like(B)
    flags = np.zeros(B.shape[1], dtype=np.int32)
    iters = np.zeros(B.shape[1], dtype=np.int32)
    for c in range(B.shape[1]):
        b = B[:, c]
        T = _Trace(trace)
        bn = np.linalg.norm(b)
        if bn == 0.0:
            continue
        x = np.zeros_like(b)
        r = b.copy()
        z = solve(r.copy())
        p = z.copy()
        rho = np.vdot(r, z)
        T.scalar("rho", 0, rho, _norm2(r))
        T.stop(1, 0)
        flag, it = 1, 0
        if not _pcg_bad(rho):
            for k in range(maxit):
                q = A @ p
                sigma = np.vdot(p, q)
                T.scalar("sigma", k, sigma, _norm2(p))
                if _pcg_bad(sigma):
                    flag, it = 1, k
                    T.stop(2, k)
                    break
                alpha = rho / sigma
                x = x + alpha * p
                r = r - alpha * q
                T.ratio(np.linalg.norm(r) / bn)
                if np.linalg.norm(r) / bn <= rtol:
                    flag, it = 0, k + 1
                    T.stop(3, k)
                    break
                if k + 1 >= maxit:
                    flag, it = 2, maxit
                    T.stop(3, k)
                    break
                z = solve(r.copy())
                rho1 = np.vdot(r, z)
                T.scalar("rho", k + 1, rho1, _norm2(r))
                if _pcg_bad(rho1):
                    flag, it = 1, k + 1
                    T.stop(4, k)
                    break
                p = z + (rho1 / rho) * p
                rho = rho1
        X[:, c], flags[c], iters[c] = x, flag, it
    return X, flags, iters


def _bad(v):
    """a breakdown value of BiCGSTAB and symmetric QMR: exactly zero or not finite (no sign test)"""
    return v == 0 or not np.isfinite(v)


def sqmr_restated(solve, A, B, rtol, maxit, hist=None, trace=None):
    """Column by column, x0 = 0 (solve(r) is M^{-1} r, filtered where the handle filters it; B is P b then):
    r = s = b, tau = |b|, theta = 0, d = g = 0, z = M^{-1} r, rho = r^H z, p = z; per iteration q = A p, sigma = p^H q,
    alpha = rho / sigma, r -= alpha q, theta' = |r| / tau, c2 = 1 / (1 + theta'^2), tau = tau theta' sqrt(c2),
    eta = c2 theta^2, zeta = c2 alpha, theta = theta', d = eta d + zeta p, g = eta g + zeta q, x += d, s -= g, stop on
    |s| / |b| <= rtol (flag 0) or after maxit iterations (flag 2), z = M^{-1} r, rho' = r^H z, p = z + (rho' / rho) p.
    rho or sigma exactly zero or not finite is a breakdown (flag 1).  hist (a list) gets one list per column: |s| / |b|
    after every iteration.  trace scales: rho / |r|^2, sigma / p^H p."""
    solve = _solver(solve)
    B = B.reshape(B.shape[0], -1)
    X = np.zeros_like(B)
    flags = np.zeros(B.shape[1], dtype=np.int32)
    iters = np.zeros(B.shape[1], dtype=np.int32)
    for c in range(B.shape[1]):
        b = B[:, c]
        h = []
        if hist is not None:
            hist.append(h)
        T = _Trace(trace)
        bn = np.linalg.norm(b)
        if bn == 0.0:
            continue
        x = np.zeros_like(b)
        r, s = b.copy(), b.copy()
        d, g = np.zeros_like(b), np.zeros_like(b)
        tau, theta = bn, 0.0
        z = solve(r.copy())
        p = z.copy()
        rho = np.vdot(r, z)
        T.scalar("rho", 0, rho, _norm2(r))
        T.stop(1, 0)
        flag, it = 1, 0
        if not _bad(rho):
            for k in range(maxit):
                q = A @ p
                sigma = np.vdot(p, q)
                T.scalar("sigma", k, sigma, _norm2(p))
                if _bad(sigma):
                    flag, it = 1, k
                    T.stop(2, k)
                    break
                alpha = rho / sigma
                r = r - alpha * q
                th = np.linalg.norm(r) / tau
                c2 = 1.0 / (1.0 + th * th)
                tau = tau * th * np.sqrt(c2)
                eta, zeta = c2 * theta * theta, c2 * alpha
                theta = th
                d = eta * d + zeta * p
                g = eta * g + zeta * q
                x = x + d
                s = s - g
                h.append(float(np.linalg.norm(s) / bn))
                T.ratio(h[-1])
                if h[-1] <= rtol:
                    flag, it = 0, k + 1
                    T.stop(4, k)
                    break
                if k + 1 >= maxit:
                    flag, it = 2, maxit
                    T.stop(4, k)
                    break
                z = solve(r.copy())
                rho1 = np.vdot(r, z)
                T.scalar("rho", k + 1, rho1, _norm2(r))
                if _bad(rho1):
                    flag, it = 1, k + 1
                    T.stop(5, k)
                    break
                p = z + (rho1 / rho) * p
                rho = rho1
        X[:, c], flags[c], iters[c] = x, flag, it
    return X, flags, iters


def bicgstab_restated(solve, A, B, rtol, maxit, nsp=False, trace=None):
    """Column by column, verbatim: r = b, r^ = b, rho = (r^, r), p = r; loop: y = M^{-1} p, v = A y (a step),
    alpha = rho / (r^, v), x += alpha y, r -= alpha v, test; y = M^{-1} r, t = A y (a step), omega = (t, r) / (t, t),
    x += omega y, r -= omega t, test; rho' = (r^, r), beta = (rho' / rho)(alpha / omega), rho = rho',
    p = r + beta (p - omega v).  Test: ||r|| / ||b|| <= rtol -> flag 0, else steps == maxit -> flag 2.  (r^, v), (t, t),
    omega, rho' or the initial rho exactly zero or not finite: flag 1.  nsp: every M^{-1} apply loses its mean.
    trace scales: (r^, v) / |r^||v|, (t, t) / |r|^2, omega |t| / |r| (the cosine of t and r), rho' / |r^||r|; its step is the
    kernel's k (steps 2k + 1 and 2k + 2)."""
    solve = _solver(solve)
    B = B.reshape(B.shape[0], -1)
    X = np.zeros_like(B)
    flags = np.zeros(B.shape[1], dtype=np.int32)
    iters = np.zeros(B.shape[1], dtype=np.int32)

    def prec(u):
        y = solve(u.copy())
        return y - y.mean() if nsp else y

    for c in range(B.shape[1]):
        b = B[:, c]
        T = _Trace(trace)
        bn = np.linalg.norm(b)
        if bn == 0.0:
            continue
        x = np.zeros_like(b)
        r = b.copy()
        rh = b.copy()
        rho = np.vdot(rh, r)
        p = r.copy()
        flag, steps = 1, 0
        k = 0
        T.stop(0, 0)
        while not _bad(rho):
            y = prec(p)
            v = A @ y
            steps += 1
            rv = np.vdot(rh, v)
            T.scalar("rv", k, rv, bn * np.linalg.norm(v))
            if _bad(rv):
                T.stop(1, k)
                break
            alpha = rho / rv
            x = x + alpha * y
            r = r - alpha * v
            T.ratio(np.linalg.norm(r) / bn)
            if np.linalg.norm(r) / bn <= rtol:
                flag = 0
                T.stop(2, k)
                break
            if steps >= maxit:
                flag = 2
                T.stop(2, k)
                break
            y = prec(r)
            t = A @ y
            steps += 1
            tt = np.vdot(t, t)
            T.scalar("tt", k, tt, _norm2(r))
            if _bad(tt):
                T.stop(3, k)
                break
            omega = np.vdot(t, r) / tt
            T.scalar("omega", k, omega, np.linalg.norm(r) / np.sqrt(tt.real))
            if _bad(omega):
                T.stop(3, k)
                break
            x = x + omega * y
            r = r - omega * t
            T.ratio(np.linalg.norm(r) / bn)
            if np.linalg.norm(r) / bn <= rtol:
                flag = 0
                T.stop(4, k)
                break
            if steps >= maxit:
                flag = 2
                T.stop(4, k)
                break
            rho1 = np.vdot(rh, r)
            T.scalar("rho", k + 1, rho1, bn * np.linalg.norm(r))
            if _bad(rho1):
                T.stop(4, k)
                break
            beta = (rho1 / rho) * (alpha / omega)
            rho = rho1
            p = r + beta * (p - omega * v)
            k += 1
        X[:, c], flags[c], iters[c] = x, flag, steps
    return X, flags, iters


RESTATED = {"pcg": pcg_restated, "sqmr": sqmr_restated, "bicgstab": bicgstab_restated}


# ---- (a) columns of different fate on real hierarchies -------------------------------------------------------------------
# (solver, fixture) -> how the matrix is made and run.  amp: krylov_edges_util.perturbed (0: the fixture's own matrix);
# spd: the random diagonal is added with its absolute value, so that a positive definite matrix stays one; a name ending in
# _z: the fixture under the diagonal unitary similarity of test_gpu_pcg._phase_similarity (a complex Hermitian pair; the
# project's complex is_symm fixture herm_24_symm is complex SYMMETRIC, F = E^T, and PCG refuses it); proj: the fixture's
# null-space basis is installed and the restatement runs with P M^{-1} and P b.  Unperturbed hierarchies converge in 1 .. 4
# steps on p2d_32_symm, cd2d_48 and young1c, too few to separate four fates.
CONFIG = {
    ("pcg", "p2d_32_symm"): dict(amp=0.05, real=True, spd=True, rtol=1e-9, widths=(1, 3, 33, 63, 64, 65, 129)),
    ("pcg", "p2d_32_symm_z"): dict(amp=0.05, real=True, spd=True, rtol=1e-9, widths=(33, 65)),
    ("sqmr", "shift2d_32_symm"): dict(amp=0.0, real=True, rtol=1e-8, widths=(1, 3, 33, 63, 64, 65, 129)),
    ("sqmr", "kktr_24_symm"): dict(amp=0.0, real=True, rtol=1e-10, widths=(1, 3, 33, 63, 64, 65, 129)),
    ("bicgstab", "cd2d_48"): dict(amp=0.05, real=True, rtol=1e-10, widths=(1, 3, 33, 63, 64, 65, 129)),
    ("bicgstab", "young1c"): dict(amp=0.05, real=False, rtol=1e-9, widths=(33, 65)),
    ("pcg", "neu2d_32_symm"): dict(amp=0.0, real=True, rtol=1e-9, widths=(33, 65), proj=True),
    ("sqmr", "neu2d_32_symm"): dict(amp=0.0, real=True, rtol=1e-9, widths=(33, 65), proj=True),
}
MAXIT = 300
EXTRA_WIDTHS = (5, 70)  # the strided-block and the no-trace tests (unprojected pairs)
BATCH_SEED = 11  # (a pair's own `seed` where this one's first column is not Pair.stable)
# random columns (seed 1000 + j) that the host test found too close to a decision on that pair -- not Pair.stable, or an
# iteration count that another fate of the batch has -- are passed over: the j-th hard column of every
# batch is the j-th seed that is left
SKIP_SEEDS = {
    ("sqmr", "kktr_24_symm"): (1013,),
    ("bicgstab", "cd2d_48"): (1005, 1008, 1011, 1012, 1013, 1015, 1016, 1018, 1024, 1025, 1026, 1028, 1030, 1032),
}
HARD_PER_BATCH = 20  # a batch of 129 columns has 18 hard ones


class Filtered:
    """the oracle's apply followed by the projection P = I - Q Q^H (what a handle with a basis filter applies)"""

    def __init__(self, O, Q):
        self.O, self.Q, self.dtype = O, Q, O.dtype

    def proj(self, x):
        return x - self.Q @ (self.Q.conj().T @ x)

    def solve(self, r):
        return self.proj(self.O.solve(r))


class Pair:
    """One (solver, fixture) of CONFIG: levels, data, matrix, the apply the restatement runs around, and its batches with
    their restated columns (each column restated once, whatever batch it sits in)."""

    def __init__(self, solver, name):
        from oracle import orc
        from util import load_hier

        self.solver, self.name, self.cfg = solver, name, CONFIG[solver, name]
        cfg = self.cfg
        levels, d = load_hier(name[:-2] if name.endswith("_z") else name)
        A = perturbed(d, cfg["amp"], real=cfg["real"])
        if cfg.get("spd"):
            A0 = csr_of(d)
            A = (A0 + sp.diags(np.abs((A - A0).diagonal()))).tocsr()
            A.sort_indices()
        if name.endswith("_z"):
            from test_gpu_pcg import _phase_similarity

            levels, A, _ = _phase_similarity(levels, A)
        self.levels, self.d, self.A = levels, d, A
        self.O = orc.Oracle(levels)
        self.Q = np.linalg.qr(d["V"])[0] if cfg.get("proj") else None
        self.apply = Filtered(self.O, self.Q) if cfg.get("proj") else self.O
        self.cplx = np.iscomplexobj(A.data) or self.O.dtype.kind == "c"
        self.rtol = cfg["rtol"]
        self.seeds = [s for s in range(1000, 1200) if s not in SKIP_SEEDS.get((solver, name), ())]
        self._ref, self._batches = {}, {}

    def hard(self, j):
        rng = np.random.default_rng(self.seeds[j])
        n = self.A.shape[0]
        v = rng.uniform(-1, 1, n)
        return v + 1j * rng.uniform(-1, 1, n) if self.cplx else v

    def batch(self, width):
        """mixed_batch with its hard columns but the first (the ladder's g) taken from the vetted seeds, tiny = 2^-100 times
        the first hard column and huge = 2^+100 times the first easy column.  -> (B, fates)"""
        if width not in self._batches:
            B, fates = mixed_batch(self.apply, self.d, self.A, width, self.cfg.get("seed", BATCH_SEED))
            j = 0
            for c, f in enumerate(fates):
                if f == "hard" and c > 0:
                    B[:, c] = self.hard(j)
                    j += 1
            assert j <= HARD_PER_BATCH
            for c, f in enumerate(fates):
                if f == "tiny":
                    B[:, c] = 2.0 ** -100 * B[:, fates.index("hard")]
                if f == "huge":
                    B[:, c] = 2.0 ** 100 * B[:, fates.index("easy")]
            self._batches[width] = (B, fates)
        return self._batches[width]

    def rhs(self, b):
        """what the restatement is given: b, or P b under a basis filter"""
        return b if self.Q is None else self.apply.proj(b)

    def restated(self, b, maxit=MAXIT, rtol=None):
        """-> (x, flag, iters, trace) of one column"""
        rtol = self.rtol if rtol is None else rtol
        key = (b.tobytes(), maxit, rtol)
        if key not in self._ref:
            tr = []
            X, fl, it = RESTATED[self.solver](self.apply, self.A, self.rhs(b).copy(), rtol, maxit, trace=tr)
            self._ref[key] = (X[:, 0], int(fl[0]), int(it[0]), tr[0])
        return self._ref[key]

    def noisy(self, b, seed, maxit=MAXIT):
        """the restatement with every apply's result multiplied elementwise by 1 + 2^-52 u, u uniform in [-1, 1]: what one
        rounding per element of M^{-1} r does to the column -> (x, flag, iters, trace)"""
        rng = np.random.default_rng(seed)
        solve = self.apply.solve

        def apply(r):
            y = solve(r)
            return y * (1.0 + 2.0 ** -52 * rng.uniform(-1, 1, len(y)))

        tr = []
        X, fl, it = RESTATED[self.solver](apply, self.A, self.rhs(b).copy(), self.rtol, maxit, trace=tr)
        return X[:, 0], int(fl[0]), int(it[0]), tr[0]

    def stable(self, b, maxit=MAXIT, seeds=(5, 6, 7, 8, 9, 10)):
        """the column's fate does not hang on a rounding: six noisy runs stop where the plain one does, with every decision
        outside its margin.  (The margin on the plain run alone does not see a residual that JUMPS across rtol: where rtol is
        close to what the recurrence can attain, one rounding in an apply moves the last ratios by a factor.)"""
        x, fl, it, tr = self.restated(b, maxit=maxit)
        if not decisions_ok(tr, self.rtol):
            return False
        for s in seeds:
            xs, fs, its, ts = self.noisy(b, s, maxit)
            if (fs, its) != (fl, it) or not decisions_ok(ts, self.rtol):
                return False
        return True

    def sensitivity(self, b, seed=5):
        """relative difference of x between the plain and a noisy restatement"""
        x = self.restated(b)[0]
        nx = np.linalg.norm(x)
        return 0.0 if nx == 0 else float(np.linalg.norm(self.noisy(b, seed)[0] - x) / nx)


_PAIRS = {}


def pair(solver, name):
    if (solver, name) not in _PAIRS:
        _PAIRS[solver, name] = Pair(solver, name)
    return _PAIRS[solver, name]


def kind_of(fate):
    """the fate whose tolerance a column takes: a scaled copy takes its original's"""
    return SCALED_COPY_OF.get(fate, fate)


def decisions_ok(trace, rtol, broke_down=False):
    """every compared residual ratio is outside [rtol / MARGIN, rtol MARGIN] and, for a column that does not break down,
    every tested scalar is at least 1e-6 of its scale from zero"""
    if any(rtol / MARGIN <= v <= rtol * MARGIN for v in trace["ratios"]):
        return False
    return broke_down or all(abs(v) >= 1e-6 for _, _, v in trace["scalars"])


# ---- (b) exact fates on a diagonal hierarchy -----------------------------------------------------------------------------
def diagonal_levels(sign):
    """One level with m = n, empty L / U / E / F, identity permutations, s = t = 1, d = sign (+-1) and no dense level:
    M^{-1} = diag(sign) exactly, and Hermitian."""
    n = len(sign)
    lv = dict(m=n, n=n)
    for k, ncols in (("L", n), ("U", n), ("E", n), ("F", 0)):  # empty CCS blocks (E: 0 x n, F: n x 0)
        lv[k + "_colptr"], lv[k + "_rowind"], lv[k + "_vals"] = np.zeros(ncols + 1, np.int64), np.zeros(0, np.int32), np.zeros(0)
    lv["d"], lv["s"], lv["t"] = np.asarray(sign, dtype=np.float64), np.ones(n), np.ones(n)
    for k in ("p", "q", "p_inv", "q_inv"):
        lv[k] = np.arange(n, dtype=np.int32)
    return [lv]


def _sym(m, upper):
    """the symmetric m x m matrix with the upper triangle `upper`, row by row"""
    S = np.zeros((m, m))
    S[np.triu_indices(m)] = upper
    return S + np.triu(S, 1).T


# name -> (A block, the signs of M^{-1} on it, b on it, (flag, iterations), (mode, step) of the finishing kernel).
# Small integers: every sign decision of PCG has its scalar at 0.3 ... 4 times its scale, and every exact zero of symmetric
# QMR and BiCGSTAB comes out of dyadic rationals of a few bits (found by a search in rational arithmetic that kept only
# such cases), so that it is a zero in floating point under ANY order of summation.
PCG_FATES = {
    "conv1": (np.diag([1.0, 1]), (1, 1), (1, 1), (0, 1), (3, 0)),
    "conv2": (np.diag([1.0, 2]), (1, 1), (1, 1), (0, 2), (3, 1)),
    "conv3": (np.diag([1.0, 2, 3]), (1, 1, 1), (1, 1, 1), (0, 3), (3, 2)),
    "conv4": (np.diag([1.0, 2, 3, 4]), (1, 1, 1, 1), (1, 1, 1, 1), (0, 4), (3, 3)),
    "rho0": (np.diag([1.0, 1]), (1, -1), (1, 2), (1, 0), (1, 0)),          # r^H M^-1 r = 1 - 4
    "sigma0": (np.diag([1.0, -2]), (1, 1), (1, 1), (1, 0), (2, 0)),        # p^H A p = 1 - 2
    "sigma1": (np.diag([1.0, -2]), (1, 1), (2, 1), (1, 1), (2, 1)),
    "sigma2": (np.diag([-1.0, 1, 3]), (1, 1, 1), (1, 3, 2), (1, 2), (2, 2)),
    "rho1": (np.diag([1.0, 1]), (1, -1), (2, 1), (1, 1), (4, 0)),
    "rho2": (np.diag([1.0, 1, 4]), (1, -1, 1), (3, 1, 2), (1, 2), (4, 1)),
    "rho3": (np.diag([1.0, 2, -3, 4]), (1, 1, -1, 1), (1, 3, 1, 1), (1, 3), (4, 2)),
}
SQMR_FATES = {
    "conv1": (np.diag([1.0, 1]), (1, 1), (1, 1), (0, 1), (4, 0)),
    "conv2": (np.diag([1.0, -2]), (1, 1), (2, 1), (0, 2), (4, 1)),
    "conv3": (np.diag([1.0, -2, 3]), (1, 1, 1), (1, 1, 1), (0, 3), (4, 2)),
    "rho0": (np.diag([1.0, 1]), (1, -1), (1, 1), (1, 0), (1, 0)),          # r^H M^-1 r = 1 - 1
    "sigma0": (np.diag([1.0, -1]), (1, 1), (1, 1), (1, 0), (2, 0)),        # p^H A p = 1 - 1
    "sigma1": (_sym(2, [-4.0, -4, -4]), (1, 1), (-3, -1), (1, 1), (2, 1)),
    "sigma2": (_sym(3, [-2.0, -2, -2, -2, -2, -1]), (1, 1, 1), (-2, 0, 0), (1, 2), (2, 2)),
    "rho1": (_sym(3, [-2.0, -2, -2, -2, -2, -2]), (1, 1, -1), (-2, -1, -2), (1, 1), (5, 0)),
}
BICGSTAB_FATES = {
    "half": (np.diag([2.0, 2]), (1, 1), (1, 3), (0, 1), (2, 0)),            # A = 2I: alpha = 1/2, r = 0 after the half step
    "skew": (np.array([[0.0, 1], [-1, 0]]), (1, 1), (1, 2), (1, 1), (1, 0)),  # (r^, v) = b^T A b = 0
    "nan": (np.diag([1.0, 1]), (1, 1), (np.nan, 1), (1, 0), (0, 0)),
    "rv1": (np.full((2, 2), -4.0), (1, 1), (-3, -1), (1, 3), (1, 1)),
    "rv2": (np.array([[-2.0, -2, -2], [-2, -2, -2], [-1, 1, -2]]), (1, 1, 1), (0, -2, 0), (1, 5), (1, 2)),
    "tt0": (np.array([[-4.0, -4], [0, 0]]), (1, 1), (-3, -3), (1, 2), (3, 0)),
    "omega0": (np.array([[-4.0, -4], [-4, 0]]), (1, 1), (-3, 0), (1, 2), (3, 0)),
    "tt1": (np.array([[-2.0, -2, -2], [-2, -2, -2], [-2, 0, -2]]), (1, 1, 1), (-2, 0, -2), (1, 4), (3, 1)),
    "omega1": (np.array([[-2.0, -2, -2], [-2, -2, -1], [1, 0, 0]]), (1, 1, 1), (-2, 0, -1), (1, 4), (3, 1)),
    "rho1": (np.array([[-2.0, -2, -2], [-2, -2, -2], [-2, 0, -1]]), (1, 1, 1), (-2, 2, 1), (1, 2), (4, 0)),
    "conv2": (np.array([[0.0, 1], [2, 1]]), (1, 1), (1, 1), (0, 2), (4, 0)),
    "conv3": (np.diag([1.0, 2]), (1, 1), (1, 1), (0, 3), (2, 1)),
    "conv4": (np.array([[0.0, 0, 1], [0, 1, 0], [1, 1, 0]]), (1, 1, 1), (1, 1, -1), (0, 4), (4, 1)),
}
EXACT_FATES = {"pcg": PCG_FATES, "sqmr": SQMR_FATES, "bicgstab": BICGSTAB_FATES}
EXACT_RTOL, EXACT_MAXIT = 1e-10, 200
HARD_ROWS = 40  # the random block of the hard column
# (flag, iterations) of the hard column, from the restatement (the host test holds them to it and to a margin)
HARD_EXPECTED = {"pcg": (0, 26), "sqmr": (0, 40), "bicgstab": (0, 37)}


class ExactCase:
    """The diagonal hierarchy of one solver: every fate on a block of rows of its own, then HARD_ROWS rows for the hard column
    (PCG: a positive diagonal 1 .. 50; symmetric QMR: the same with random signs; BiCGSTAB: that diagonal plus a dense random
    block of size 0.3), M^{-1} = +1 there."""

    def __init__(self, solver, seed=4):
        self.solver, fates = solver, EXACT_FATES[solver]
        rng = np.random.default_rng(seed)
        dg = rng.uniform(1, 50, HARD_ROWS)
        if solver == "sqmr":
            dg = dg * rng.choice([-1.0, 1.0], HARD_ROWS)
        H = np.diag(dg)
        if solver == "bicgstab":
            H = H + 0.3 * rng.uniform(-1, 1, (HARD_ROWS, HARD_ROWS))
        self.hard_b = rng.integers(1, 8, HARD_ROWS).astype(np.float64)
        blocks, sign, self.rows, at = [], [], {}, 0
        for nm, (Ab, sg, b, exp, ms) in fates.items():
            blocks.append(Ab)
            sign += list(sg)
            self.rows[nm] = slice(at, at + len(sg))
            at += len(sg)
        blocks.append(H)
        sign += [1] * HARD_ROWS
        self.rows["hard"] = slice(at, at + HARD_ROWS)
        self.sign = np.array(sign, dtype=np.float64)
        self.A = sp.csr_matrix(sp.block_diag(blocks))
        self.A.sort_indices()
        self.levels = diagonal_levels(self.sign)
        self.cycle = list(fates) + ["hard"]
        self._ref = {}

    def solve(self, r):
        return self.sign * r

    def column(self, fate):
        b = np.zeros(self.A.shape[0])
        b[self.rows[fate]] = self.hard_b if fate == "hard" else EXACT_FATES[self.solver][fate][2]
        return b

    def batch(self, width):
        """fates in turn, each column times a power of two of its own -> (B, fates)"""
        fates = [self.cycle[c % len(self.cycle)] for c in range(width)]
        B = np.stack([self.column(f) * self.scale(c) for c, f in enumerate(fates)], axis=1)
        return B, fates

    @staticmethod
    def scale(c):
        return 2.0 ** ((7 * c) % 41 - 20)

    def expected(self, fate):
        return HARD_EXPECTED[self.solver] if fate == "hard" else EXACT_FATES[self.solver][fate][3]

    def restated(self, b):
        key = b.tobytes()
        if key not in self._ref:
            tr = []
            X, fl, it = RESTATED[self.solver](self.solve, self.A, b.copy(), EXACT_RTOL, EXACT_MAXIT, trace=tr)
            self._ref[key] = (X[:, 0], int(fl[0]), int(it[0]), tr[0])
        return self._ref[key]

    def exact_x(self, fate):
        """A^{-1} b of a converged fate, on the whole row range"""
        x = np.zeros(self.A.shape[0])
        Ab, sg, b = EXACT_FATES[self.solver][fate][:3]
        x[self.rows[fate]] = np.linalg.solve(Ab, np.asarray(b, dtype=np.float64))
        return x


# ---- (c) maxit edges --------------------------------------------------------------------------------------------------------
def ladder(P, K=EASY_POWER):
    """G^k g / |G^k g|, k = 0 .. K, G = I - A M^{-1}, g the batch's column 0 (mixed_batch's ladder)"""
    v = P.batch(1)[0][:, 0]
    out = [v]
    for k in range(K):
        v = v - P.A @ P.apply.solve(v)
        v = v / np.linalg.norm(v)
        out.append(v)
    return out


# solver -> (fixture, m, three columns that need m - 1, m and m + 1 iterations (BiCGSTAB: steps; an odd m stops in the half
# step, an even one in the full step): ("pow", k) is the ladder's G^k g, ("seed", j) the j-th hard column)
MAXIT_EDGES = {
    "pcg": [("p2d_32_symm", 7, (("pow", 7), ("pow", 6), ("pow", 5)))],
    "sqmr": [("shift2d_32_symm", 11, (("pow", 2), ("pow", 1), ("pow", 0)))],
    "bicgstab": [("cd2d_48", 19, (("pow", 1), ("pow", 2), ("pow", 0))), ("cd2d_48", 20, (("pow", 2), ("pow", 0), ("seed", 0)))],
}


def maxit_columns(P, spec):
    L = ladder(P)
    return np.stack([L[k] if what == "pow" else P.hard(k) for what, k in spec], axis=1)


# ---- the tolerance on x against the restatement ------------------------------------------------------------------------------
# The measured sensitivity of every kind of column on every pair (Pair.sensitivity, the largest over the columns of that kind
# in the widest batch; "ladder": over G^k g, k = 0 .. 12, the columns of the maxit edges), rounded up to two digits.  The
# bound on |x - x_restated| / |x_restated| is 1000 times that, floored at 1e-12; hard, b and ones on an unperturbed,
# unprojected fixture at rtol 1e-6 or 1e-10 are the columns the older solver tests hold to 1e-8 and keep that.
SENS = {
    ("pcg", "p2d_32_symm"): {"hard": 6.6e-11, "easy": 5.5e-16, "b": 1.9e-10, "ones": 1.1e-10, "pow4": 7.7e-14, "pow8": 7.9e-16, "ladder": 1.7e-10},
    ("pcg", "p2d_32_symm_z"): {"hard": 9.5e-11, "easy": 3.0e-16, "b": 1.8e-10, "ones": 2.5e-12, "pow4": 1.4e-13, "pow8": 2.5e-16, "ladder": 6.9e-11},
    ("sqmr", "shift2d_32_symm"): {"hard": 1.1e-10, "easy": 4.3e-15, "b": 1.6e-10, "ones": 5.0e-13, "pow4": 4.1e-14, "pow8": 2.6e-15, "ladder": 3.6e-12},
    ("sqmr", "kktr_24_symm"): {"hard": 2.3e-16, "easy": 2.9e-16, "b": 2.2e-16, "ones": 3.0e-16, "pow4": 1.9e-16, "pow8": 2.3e-16, "ladder": 2.6e-16},
    ("bicgstab", "cd2d_48"): {"hard": 5.3e-14, "easy": 6.9e-16, "b": 6.5e-16, "ones": 5.6e-12, "pow4": 4.3e-16, "pow8": 4.0e-16, "ladder": 9.5e-11},
    ("bicgstab", "young1c"): {"hard": 1.6e-15, "easy": 1.3e-15, "b": 6.6e-16, "ones": 8.7e-16, "pow4": 9.4e-16, "pow8": 1.2e-15, "ladder": 1.6e-15},
    ("pcg", "neu2d_32_symm"): {"hard": 1.9e-15, "easy": 1.6e-15, "b": 1.6e-15, "pow4": 1.3e-15, "pow8": 6.6e-16, "ladder": 1.7e-15},
    ("sqmr", "neu2d_32_symm"): {"hard": 1.8e-15, "easy": 1.6e-15, "b": 1.5e-15, "pow4": 1.3e-15, "pow8": 6.5e-16, "ladder": 1.7e-15},
}


def tolerance(P, kind):
    if P.cfg["amp"] == 0.0 and not P.cfg.get("proj") and P.rtol in (1e-6, 1e-10) and kind in ("hard", "b", "ones"):
        return 1e-8
    return max(1000.0 * SENS[P.solver, P.name][kind], 1e-12)


def measured_sensitivities(P):
    B, fates = P.batch(max(P.cfg["widths"]))
    out = {}
    for c, f in enumerate(fates):
        if f != "zero" and P.rhs(B[:, c]).any():
            out[kind_of(f)] = max(out.get(kind_of(f), 0.0), P.sensitivity(B[:, c]))
    out["ladder"] = max(P.sensitivity(v) for v in ladder(P))
    return out
