"""Inputs and restatements for the batched IDR(s) driver (hifamd_idrs_batch / HIF.idrs): test_idrs_host.py pins everything
here on the CPU, test_gpu_idrs.py holds the device against it.  numpy / scipy only.

idrs_restated is IDR(s) with biorthogonalization (van Gijzen / Sonneveld, ACM TOMS 38(1), 2011; omega by "maintaining
convergence", kappa = 0.7) column by column around a solve(r) callback, in the order of operations of Engine::idrs_tile: the
biorthogonalization coefficients alpha and the new column of M come out of ONE product raw = P^H g and the stored columns of M
(blocked form); sequential=True is the textbook form, one inner product and one update after the other.  The trace follows
lockstep_edges_util._Trace: mode and step as k_idr_finish numbers them (step = steps completed before the one that stopped),
`ratios` = the residual ratio of every stopping test, `scalars` = M[k,k] / (|p_k| |g_k|), (t, t) / |r|^2 and
(t, r) / (|t| |r|); `cosines` = every rho the omega rule compared with kappa.

The protocol is lockstep_edges_util's: a column is used only if it is `stable` (six restatements with one-ulp noise on every
apply, and the sequential form, stop at the same step, every decision outside its margin), the bound on |x - x_restated| / |x_restated| is 1000 times the
measured sensitivity of the column's kind (floor 1e-12), and the host test holds SENS, SKIP_SEEDS and UNVETTED to what it
measures."""
import numpy as np
import scipy.sparse as sp

import lockstep_edges_util as L
from lockstep_edges_util import MARGIN, _Trace, _bad, _solver, diagonal_levels, ladder, perturbed  # noqa: F401

KAPPA = 0.7
COS_MARGIN = 1e-4  # rho / kappa stays this far (relative) from 1: the comparison moves with roundings only, it never jumps
IDRS_MAX = 8


def _run_sum(coef, vecs):
    """sum_j coef_j vecs_j, j ascending, formed before it is used (k_idr_comb / k_idr_gu)"""
    acc = coef[0] * vecs[0]
    for j in range(1, len(vecs)):
        acc = acc + coef[j] * vecs[j]
    return acc


def _forward(M, f, k):
    """c_k .. c_{s-1} by forward substitution on the lower triangle M[k:, k:] c = f[k:] (entries below k stay zero)"""
    s = len(f)
    c = np.zeros_like(f)
    with np.errstate(all="ignore"):
        for i in range(k, s):
            v = f[i]
            for l in range(k, i):
                v = v - M[i, l] * c[l]
            c[i] = v / M[i, i]
    return c


def idrs_restated(solve, A, B, P, rtol, maxit, trace=None, sequential=False):
    """-> (X, flags, steps).  P [n][s] is used as given.  Flags 0 converged / 1 breakdown (M[k,k], (t, t) or (t, r) exactly zero
    or not finite; a non-finite column: 0 steps) / 2 reached maxit; a step is one apply plus one product with A."""
    solve = _solver(solve)
    B = B.reshape(B.shape[0], -1)
    P = np.asarray(P).reshape(B.shape[0], -1)
    s = P.shape[1]
    dt = np.result_type(B.dtype, P.dtype, A.dtype, np.float64)
    X = np.zeros(B.shape, dtype=dt)
    flags = np.zeros(B.shape[1], dtype=np.int32)
    iters = np.zeros(B.shape[1], dtype=np.int32)
    pn = np.linalg.norm(P, axis=0)
    PH = P.conj().T
    for col in range(B.shape[1]):
        b = B[:, col].astype(dt)
        T = _Trace(trace)
        if T.t is not None:
            T.t["cosines"] = []
        bb = float(np.vdot(b, b).real)
        bn = np.sqrt(bb)
        if bn == 0.0:
            continue
        if not np.isfinite(bb):
            flags[col] = 1
            T.stop(0, 0)
            continue
        n = len(b)
        x = np.zeros(n, dtype=dt)
        r = b.copy()
        G = [np.zeros(n, dtype=dt) for _ in range(s)]
        U = [np.zeros(n, dtype=dt) for _ in range(s)]
        M = np.eye(s, dtype=dt)
        om = dt.type(1.0)
        rr = bb
        step, flag, it = 0, None, 0

        def tested():
            """the two tests after an update of r -> (flag, steps) or None"""
            ratio = np.sqrt(rr) / bn
            T.ratio(ratio)
            if ratio <= rtol:
                T.stop(3, step)
                return 0, step + 1
            if step + 1 >= maxit:
                T.stop(3, step)
                return 2, maxit
            return None

        with np.errstate(all="ignore"):
            while flag is None:
                f = PH @ r
                for k in range(s):
                    c = _forward(M, f, k)
                    v = r - _run_sum(c[k:], G[k:])
                    vh = solve(v.copy())
                    u = om * vh + _run_sum(c[k:], U[k:])
                    g = A @ u
                    if sequential:
                        for l in range(k):
                            al = np.vdot(P[:, l], g) / M[l, l]
                            g = g - al * G[l]
                            u = u - al * U[l]
                        for i in range(k, s):
                            M[i, k] = np.vdot(P[:, i], g)
                    else:
                        raw = PH @ g
                        al = np.zeros(k, dtype=dt)
                        for i in range(k):
                            a = raw[i]
                            for l in range(i):
                                a = a - al[l] * M[i, l]
                            al[i] = a / M[i, i]
                        for i in range(k, s):
                            m = raw[i]
                            for l in range(k):
                                m = m - al[l] * M[i, l]
                            M[i, k] = m
                        if k > 0:
                            g = g - _run_sum(al, G[:k])
                            u = u - _run_sum(al, U[:k])
                    G[k], U[k] = g, u
                    mkk = M[k, k]
                    T.scalar("mkk", step, mkk, pn[k] * np.linalg.norm(g))
                    if _bad(mkk):
                        flag, it = 1, step + 1
                        T.stop(2, step)
                        break
                    beta = f[k] / mkk
                    r = r - beta * g
                    x = x + beta * u
                    rr = float(np.vdot(r, r).real)
                    out = tested()
                    if out is not None:
                        flag, it = out
                        break
                    f[:k + 1] = 0
                    f[k + 1:] = f[k + 1:] - beta * M[k + 1:, k]
                    step += 1
                if flag is not None:
                    break
                vh = solve(r.copy())
                t = A @ vh
                tr, tt = np.vdot(t, r), np.vdot(t, t)
                T.scalar("tt", step, tt, rr)
                T.scalar("tr", step, tr, np.sqrt(tt.real) * np.sqrt(rr))
                if _bad(tt) or _bad(tr):
                    flag, it = 1, step + 1
                    T.stop(4, step)
                    break
                om = tr / tt
                rho = abs(tr) / (np.sqrt(tt.real) * np.sqrt(rr))
                if T.t is not None:
                    T.t["cosines"].append(float(rho))
                if rho < KAPPA:
                    om = om * (KAPPA / rho)
                r = r - om * t
                x = x + om * vh
                rr = float(np.vdot(r, r).real)
                out = tested()
                if out is not None:
                    flag, it = out
                    break
                step += 1
        X[:, col], flags[col], iters[col] = x, flag, it
    return X, flags, iters


def idrs_sequential(solve, A, B, P, rtol, maxit, trace=None):
    """the textbook form: one inner product with p_l and one update of g and u after the other"""
    return idrs_restated(solve, A, B, P, rtol, maxit, trace=trace, sequential=True)


# ---- the generated shadow block ---------------------------------------------------------------------------------------------
def probe_value(seed, counter):
    """include/hifir_amd.h: z = seed + 0x9E3779B97F4A7C15 counter (mod 2^64), the splitmix64 finalizer, u = (z >> 11) 2^-53,
    value 2 u - 1; counter an array of uint64"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * np.asarray(counter, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return 2.0 * ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) - 1.0


def generated_P(n, s, seed, cplx):
    """what the device generates for P == NULL: entry (i, j) from counter 16 i + j + 1, the imaginary part of a complex entry
    from counter 16 (n + i) + j + 1"""
    i, j = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(s, dtype=np.uint64), indexing="ij")
    re = probe_value(seed, np.uint64(16) * i + j + np.uint64(1))
    if not cplx:
        return re
    return re + 1j * probe_value(seed, np.uint64(16) * (np.uint64(n) + i) + j + np.uint64(1))


# ---- the pairs -----------------------------------------------------------------------------------------------------------------
CONFIG = {
    "cd2d_48": dict(amp=0.05, real=True, rtol=1e-10, widths=(1, 3, 33, 63, 64, 65, 129)),
    "pcd2d_32": dict(amp=0.05, real=True, rtol=1e-10, widths=(33, 65)),
    "young1c": dict(amp=0.05, real=False, rtol=1e-9, widths=(33, 65)),
}
CASES = [("cd2d_48", 4), ("pcd2d_32", 4), ("young1c", 4)] + [("cd2d_48", s) for s in (1, 2, 3, 8)]  # (fixture, s)
GEN_SEED = 5
GEN_CASES = [("cd2d_48", 4, GEN_SEED), ("young1c", 4, GEN_SEED)]  # (fixture, s, seed): the block the device generates from seed
ALL_CASES = CASES + GEN_CASES  # the keys of the tables below
SIDE_WIDTH = 33  # the only width of s != 4 and of the generated blocks
MAXIT = 300
P_SEED = 77  # numpy seed of the explicit shadow block
# random columns (seed 1000 + j) that are not IdrsPair.stable on that (fixture, s) are passed over: the j-th hard column of every
# batch is the j-th seed that is left
SKIP_SEEDS = {("pcd2d_32", 4): (1001, 1002, 1004, 1006, 1007, 1009, 1010, 1012, 1014, 1015, 1017)}
# (fixture, s) -> {width: columns of that batch that are not stable}: the device is not held to the restatement there
# (on pcd2d_32 that is every column of the ladder -- easy, pow4, pow8, huge -- and b and A 1: one rounding moves their step count;
# its hard columns come from the vetted seeds)
UNVETTED = {
    ("pcd2d_32", 4): {33: (2, 4, 5, 6, 7, 8, 11, 13, 14, 15, 16, 17, 20, 22, 23, 24, 25, 26, 29, 31),
                      65: (2, 4, 5, 6, 7, 8, 11, 13, 14, 15, 16, 17, 20, 22, 23, 24, 25, 26, 29, 31, 33, 34, 35, 36, 37, 38, 41, 43, 44,
                           45, 46, 47, 50, 52, 53, 54, 55, 56, 59, 61, 62, 63)},
    ("cd2d_48", 1): {33: (5, 14, 23)},
    ("cd2d_48", 3): {33: (8, 17, 26)},
    ("cd2d_48", 4, GEN_SEED): {33: (5, 14, 23)},
    ("young1c", 4, GEN_SEED): {33: (6, 15, 24)},
}
# (fixture, s) -> the measured sensitivity of every kind of vetted column (measured_sensitivities), rounded up to two digits
SENS = {
    ("cd2d_48", 4): {"hard": 1.8e-13, "easy": 3.6e-13, "b": 5.9e-15, "ones": 8.5e-16, "pow4": 5.6e-12, "pow8": 1.3e-11, "ladder": 6e-11},
    ("pcd2d_32", 4): {"hard": 8.3e-11, "ladder": 6.8e-11},
    ("young1c", 4): {"hard": 3.5e-15, "easy": 1.4e-15, "b": 1.9e-15, "ones": 1.9e-15, "pow4": 8.9e-16, "pow8": 1.1e-15, "ladder": 2e-15},
    ("cd2d_48", 1): {"hard": 2.2e-14, "easy": 6.1e-16, "ones": 5.9e-16, "pow4": 1.7e-15, "pow8": 8.4e-16, "ladder": 7.7e-15},
    ("cd2d_48", 2): {"hard": 1.6e-15, "easy": 1.2e-15, "b": 3.7e-15, "ones": 4.4e-13, "pow4": 2.7e-13, "pow8": 1.5e-15, "ladder": 2.7e-13},
    ("cd2d_48", 3): {"hard": 2.6e-12, "easy": 5.1e-16, "b": 4e-15, "ones": 8.8e-16, "pow4": 3.8e-16, "ladder": 7.1e-15},
    ("cd2d_48", 8): {"hard": 4.5e-15, "easy": 9.2e-15, "b": 1.4e-14, "ones": 6.4e-16, "pow4": 3.1e-15, "pow8": 1.4e-12, "ladder": 1.4e-12},
    ("cd2d_48", 4, GEN_SEED): {"hard": 1.5e-14, "easy": 2.9e-15, "ones": 2.5e-11, "pow4": 7.1e-15, "pow8": 1.6e-11, "ladder": 1.6e-11},
    ("young1c", 4, GEN_SEED): {"hard": 3.3e-15, "easy": 1.3e-15, "b": 8.7e-16, "pow4": 9.7e-16, "pow8": 1.1e-15, "ladder": 2.1e-15},
}


def widths_of(name, s, gen=None):
    return CONFIG[name]["widths"] if s == 4 and gen is None else (SIDE_WIDTH,)


class IdrsPair(L.Pair):
    """lockstep_edges_util.Pair for IDR(s) on one fixture: its batches, restated columns, noise runs and sensitivities, with an
    explicit shadow block from numpy's generator (gen: the twin of the block the device generates from that seed)"""

    def __init__(self, name, s, gen=None):
        from oracle import orc
        from util import load_hier

        self.solver, self.name, self.s, self.gen = "idrs", name, s, gen
        self.key = (name, s) if gen is None else (name, s, gen)
        self.cfg = cfg = dict(CONFIG[name], widths=widths_of(name, s, gen))
        self.levels, self.d = load_hier(name)
        self.A = perturbed(self.d, cfg["amp"], real=cfg["real"])
        self.O = orc.Oracle(self.levels)
        self.Q, self.apply = None, self.O
        self.cplx = np.iscomplexobj(self.A.data) or self.O.dtype.kind == "c"
        self.rtol = cfg["rtol"]
        self.seeds = [j for j in range(1000, 1200) if j not in SKIP_SEEDS.get(self.key, ())]
        n = self.A.shape[0]
        rng = np.random.default_rng(P_SEED)
        self.P = rng.uniform(-1, 1, (n, s)) + (1j * rng.uniform(-1, 1, (n, s)) if self.cplx else 0.0)
        if gen is not None:
            self.P = generated_P(n, s, gen, self.cplx)
        self._ref, self._batches = {}, {}

    def _run(self, solve, b, maxit, sequential=False, P=None):
        tr = []
        X, fl, it = idrs_restated(solve, self.A, b.copy(), self.P if P is None else P, self.rtol, maxit, trace=tr,
                                  sequential=sequential)
        return X[:, 0], int(fl[0]), int(it[0]), tr[0]

    def restated(self, b, maxit=MAXIT, rtol=None, sequential=False):
        assert rtol is None or rtol == self.rtol
        key = (b.tobytes(), maxit, sequential)
        if key not in self._ref:
            self._ref[key] = self._run(self.apply.solve, b, maxit, sequential)
        return self._ref[key]

    def noisy(self, b, seed, maxit=MAXIT):
        rng = np.random.default_rng(seed)
        solve = self.apply.solve

        def apply(r):
            y = solve(r)
            return y * (1.0 + 2.0 ** -52 * rng.uniform(-1, 1, len(y)))

        return self._run(apply, b, maxit)

    def stable(self, b, maxit=MAXIT, seeds=(5, 6, 7, 8, 9, 10)):
        """lockstep_edges_util.Pair.stable, and the textbook sequential form stops where the blocked one does: its roundings sit
        in the biorthogonalization, where noise on the applies does not reach"""
        x, fl, it, tr = self.restated(b, maxit=maxit)
        if not decisions_ok(tr, self.rtol):
            return False
        xs, fs, its, ts = self.restated(b, maxit=maxit, sequential=True)
        if (fs, its) != (fl, it) or not decisions_ok(ts, self.rtol):
            return False
        for sd in seeds:
            xs, fs, its, ts = self.noisy(b, sd, maxit)
            if (fs, its) != (fl, it) or not decisions_ok(ts, self.rtol):
                return False
        return True

    def vetted(self, width):
        """the columns of batch(width) the device is held to the restatement on"""
        bad = UNVETTED.get(self.key, {}).get(width, ())
        return [c for c in range(width) if c not in bad]


def decisions_ok(trace, rtol):
    return L.decisions_ok(trace, rtol) and all(abs(v / KAPPA - 1.0) >= COS_MARGIN for v in trace["cosines"])


_PAIRS = {}


def pair(name, s, gen=None):
    key = (name, s) if gen is None else (name, s, gen)
    if key not in _PAIRS:
        _PAIRS[key] = IdrsPair(name, s, gen)
    return _PAIRS[key]


def tolerance(P, kind):
    return max(1000.0 * SENS[P.key][kind], 1e-12)


def measured_sensitivities(P):
    """the largest Pair.sensitivity over the vetted columns of every kind in the widest batch, and over the ladder"""
    w = max(P.cfg["widths"])
    B, fates = P.batch(w)
    out = {}
    for c in P.vetted(w):
        if B[:, c].any():
            k = L.kind_of(fates[c])
            out[k] = max(out.get(k, 0.0), P.sensitivity(B[:, c]))
    out["ladder"] = max(P.sensitivity(v) for v in ladder(P) if P.stable(v))
    return out


def round_up(v):
    """v rounded up to two digits"""
    if v == 0.0:
        return 0.0
    e = int(np.floor(np.log10(v))) - 1
    return float("%.1e" % (np.ceil(v / 10.0 ** e * (1 - 1e-12)) * 10.0 ** e))


# ---- maxit edges -------------------------------------------------------------------------------------------------------------
# (fixture, s, m, three columns that need m - 1, m and m + 1 steps; ("pow", k) is the ladder's G^k g, ("seed", j) the j-th hard
# column): with s = 4 a cycle is 5 steps, steps 5, 10, 15 .. are omega steps and the others lie inside a cycle
MAXIT_EDGES = [("cd2d_48", 4, 16, (("pow", 10), ("pow", 7), ("pow", 1)))]  # 15: an omega step; 16: the first step of a cycle


def maxit_columns(P, spec):
    Ld = ladder(P)
    return np.stack([Ld[k] if what == "pow" else P.hard(k) for what, k in spec], axis=1)




# ---- exact constructions on a diagonal hierarchy ------------------------------------------------------------------------------
def exact_case():
    """M^{-1} = I on 14 rows (diagonal_levels) and A = blockdiag(2 I_4, [[0, 1], [-1, 0]], diag(1 .. 8)); every case lives on one
    block (b and P vanish elsewhere) and holds small integers only, so that its zeros are exact under any order of summation.
    -> dict(levels, A, cases {name: (b, P, (flag, steps), updates)}), updates = completed updates x holds
      half     rows 0..3, s = 2: u = b, g = 2 b, M[0,0] = 2 f_0, beta = 1/2, r = b - (1/2)(2 b) = 0: flag 0 at step 1, x = b / 2
      pzeroJ   rows 6..13, s = 3, column J of P zero: raw_J and every stored M[J,l] are sums of zeros, M[J,J] = 0 at step J + 1
               (mode 2), x holds the J updates before it
      skew     rows 4..5, s = 1, b = (1, 1), p = e_4: g = A b = (1, -1), M[0,0] = 1, beta = 1, r = (0, 2), x = (1, 1); then
               t = A r = (2, 0) and (t, r) = 0: flag 1 at step 2 (mode 4), x keeps the one update"""
    n = 14
    A = sp.csr_matrix(sp.block_diag([2.0 * np.eye(4), np.array([[0.0, 1.0], [-1.0, 0.0]]), np.diag(np.arange(1.0, 9.0))]))
    A.sort_indices()
    cases = {}
    b = np.zeros(n)
    b[:4] = (1, 3, -2, 1)
    P = np.zeros((n, 2))
    P[:4, 0], P[:4, 1] = (1, 1, 0, 2), (0, 1, 1, -1)
    cases["half"] = (b, P, (0, 1), 1)
    b = np.zeros(n)
    b[6:] = (1, 2, 1, 3, 1, 2, 2, 1)
    P3 = np.zeros((n, 3))
    P3[6:, 0], P3[6:, 1], P3[6:, 2] = (1, 0, 2, 1, 0, 1, 1, 0), (0, 1, 1, 0, 2, 0, 1, 1), (1, 1, 0, 0, 1, 2, 0, 1)
    for j in range(3):
        Pj = P3.copy()
        Pj[:, j] = 0.0
        cases["pzero%d" % j] = (b, Pj, (1, j + 1), j)
    b = np.zeros(n)
    b[4:6] = (1, 1)
    P = np.zeros((n, 1))
    P[4, 0] = 1.0
    cases["skew"] = (b, P, (1, 2), 1)
    return dict(levels=diagonal_levels(np.ones(n)), A=A, cases=cases)
