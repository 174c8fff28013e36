"""Inputs and restatements for the batch, restart and stopping edges of GMRES, FGMRES and iterative refinement
(test_krylov_edges_host.py pins them on the CPU, test_gpu_krylov_edges.py holds the drivers against them).  numpy / scipy only.

The restatement of GMRES / FGMRES is oracle.orc.gmres; the one of the refinement is ir_restated below.  Two kinds of input:

  real hierarchies with a mediocre preconditioner (perturbed): columns of different difficulty in one batch (mixed_batch).  The
  difficulty ladder is G^k g with G = I - A M^-1 and g random: every application of G removes the directions the
  preconditioner handles well, what is left lies in ever fewer dominant directions of G and GMRES needs ever fewer steps.

  the identity hierarchy (identity_levels: M^-1 = I exactly) with a matrix that acts on unit vectors as a weighted graph:
  every residual ratio a stopping rule looks at is 0, 1 or a weight of the graph, in exact arithmetic and -- because the
  products and sums involved are exact or off by one rounding -- on the device as well (stagnating_case, ir_mixed_batch).
  Why not a real hierarchy there: refinement contracts by a fixed factor per sweep (0.08 ... 0.9 on the perturbed fixtures),
  so consecutive residual ratios of a column are never a factor 100 apart and no beta can keep a factor 10 from both;
  GMRES approaches stagnation gradually, through the whole band between 1 - 1e-4 and 1 - 1e-8."""
import numpy as np
import scipy.sparse as sp

from dense_level_util import dense_level


QUIRK = ("cd2d_48", 4, 8, 1e-9)  # fixture (perturbed, amp 0.05, real), restart, maxit = 2 * restart, rtol: flag 0, iters == maxit


def csr_of(d):
    n = len(d["b"])
    return sp.csr_matrix((d["A_vals"], d["A_indices"], d["A_indptr"]), shape=(n, n))


def perturbed(d, amp, seed=7, real=False):
    """the fixture's matrix with a random complex diagonal added: the hierarchy becomes a mediocre preconditioner,
    so that the solve needs tens of iterations and crosses restarts.  real: only the real part of that diagonal (a
    real handle's matrix stays real)."""
    n = len(d["b"])
    A = csr_of(d)
    if amp:
        rng = np.random.default_rng(seed)
        re, im = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
        A = (A + sp.diags(amp * abs(A).max() * (re if real else re + 1j * im))).tocsr()
    A.sort_indices()
    return A


def identity_levels(n):
    """A one-level hierarchy with M^-1 = I: no sparse rows, unit scalings, identity permutations, dense block I."""
    lv = dense_level(n, "qrcp", np.float64, m=0, seed=1)[0]
    lv["s"], lv["t"] = np.ones(n), np.ones(n)
    for k in ("p", "q", "p_inv", "q_inv"):
        lv[k] = np.arange(n, dtype=np.int32)
    lv["dense"] = np.eye(n).ravel(order="F")
    return [lv]


def _rand(rng, n, cplx):
    v = rng.uniform(-1, 1, n)
    return v + 1j * rng.uniform(-1, 1, n) if cplx else v


# ---- columns of prescribed fate for the lock-step drivers ------------------------------------------------------------------
EASY_POWER = 12  # G^12 g: finishes inside the first cycle of GMRES(12) on the perturbed fixtures (the host test asserts it)
FILL = ("zero", "easy", "tiny", "huge", "b", "ones", "pow4", "pow8", "hard")
SCALED_COPY_OF = {"tiny": "hard", "huge": "easy"}  # the fate whose first column a scaled copy repeats


def mixed_fates(width):
    """The fate of every column: hard ones at 0, 32 and width - 1, easy ones at 31 and 33 (either side of the lane boundaries
    of the c = threadIdx.x % nc mapping and of the 64-column tile cut where the width reaches them), the rest FILL in turn."""
    fates = [None] * width

    def put(i, f):
        if 0 <= i < width and fates[i] is None:
            fates[i] = f

    put(0, "hard"), put(width - 1, "hard"), put(32, "hard"), put(31, "easy"), put(33, "easy"), put(63, "easy"), put(64, "hard")
    k = 0
    for i in range(width):
        if fates[i] is None:
            fates[i] = FILL[k % len(FILL)]
            k += 1
    return fates


def mixed_batch(O, d, A, width, seed):
    """-> (B [n][width], fates).  zero: 0 | ones: A @ ones | b: the fixture's | hard: uniform random (a fresh one per column) |
    powK / easy: G^K g normalized, G = I - A M^-1, g column 0 | tiny: column 0 (hard) times 1e-30 | huge: the easy column
    (G^12 g) times 1e+30.  O, the oracle of the hierarchy, is an argument because the ladder G^k g needs the apply: nothing
    but G's own dominant directions gives columns that finish a whole outer cycle earlier on these fixtures (A @ ones, the
    fixture's b and random columns all need 16 ... 18 iterations on cd2d_48)."""
    n = A.shape[0]
    cplx = np.iscomplexobj(A.data) or O.dtype.kind == "c"
    rng = np.random.default_rng(seed)
    fates = mixed_fates(width)
    B = np.zeros((n, width), dtype=np.complex128 if cplx else np.float64)
    g = _rand(rng, n, cplx)
    powers = {0: g}
    v = g
    for k in range(1, EASY_POWER + 1):
        v = v - A @ O.solve(v)
        v = v / np.linalg.norm(v)
        powers[k] = v
    for c, f in enumerate(fates):
        if f == "hard":
            B[:, c] = g if c == 0 else _rand(rng, n, cplx)
        elif f == "ones":
            B[:, c] = A @ np.ones(n)
        elif f == "b":
            B[:, c] = d["b"]
        elif f == "easy":
            B[:, c] = powers[EASY_POWER] * (1.0 + c)
        elif f.startswith("pow"):
            B[:, c] = powers[int(f[3:])]
        elif f == "tiny":
            B[:, c] = 1e-30 * g
        elif f == "huge":
            B[:, c] = 1e+30 * powers[EASY_POWER]
    return B, fates


def finishing_steps(iters, restart):
    """(outer cycle, inner step) at which a converged column of `iters` iterations left"""
    return (iters - 1) // restart, (iters - 1) % restart


def neighbours_replaced(B, keep, how, seed=3):
    """B with every column but `keep` replaced by zeros / NaN / inf / 1e300 * random"""
    rng = np.random.default_rng(seed)
    R = {"zero": lambda: np.zeros(B.shape), "nan": lambda: np.full(B.shape, np.nan), "inf": lambda: np.full(B.shape, np.inf),
         "big": lambda: 1e300 * rng.uniform(-1, 1, B.shape)}[how]().astype(B.dtype)
    R[:, keep] = B[:, keep]
    return R


# ---- exact stopping rules on the identity hierarchy ------------------------------------------------------------------------
def _graph(n, edges):
    """G with G e_src = w e_dst for (src, dst, w) in edges"""
    s, t, w = zip(*edges)
    return sp.csr_matrix((w, (t, s)), shape=(n, n))


def stagnating_case():
    """M^-1 = I on 128 rows and A block diagonal:
      rows 0..31   the cyclic shift, A e_i = e_(i+1).  b = e_0: the first step has h = 0, |v| = 1, residual ratio exactly 1:
                   flag 1, 0 iterations, x = 0  ("now")
      rows 32..63  the cyclic shift plus A[32, 32] = 1.  b = e_32: A e_32 = e_32 + e_33, the first step halves the squared
                   residual (ratio 2^-1/2), the second finds A e_33 = e_34 orthogonal to everything (ratio exactly 1): flag 1,
                   1 iteration, x = e_32 / 2  ("later")
      rows 64..95  diag(1, 2, 3, 1, 2, 3, ...).  A column on them has 1, 2 or 3 distinct eigenvalues and converges to rounding
                   in as many steps ("conv1", "conv2", "conv3").
      rows 96..127 the cyclic shift with A e_96 = a e_96 + t e_97, t = fl(1 - 1e-8) and a = sqrt(1 - t^2).  b = e_96: h = a,
                   |v| = t, rho = sqrt(fl(a^2) + fl(t^2)) rounds to 1 and the residual ratio is t, EQUAL to the bound of
                   resid >= resid_prev * (1 - 1e-8): flag 1, 0 iterations  ("edge").  Not a margin but the comparison itself
                   (>= against >): every sum has one nonzero term and sqrt and the quotients are correctly rounded on
                   both sides, so the equality is exact on the host and on the device.  The library is built with
                   -ffp-contract=off, so rho is formed from two rounded squares as on the host; were the sum contracted to
                   an fma, a^2 + t^2 would still be 1 +- one rounding and rho 1 or the double below it, the ratio t or larger
                   and the flag the same.
    Arnoldi on the shifts walks the unit vectors, so the device meets the same exact zeros and ones.
    -> dict(levels, A, columns {name: b}, expected {name: (flag, iters)})"""
    n = 128
    t = 1.0 * (1.0 - 1e-8)
    a = float(np.sqrt(1.0 - t * t))
    assert np.sqrt(a * a + t * t) == 1.0
    edges = [(i, (i + 1) % 32, 1.0) for i in range(32)] + [(32 + i, 32 + (i + 1) % 32, 1.0) for i in range(32)] + [(32, 32, 1.0)]
    edges += [(96 + i, 96 + (i + 1) % 32, t if i == 0 else 1.0) for i in range(32)] + [(96, 96, a)]
    A = (_graph(n, edges) + sp.diags(np.r_[np.zeros(64), np.tile([1.0, 2.0, 3.0], 11)[:32], np.zeros(32)])).tocsr()
    A.sort_indices()
    cols = {"edge": np.zeros(n)}
    cols["edge"][96] = 1.0
    for name, rows in (("now", [0]), ("later", [32]), ("conv1", [64, 67, 70]), ("conv2", [64, 65, 67, 68]), ("conv3", range(64, 96))):
        b = np.zeros(n)
        b[list(rows)] = 1.0 + 0.25 * np.arange(len(list(rows)))
        cols[name] = b
    expected = {"now": (1, 0), "later": (1, 1), "conv1": (0, 1), "conv2": (0, 2), "conv3": (0, 3), "edge": (1, 0)}
    return dict(levels=identity_levels(n), A=A, columns=cols, expected=expected)


def gmres_ratio_history(C, b, steps):
    """resid_j / resid_(j-1), j = 1 .. steps, of GMRES on the dense operator C = A M^-1 from x0 = 0, by least squares over
    the Krylov matrix (independent of the Arnoldi restatement): resid_j = min_y |b - C K_j y| / |b|."""
    K = np.zeros((len(b), 0))
    v = b / np.linalg.norm(b)
    prev, out = 1.0, []
    for _ in range(steps):
        K = np.column_stack([K, v])
        K, _ = np.linalg.qr(K)
        W = C @ K
        y = np.linalg.lstsq(W, b, rcond=None)[0]
        res = np.linalg.norm(b - W @ y) / np.linalg.norm(b)
        out.append(res / prev)
        prev = res
        v = C @ v
        v = v / np.linalg.norm(v)
    return out


# ---- iterative refinement ---------------------------------------------------------------------------------------------------
def ir_restated(O, A, b, nirs, betas=None, trans=False, rank=-1, history=None):
    """HIF::hifir (IterRefine.hpp:77-105 without betas, :121-165 with) around the oracle's apply, in the order of operations
    of Engine::hifir_dev.  trans: A^H x = b with M^-H.  -> (x, iters, flag); history (a list) receives the residual ratios
    |b - A x| / |b| the bounded loop compared with betas."""
    Aop = A.conj().T.tocsr() if trans else A
    dt = np.complex128 if (O.dtype.kind == "c" or np.iscomplexobj(A.data) or np.iscomplexobj(b)) else np.float64
    b = np.asarray(b, dtype=dt)
    if nirs <= 1:
        return O.solve(b, rank=rank, trans=trans), 1, -1
    x = np.zeros(len(b), dtype=dt)
    if betas is None:
        for i in range(nirs):
            xk = x
            r = b - Aop @ xk if i else b
            x = O.solve(r, rank=rank, trans=trans) + xk
        return x, nirs, -1
    bnorm = np.linalg.norm(b)
    iters, flag = 0, 0
    if bnorm != 0.0:
        r = b
        while True:
            x = x + O.solve(r, rank=rank, trans=trans)
            iters += 1
            if iters >= nirs:
                flag = -1
                break
            r = b - Aop @ x
            res = np.linalg.norm(r) / bnorm
            if history is not None:
                history.append(res)
            if res <= betas[0]:
                break
            if res > betas[1]:
                flag = 1
                break
    return x, iters, flag


IR_FATES = ("zero", "two", "later", "exhaust", "diverge")


def ir_mixed_batch(width=5, seed=2):
    """Bounded refinement with all five fates in one batch, M^-1 = I on 64 rows, A = I - G with G a weighted graph on the unit
    vectors: a chain entered with weight 0.02 and followed with weight 1 gives the residual ratio 0.02 sweep after sweep and
    exactly 0 once it ends.  betas = (1e-3, 0.5), nirs = 8: every ratio is 0, 0.02 or 8 -- a factor >= 10 from both betas.
      zero     b = 0                             (0, 0)
      two      a chain of one edge               (2, 0)
      later    chains of 2 .. 5 edges            (3 .. 6, 0), by the column
      exhaust  a chain of 12 edges               (8, -1)
      diverge  one edge of weight 8              (1, 1)
    Columns take the fates in turn and a random scale each.  -> dict(levels, A, B, betas, nirs, fates, expected [(iters, flag)])"""
    n, nirs, betas = 64, 8, (1e-3, 0.5)
    chains = {}
    edges = [(0, 1, 0.02), (60, 61, 8.0)] + [(40 + i, 41 + i, 0.02 if i == 0 else 1.0) for i in range(12)]
    at = 4
    for L in range(2, 6):
        edges += [(at + i, at + i + 1, 0.02 if i == 0 else 1.0) for i in range(L)]
        chains[L] = at
        at += L + 2
    A = (sp.identity(n) - _graph(n, edges)).tocsr()
    A.sort_indices()
    rng = np.random.default_rng(seed)
    B = np.zeros((n, width))
    fates, expected = [], []
    for c in range(width):
        f = IR_FATES[c % 5]
        scale = 10.0 ** rng.uniform(-3, 3)
        if f == "two":
            B[0, c] = scale
            expected.append((2, 0))
        elif f == "later":
            L = 2 + (c // 5) % 4
            B[chains[L], c] = scale
            expected.append((L + 1, 0))
        elif f == "exhaust":
            B[40, c] = scale
            expected.append((nirs, -1))
        elif f == "diverge":
            B[60, c] = scale
            expected.append((1, 1))
        else:
            expected.append((0, 0))
        fates.append(f)
    return dict(levels=identity_levels(n), A=A, B=B, betas=betas, nirs=nirs, fates=fates, expected=expected)
