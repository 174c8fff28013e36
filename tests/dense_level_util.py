"""Generators and references for the dense last level at its tile, K-split and rank edges (test_dense_level_host.py pins the
references to each other on the CPU, test_gpu_dense_level.py holds the kernels against them).

What the kernels of the level rest on (Engine::launch_dense / launch_dense_mul / zgemm, k_dense_gemm_d<4>): guards on 16-row
strips, k-quads of 4, operand sets of 32 k dealt to 4 waves (K stride 128), two register sets rotating at kb, kb + 128 and
kb + 256, kend clipped to the strip (tri == 2), kbeg = i0 (tri == 1), rank truncation (mrows_valid < mrows_total and kend = rk)
and column tiles cut at R.  LADDER and STEP_RANKS put a dimension and a rank on either side of each of those steps: 257 and 300
are the smallest sizes that reach the kb + 256 reload, 417 = 3 * 128 + 32 + 1 the smallest at which a second wave loads a
fourth operand set in the second trip of the pipelined loop.

References: numpy / scipy restatements of the four block operators (BlockRef: LAPACK's geqp3, heevd / syevd, gesv) and of the
level's scaling / permutation wrapper around the block (level_apply), independent of the oracle and of the engine.  The
symmetric kinds are measured against eigh because the oracle's cyclic Jacobi loses about nd * 1e-15 on the eigenvalues
(DESIGN section 5); its QRCP and LUP agree with LAPACK to a few 1e-15 at every size."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from util import rand_rhs, rand_tri, synth_level

KINDS = ("qrcp", "symm0", "symm1", "lup")  # symm0: dense_symm with spd = 0 (indefinite), symm1: spd = 1
OPS = ("S", "SH", "M", "MH")  # M^-1, M^-H, M, M^H
LADDER = (1, 2, 5, 15, 16, 17, 33, 64, 65, 127, 129, 161, 257, 300, 417)
LADDER_Z = tuple(nd for nd in LADDER if nd not in (127, 300))  # complex handles (every real plane is twice as wide)
FRONT_SIZES = (17, 65, 129)  # the sizes that also run behind a 37-row sparse level, and in narrow arenas
FRONT_ROWS = 37
STEP_RANKS = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 385)
COND_GENERAL, COND_SYMM = 100.0, 128.0  # what the generators promise about the blocks' 2-norm condition numbers
LEAD = 2.0  # weight of the lead direction in a right-hand side, in units of the random part's norm (block_rhs)


def qrcp_ranks(nd):
    """The truncation ranks tried on a QRCP block: every step rank below nd, nd - 1 and nd."""
    return tuple(sorted(({r for r in STEP_RANKS if r < nd} | {nd - 1, nd}) - {0}))


def symm_ranks(nd):
    """At most 7 of qrcp_ranks(nd), the ones a symmetric block's spectrum gets a gap for: 1, nd - 1 and nd, the ranks one past
    a step of the kernel (r = 1 mod 4, 16, 32, 128: the last k-quad, operand set and K stride hold one column), largest
    first, then the largest of the rest."""
    cand = qrcp_ranks(nd)
    if len(cand) <= 7:
        return cand
    keep = [1, nd, nd - 1]
    for r in (385, 257, 129, 33, 17, 5) + tuple(reversed(cand)):
        if len(keep) < 7 and r in cand and r not in keep:
            keep.append(r)
    return tuple(sorted(keep))


def rank_arguments(kind, nd):
    """The rank ARGUMENTS of a case: explicit ranks, then 0 (the numerical rank), -1 and nd + 5 (both: nd).  LUP ignores the
    argument (LUP.hpp:141,181): 0 and 7."""
    if kind == "lup":
        return (0, 7)
    return (qrcp_ranks(nd) if kind == "qrcp" else symm_ranks(nd)) + (0, -1, nd + 5)


def truncated_rank(kind, nd):
    """The second largest rank tested (nd - 1; at nd = 1 there is none below nd)."""
    if kind == "lup":
        return 0
    return max(nd - 1, 1)


def eff_rank(rank, nd, numerical):
    """The rank-argument contract (Engine::eff_rank, QRCP.hpp:376-377): 0 the numerical rank, < 0 or > nd the dimension."""
    if rank == 0:
        return numerical
    return nd if rank < 0 or rank > nd else rank


def symm_spectrum(nd, spd):
    """Eigenvalues in truncation order (syeig_factorize: spd = 0 decreasing |w|, spd > 0 ascending w): position i has modulus
    2^-g(i) (spd = 0) or 2^g(i) (spd > 0) with g(i) the number of tested ranks <= i -- plateaus with a factor-2 gap behind
    position r - 1 for every tested rank r < nd.  spd = 0: every third eigenvalue is negative."""
    ranks = symm_ranks(nd)
    g = np.array([sum(1 for r in ranks if r <= i) for i in range(nd)], dtype=np.float64)
    if spd > 0:
        return 2.0 ** g
    w = 2.0 ** -g
    w[2::3] *= -1.0
    return w


def _normal(rng, shape, dtype):
    A = rng.normal(size=shape)
    if np.dtype(dtype).kind == "c":
        A = A + 1j * rng.normal(size=shape)
    return A.astype(dtype)


def dense_matrix(nd, kind, dtype, rng):
    """The block of a case, (nd, nd).  qrcp / lup: normal (+ 1j normal) + 2.5 sqrt(nd) I, condition number <= 100 asserted
    (every leading block R(1:r, 1:r) of the pivoted factor is then at least as well conditioned: the first r pivoted
    columns are a column subset of a full-rank matrix).  symm*: V diag(w) V^H symmetrised, V random orthogonal / unitary,
    w = symm_spectrum, condition number <= 128."""
    if kind in ("qrcp", "lup"):
        D = _normal(rng, (nd, nd), dtype) + 2.5 * np.sqrt(nd) * np.eye(nd)
        assert np.linalg.cond(D) <= COND_GENERAL
        return D
    w = symm_spectrum(nd, 1 if kind == "symm1" else 0)
    assert np.abs(w).max() / np.abs(w).min() <= COND_SYMM
    V, _ = np.linalg.qr(_normal(rng, (nd, nd), dtype))
    D = (V * w) @ V.conj().T
    return ((D + D.conj().T) / 2).astype(dtype)


def _seed(nd, kind, dtype, m):
    return 100000 * KINDS.index(kind) + 10000 * (np.dtype(dtype).kind == "c") + 1000 * (m > 0) + nd


def dense_level(nd, kind, dtype, m=0, seed=None):
    """A one-level hierarchy whose dense block is the last level AT level 0 (launch_dense / launch_dense_mul run, no tail
    operator forms): the front level is synth_level with random p, q, s, t, empty (m = 0: everything is deferred to the block)
    or a 37-row sparse level with random triangles, E and F (m = 37: the block starts at row 37 of the work arrays)."""
    assert kind in KINDS and m in (0, FRONT_ROWS)
    rng = np.random.default_rng(_seed(nd, kind, dtype, m) if seed is None else seed)
    n = m + nd
    if m == 0:
        lv = synth_level(0, n, sp.csr_matrix((0, 0)), sp.csr_matrix((0, 0)), sp.csr_matrix((n, 0)), sp.csr_matrix((0, n)), rng,
                         dtype=dtype)
    else:
        rs = np.random.RandomState(int(rng.integers(1 << 30)))
        lv = synth_level(m, n, rand_tri(m, 0.3, True, rng, dtype=dtype), rand_tri(m, 0.3, False, rng, dtype=dtype),
                         sp.random(nd, m, density=0.2, random_state=rs, format="csr"),
                         sp.random(m, nd, density=0.2, random_state=rs, format="csr"), rng, dtype=dtype)
    lv["dense_n"], lv["dense"] = nd, dense_matrix(nd, kind, dtype, rng).ravel(order="F")
    if kind.startswith("symm"):
        lv["dense_symm"], lv["spd"] = 1, int(kind[-1])
    elif kind == "lup":
        lv["dense_lup"] = 1
    return [lv]


def block_of(levels):
    nd = int(levels[-1]["dense_n"])
    return np.asarray(levels[-1]["dense"]).reshape(nd, nd, order="F")


class BlockRef:
    """The four operators of one block, (nd, k) -> (nd, k), restated with LAPACK through numpy / scipy.

    qrcp (QRCP.hpp:371-541), D P = Q R from scipy.linalg.qr(pivoting=True), r = eff_rank:
        S   z[P[:r]] = R11^-1 Q[:, :r]^H c        SH  Q[:, :r] R11^-H c[P[:r]]
        M   Q[:, :r] R11 c[P[:r]]                 MH  z[P[:r]] = R11^H Q[:, :r]^H c        (rows of z beyond P[:r]: 0)
    symm* (SYEIG.hpp:181-273), D = V diag(w) V^H from numpy.linalg.eigh, `to` the truncation order of syeig_factorize:
        S = SH  V[:, to[:r]] diag(1 / w) V[:, to[:r]]^H c        M = MH  the same with w
    lup (LUP.hpp:141-188):  S solve(D, c),  M  D c,  SH solve(D^T, c) -- the PLAIN transpose, also for complex data, as the
        reference passes 'T' to ?getrs (LUP.hpp:150) -- and MH  D^H c."""

    def __init__(self, D, kind):
        self.kind, self.D, self.nd = kind, np.asarray(D), D.shape[0]
        self.rank = self.nd  # (the generators' blocks have full numerical rank; the host test asserts the oracle agrees)
        if kind == "qrcp":
            self.Q, self.R, self.P = sla.qr(self.D, pivoting=True)
        elif kind.startswith("symm"):
            self.w, self.V = np.linalg.eigh(self.D)
            self.to = np.arange(self.nd) if kind == "symm1" else np.argsort(-np.abs(self.w), kind="stable")

    def apply(self, op, C, rank=0):
        nd = self.nd
        r = eff_rank(rank, nd, self.rank)
        if self.kind == "lup":
            D = self.D
            return {"S": lambda: np.linalg.solve(D, C), "SH": lambda: np.linalg.solve(D.T, C), "M": lambda: D @ C,
                    "MH": lambda: D.conj().T @ C}[op]()
        if self.kind != "qrcp":
            Vk, wk = self.V[:, self.to[:r]], self.w[self.to[:r]]
            f = 1.0 / wk if op in ("S", "SH") else wk
            return Vk @ (f[:, None] * (Vk.conj().T @ C))
        Q1, R11, P1 = self.Q[:, :r], self.R[:r, :r], self.P[:r]
        Z = np.zeros_like(C)
        if op == "S":
            Z[P1] = sla.solve_triangular(R11, Q1.conj().T @ C)
        elif op == "SH":
            Z = Q1 @ sla.solve_triangular(R11, C[P1], trans="C")
        elif op == "M":
            Z = Q1 @ (R11 @ C[P1])
        else:
            Z[P1] = R11.conj().T @ (Q1.conj().T @ C)
        return Z


def level_apply(lv, ref, op, B, rank=0):
    """The m = 0 level around the block (prec_solve.hpp:359-411, :565-612; prec_prod.hpp:76-132, :171-230 with nothing but
    the deferred rows): gather with one permutation and scaling, the block operator, scatter with the other pair."""
    s, t = np.asarray(lv["s"])[:, None], np.asarray(lv["t"])[:, None]
    p, q, p_inv, q_inv = (np.asarray(lv[k]) for k in ("p", "q", "p_inv", "q_inv"))
    if op == "S":
        return t * ref.apply(op, (s * B)[p], rank)[q_inv]
    if op == "SH":
        return s * ref.apply(op, (t * B)[q], rank)[p_inv]
    if op == "M":
        return ref.apply(op, (B / t)[q], rank)[p_inv] / s
    return ref.apply(op, (B / s)[p], rank)[q_inv] / t


def lead_direction(ref, op):
    """The unit vector of the block's INPUT space that every truncation of the operator keeps (the truncations are nested):
    the eigenvector first in truncation order (SYEIG), the first column of Q (QRCP, M^-1 and M^H: they start with
    Q[:, :r]^H c) or the first pivot's unit vector (QRCP, M^-H and M: they start with c[P[:r]]); LUP has no truncation."""
    if ref.kind == "lup":
        return None
    if ref.kind != "qrcp":
        return ref.V[:, ref.to[0]]
    if op in ("S", "MH"):
        return ref.Q[:, 0]
    e = np.zeros(ref.nd, dtype=ref.D.dtype)
    e[ref.P[0]] = 1.0
    return e


def block_rhs(ref, op, k, rng, dtype):
    """(nd, k) inputs of the block operator: uniform random G plus, per column, LEAD * ||g|| * (a random sign / phase) times
    lead_direction.  Why: a truncated result is the image of the input's projection on the kept subspace, and the
    per-column relative error measures against that image.  A column nearly orthogonal to the kept subspace -- of 70
    random columns one always is, at rank 1 -- turns the measure into |dv^H c| / |v^H c|, the eigensolver's (or LAPACK's
    own) rounding in v times an arbitrary cancellation factor: a property of the column, not of the kernel.  With the
    lead component every column keeps >= LEAD / sqrt(LEAD^2 + 1) = 0.89 of its norm inside every kept subspace, all other
    directions still carry 0.45 of it, and an error in any term of a product stays far above the bars."""
    G = rand_rhs(rng, (ref.nd, k), dtype)
    u = lead_direction(ref, op)
    if u is None:
        return G
    gamma = rng.choice([-1.0, 1.0], k)
    if np.dtype(dtype).kind == "c":
        gamma = gamma * np.exp(1j * rng.uniform(-np.pi, np.pi, k))
    return (G + LEAD * u[:, None] * (gamma * np.linalg.norm(G, axis=0))[None, :]).astype(dtype)


def level_preimage(lv, op, Y):
    """B whose gather by the level (level_apply's first step: (s B)[p], (t B)[q], (B / t)[q], (B / s)[p]) is Y."""
    s, t = np.asarray(lv["s"])[:, None], np.asarray(lv["t"])[:, None]
    p_inv, q_inv = np.asarray(lv["p_inv"]), np.asarray(lv["q_inv"])
    if op == "S":
        return Y[p_inv] / s
    if op == "SH":
        return Y[q_inv] / t
    if op == "M":
        return Y[q_inv] * t
    return Y[p_inv] * s


def level_rhs(levels, ref, op, k, rng, dtype):
    """(n, k) right-hand sides of the hierarchy whose deferred rows reach the block as block_rhs.  m = 37: the leading rows
    are random at a tenth of the scale -- in a solve the block's input also receives the coupling term E (LDU)^-1 y[:m]
    (F^H ... for M^-H), which must not cancel the lead component; the products hand y[m:] to the block as it is."""
    lv = levels[0]
    m = int(lv["m"])
    Y = np.concatenate([0.1 * rand_rhs(rng, (m, k), dtype), block_rhs(ref, op, k, rng, dtype)])
    return np.ascontiguousarray(level_preimage(lv, op, Y).astype(dtype))


def engine_apply(M, op, B, rank=0):
    if op in ("S", "SH"):
        return M.solve_mrhs(B, rank=rank, trans=op == "SH")
    return M.mmultiply(B, rank=rank, trans=op == "MH")


def oracle_apply(O, op, B, rank=0):
    if op in ("S", "SH"):
        return O.solve_batch(B, rank=rank, threads=4, trans=op == "SH")
    return O.mmultiply_batch(B, rank=rank, trans=op == "MH")


def colerr(X, Xo):
    """largest relative error (infinity norm) of a column against the same column of the reference"""
    num, den = np.abs(X - Xo).max(axis=0), np.abs(Xo).max(axis=0)
    return float((num / np.maximum(den, 1e-300)).max())


def expected_census(kind, cplx, op):
    """Launches of one lane at the dense level (launch_dense / launch_dense_mul; complex: zgemm = two real planes and
    k_zcombine per product): LUP one product, QRCP and SYEIG two; k_row_gather in front of the adjoint QRCP solve and the
    forward QRCP product."""
    g = 1 if kind == "lup" else 2
    return dict(dense_gemm=2 * g if cplx else g, zcombine=g if cplx else 0,
                row_gather=1 if kind == "qrcp" and op in ("SH", "M") else 0)
