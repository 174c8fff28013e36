"""Coupling blocks and hierarchies that put the Schur products out = s[p] b[p] - A x (A = E: S3, A = F: S5) at the edges of
their control flow -- the generators of test_schur_edges_host.py (CPU: the classes arrive, the oracle is pinned) and
test_gpu_schur_edges.py (GPU: the kernels against the oracle).  No reference access; built on util.synth_level.

Two ladders:

 * ladder_coupling: blocks of 16 rb rows whose distinct columns walk G_LADDER groups of four (host.hpp build_spmm_tiles cuts
   a block's distinct columns into such groups; k_spmm_tile / k_spmm_tile_z walk them in trips of 8 with look-aheads of 3 and
   7, k_spmm_tile4 deals them to four waves first), the last group padded by 0, 1, 2, 3 repeated columns in turn;
 * row_ladder_coupling: rows of ROW_NNZ nonzeros among thin rows (spmm_stream_r64 cuts a row into items of 64 nonzeros,
   k_spmm_epi_narrow unrolls by 8), and -- pairs_at -- rows w and w + pairs_at in every ordered pair of PAIR_CLASSES: with
   more than 16,384 rows wave w of k_spmm_epi takes both, the second prefetched while the first is consumed.

Values: sign * uniform(0.5, 1) * 0.5 / max(4, nonzeros of the row).  Absolute row sums stay <= 0.5 (real part), and NO
coefficient is negligible (MIN_COEF): a dropped, doubled or misplaced term moves the answer by orders of magnitude more
than the tolerance, which a uniform(-1, 1) draw does not guarantee (its smallest entry can be 1e-9)."""
import numpy as np
import scipy.sparse as sp

from util import dense_block, rand_tri, synth_level

# groups per block.  0: the empty block (g0 == g1); 1-3: waves of k_spmm_tile4 without groups; 3 / 4 and 7 / 8: the look-ahead
# depths (operands, source indices); 8 / 9 and 16 / 17: the trip boundary of k_spmm_tile; 28 ... 37: 7, 8 and 9 groups per wave
# of k_spmm_tile4 (29, 33, 37: one wave more than the others); 61 ... 68: 16 and 17 per wave, a third trip
G_LADDER = (0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 28, 29, 31, 32, 33, 35, 36, 37, 61, 64, 65, 68)
# nonzeros per row.  0: the empty row; 7 / 8 / 9, 15 / 16 / 17: the 8-unroll of k_spmm_epi_narrow and the gather batches of the
# stream; 63 / 64 / 65, 127 / 128 / 129: the item boundary of spmm_stream_r64 (row_done, k_c += 64); 200: four items
ROW_NNZ = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)
PAIR_CLASSES = (0, 1, 64, 65, 129)
PAIRS = tuple((a, b) for a in PAIR_CLASSES for b in PAIR_CLASSES) + ((200, 0), (0, 200))  # (row w, row w + pairs_at)
PAIRS_AT = 16384  # waves of k_spmm_epi at 64 columns (engine.hip grid_for: 4,096 workgroups of four)
MIN_COEF = 0.5 * 0.5 / 272  # (272 = 4 * 68 distinct columns: the longest row either ladder can make)


def _valued(rows, cols, shape, rng, dtype):
    """CSR matrix on the pattern with the value law of the module docstring."""
    A = sp.csr_matrix((np.ones(len(rows)), (np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64))), shape=shape)
    A.sort_indices()
    assert A.nnz == len(rows)  # (no entry twice)
    cnt = np.diff(A.indptr)
    scale = np.repeat(0.5 / np.maximum(cnt, 4), cnt)

    def draw():
        return rng.choice([-1.0, 1.0], A.nnz) * rng.uniform(0.5, 1.0, A.nnz) * scale

    data = draw()
    if np.dtype(dtype).kind == "c":
        data = data + 1j * draw()
    return sp.csr_matrix((data.astype(dtype), A.indices, A.indptr), shape=shape)


def ladder_coupling(nrows, ncols, rng, rb=1, dtype=np.float64):
    """Block b (rows 16 rb b ...) has D = 4 G - (b // 24) % 4 distinct columns, G = G_LADDER[b % 24] (none for G = 0): a
    random D-subset of the columns, each kept by every row with probability 0.75, repaired so that every chosen column has
    an entry."""
    brows = 16 * rb
    rows, cols = [], []
    for b in range((nrows + brows - 1) // brows):
        G = G_LADDER[b % len(G_LADDER)]
        if G == 0:
            continue
        D = 4 * G - (b // len(G_LADDER)) % 4
        r0, r1 = brows * b, min(nrows, brows * b + brows)
        cs = np.sort(rng.choice(ncols, size=D, replace=False))
        mask = rng.random((r1 - r0, D)) < 0.75
        for j in np.nonzero(~mask.any(axis=0))[0]:
            mask[rng.integers(r1 - r0), j] = True
        ii, jj = np.nonzero(mask)
        rows.extend(r0 + ii)
        cols.extend(cs[jj])
    return _valued(rows, cols, (nrows, ncols), rng, dtype)


def row_classes(nrows, pairs_at=None):
    """Nonzeros per row of row_ladder_coupling, -1 for a thin row (2-4 nonzeros).  The ladder takes the first 15 k rows with
    k = 3 nrows // 800: even with four nonzeros in every thin row the block has fewer than 8 nrows nonzeros and never
    qualifies for tiles.  The pairs overwrite rows 0 ... 26 and pairs_at ... pairs_at + 26."""
    cls = np.full(nrows, -1)
    k = max(1, 3 * nrows // 800)
    cls[:15 * k] = np.tile(ROW_NNZ, k)
    if pairs_at is not None:
        assert pairs_at + len(PAIRS) <= nrows and len(PAIRS) <= 30 and 45 <= 15 * k <= pairs_at  # (whole cycles are left)
        for w, (a, b) in enumerate(PAIRS):
            cls[w], cls[pairs_at + w] = a, b
    return cls


def row_ladder_coupling(nrows, ncols, rng, pairs_at=None, dtype=np.float64):
    cls = row_classes(nrows, pairs_at)
    rows, cols = [], []
    for i, c in enumerate(cls):
        k = int(rng.integers(2, 5)) if c < 0 else int(c)
        rows.extend([i] * k)
        cols.extend(rng.choice(ncols, size=k, replace=False))
    A = _valued(rows, cols, (nrows, ncols), rng, dtype)
    assert A.nnz < 8 * nrows
    return A


def thin_coupling(nrows, ncols, rng, dtype=np.float64):
    """A plain thin block: 2-4 nonzeros in every row, the same value law."""
    rows, cols = [], []
    for i in range(nrows):
        k = int(rng.integers(2, 5))
        rows.extend([i] * k)
        cols.extend(rng.choice(ncols, size=k, replace=False))
    return _valued(rows, cols, (nrows, ncols), rng, dtype)


# ---- what the engine makes of a block, restated ------------------------------------------------------------------------
def _distinct(A, rb):
    A = sp.csr_matrix(A)
    A.sort_indices()
    brows = 16 * rb
    return [len(np.unique(A.indices[A.indptr[r0]:A.indptr[min(A.shape[0], r0 + brows)]])) for r0 in range(0, A.shape[0], brows)]


def tile_groups(A, rb=1):
    """host.hpp build_spmm_tiles: groups of four distinct columns per block of 16 rb rows."""
    return [(d + 3) // 4 for d in _distinct(A, rb)]


def tile_padding(A, rb=1):
    """repeated columns in the last group of every block that has groups"""
    return [(-d) % 4 for d in _distinct(A, rb) if d]


def tile_qualifies(A, rb=1):
    """engine.hip finalize: a block gets tiles with at least 64 rows, 8 nonzeros per row and 2 nonzeros per distinct
    (block, column) pair."""
    A = sp.csr_matrix(A)
    distinct = sum(_distinct(A, rb))
    return bool(A.shape[0] >= 64 and A.nnz >= 8 * A.shape[0] and distinct > 0 and A.nnz / distinct >= 2.0)


def coupling(lv, which):
    """E ((n - m) x m) or F (m x (n - m)) of a level, as CSR."""
    m, n = int(lv["m"]), int(lv["n"])
    shape = (n - m, m) if which == "E" else (m, n - m)
    return sp.csc_matrix((lv[which + "_vals"], lv[which + "_rowind"], lv[which + "_colptr"]), shape=shape).tocsr()


def adjoint_couplings(lv):
    """The blocks that take E's and F's place in the conjugate-transposed apply (import.hpp adjoint_level): F^H, E^H."""
    return sp.csr_matrix(coupling(lv, "F").conj().T), sp.csr_matrix(coupling(lv, "E").conj().T)


# ---- hierarchies --------------------------------------------------------------------------------------------------------
M_ONE, ND_ONE = 1169, 385  # 385 = 24 * 16 + 1: the ladder once and a one-row block; 1169 = 73 * 16 + 1 = 36 * 32 + 17


def _thin_tri(m, lower, rng, dtype, scale=0.3):
    """Strict triangle with about two nonzeros per row: util.rand_tri, and beyond 4,096 rows the same law drawn directly
    (4 m places of the square, one triangle of them kept -- scipy.sparse.random samples the m^2 places of the square
    without replacement and takes 13 s at 16,584 rows)."""
    if m <= 4096:
        return rand_tri(m, 4.0 / m, lower, rng, dtype=dtype)
    i, j = rng.integers(m, size=4 * m), rng.integers(m, size=4 * m)
    keep = i > j if lower else i < j
    A = sp.csr_matrix((np.ones(int(keep.sum())), (i[keep], j[keep])), shape=(m, m))  # (a place drawn twice is one entry)
    A.sort_indices()
    A.data = rng.uniform(-scale, scale, A.nnz)
    if np.dtype(dtype).kind == "c":
        A = A.astype(np.complex128)
        A.data = A.data + 1j * rng.uniform(-scale, scale, A.nnz)
    return A


def _one_level(E, F, rng, dtype):
    m, nd = M_ONE, ND_ONE
    lv = synth_level(m, m + nd, _thin_tri(m, True, rng, dtype), _thin_tri(m, False, rng, dtype), E, F, rng, dtype=dtype)
    lv["dense_n"], lv["dense"] = nd, dense_block(nd, 6.0, rng, dtype, scale=0.2)
    return [lv]


def tiles(dtype=np.float64, rb=1):
    """One level + dense block, 1,554 rows, E (385 x 1169) and F (1169 x 385) group ladders over blocks of 16 rb rows.  Under
    rb = 2 the second row tile of E's last block lies beyond the block's rows, that of F's last block holds one row."""
    rng = np.random.default_rng(61 + rb)
    E = ladder_coupling(ND_ONE, M_ONE, rng, rb, dtype)
    F = ladder_coupling(M_ONE, ND_ONE, rng, rb, dtype)
    return _one_level(E, F, rng, dtype)


def rows(dtype=np.float64):
    """The same sizes with row ladders for E and F."""
    rng = np.random.default_rng(64)
    E = row_ladder_coupling(ND_ONE, M_ONE, rng, dtype=dtype)
    F = row_ladder_coupling(M_ONE, ND_ONE, rng, dtype=dtype)
    return _one_level(E, F, rng, dtype)


LONG = dict(m0=600, n1=16884, m1=16584, nd=300)


def long_rows(dtype=np.float64):
    """Two levels + dense block, 17,484 rows: E of level 0 (16,884 x 600) and F of level 1 (16,584 x 300) are row ladders of
    more than 16,384 rows with the pairs; F of level 0 and E of level 1 are thin."""
    rng = np.random.default_rng(65)
    m0, n1, m1, nd = LONG["m0"], LONG["n1"], LONG["m1"], LONG["nd"]
    lv0 = synth_level(m0, m0 + n1, _thin_tri(m0, True, rng, dtype), _thin_tri(m0, False, rng, dtype),
                      row_ladder_coupling(n1, m0, rng, PAIRS_AT, dtype), thin_coupling(m0, n1, rng, dtype), rng, dtype=dtype)
    lv1 = synth_level(m1, n1, _thin_tri(m1, True, rng, dtype), _thin_tri(m1, False, rng, dtype),
                      thin_coupling(nd, m1, rng, dtype), row_ladder_coupling(m1, nd, rng, PAIRS_AT, dtype), rng, dtype=dtype)
    lv1["dense_n"], lv1["dense"] = nd, dense_block(nd, 6.0, rng, dtype, scale=0.2)
    return [lv0, lv1]


HIERS = {
    "tiles": lambda: tiles(np.float64),
    "tiles2": lambda: tiles(np.float64, rb=2),
    "tilesz": lambda: tiles(np.complex128),
    "rows": lambda: rows(np.float64),
    "rowsz": lambda: rows(np.complex128),
    "long_rows": lambda: long_rows(np.float64),
    "long_rowsz": lambda: long_rows(np.complex128),
}
WIDE = 100  # columns of the shared batch
_cache = {}


def levels_of(name):
    if ("levels", name) not in _cache:
        levels = HIERS[name]()
        _cache[("levels", name)] = (levels, np.complex128 if name.endswith("z") else np.float64)
    return _cache[("levels", name)]


def hier(name, products=False):
    """levels, the 100-column batch of test_gpu_variants.py and the oracle's answers (solve forwards and
    conjugate-transposed; products=True: M B and M^H B as well): once per hierarchy, never written to."""
    from oracle import orc
    from util import rand_rhs

    key = ("hier", name)
    if key not in _cache:
        levels, dtype = levels_of(name)
        B = rand_rhs(np.random.default_rng(41), (int(levels[0]["n"]), WIDE), dtype)
        O = orc.Oracle(levels, dtype=dtype)
        h = dict(name=name, levels=levels, dtype=dtype, B=B, O=O, Xo=O.solve_batch(B, threads=4),
                 XoT=O.solve_batch(B, threads=4, trans=True))
        for k in ("B", "Xo", "XoT"):
            h[k].setflags(write=False)
        _cache[key] = h
    h = _cache[key]
    if products and "Yo" not in h:
        h["Yo"] = h["O"].mmultiply_batch(h["B"], rank=-1)  # (rank -1 on both sides, as test_gpu_product.py)
        h["YoT"] = h["O"].mmultiply_batch(h["B"], rank=-1, trans=True)
        h["Yo"].setflags(write=False), h["YoT"].setflags(write=False)
    return h


def colerr(X, Xo):
    """largest relative error of a column against the same column of the reference (max norm)"""
    return float(max(np.abs(X[:, c] - Xo[:, c]).max() / max(np.abs(Xo[:, c]).max(), 1e-300) for c in range(X.shape[1])))


# ---- the apply, restated (prec_solve of the reference with unit triangles) ------------------------------------------------
def restate(levels, B, extended=True):
    """X = M^{-1} B level by level:

        y = (s B)[p];  y1 = U^-1 D^-1 L^-1 y[:m];  z2 = child(y[m:] - E y1);  y1 = U^-1 D^-1 L^-1 (y[:m] - F z2)
        X = t [y1; z2][q_inv]

    child = the next level, or the dense block.  extended=True accumulates everything in np.longdouble (dense triangles,
    substitution row by row; the dense block by a float64 LU with two steps of refinement in longdouble) -- for the
    one-level hierarchies.  extended=False: float64 with scipy's sparse triangular solves -- for long_rows, whose
    triangles have 16,584 rows."""
    import scipy.linalg as sla
    from scipy.sparse.linalg import spsolve_triangular

    z = any(np.iscomplexobj(lv["L_vals"]) for lv in levels) or np.iscomplexobj(B)
    if extended:
        ft = np.clongdouble if z else np.longdouble
    else:
        ft = np.complex128 if z else np.float64

    def level(l, b):
        lv = levels[l]
        m, n = int(lv["m"]), int(lv["n"])
        nd = n - m
        L = sp.csc_matrix((lv["L_vals"], lv["L_rowind"], lv["L_colptr"]), shape=(m, m)).tocsr()
        U = sp.csc_matrix((lv["U_vals"], lv["U_rowind"], lv["U_colptr"]), shape=(m, m)).tocsr()
        E, F = coupling(lv, "E"), coupling(lv, "F")
        d = np.asarray(lv["d"]).astype(ft)[:, None]
        if extended:
            Ld, Ud = L.toarray().astype(ft), U.toarray().astype(ft)
            Ed, Fd = E.toarray().astype(ft), F.toarray().astype(ft)

            def ldu(y):
                y = y.copy()
                for i in range(1, m):
                    y[i] -= Ld[i, :i] @ y[:i]
                y /= d
                for i in range(m - 2, -1, -1):
                    y[i] -= Ud[i, i + 1:] @ y[i + 1:]
                return y

            mulE, mulF = (lambda v: Ed @ v), (lambda v: Fd @ v)
        else:
            I = sp.identity(m, format="csr")
            Lu, Uu = (L + I).tocsr(), (U + I).tocsr()

            def ldu(y):
                y = spsolve_triangular(Lu, y, lower=True, unit_diagonal=True) / d
                return spsolve_triangular(Uu, y, lower=False, unit_diagonal=True)

            mulE, mulF = (lambda v: E @ v), (lambda v: F @ v)
        y = (np.asarray(lv["s"]).astype(ft)[:, None] * b.astype(ft))[lv["p"]]
        y1 = ldu(y[:m])
        y2 = y[m:] - mulE(y1)
        if l + 1 < len(levels):
            z2 = level(l + 1, y2)
        else:
            D = np.asarray(lv["dense"]).reshape(nd, nd, order="F")
            lu = sla.lu_factor(D)
            w = np.complex128 if z else np.float64
            z2 = sla.lu_solve(lu, y2.astype(w)).astype(ft)
            for _ in range(2 if extended else 0):
                z2 = z2 + sla.lu_solve(lu, (y2 - D.astype(ft) @ z2).astype(w)).astype(ft)
        y1 = ldu(y[:m] - mulF(z2))
        return np.asarray(lv["t"]).astype(ft)[:, None] * np.vstack([y1, z2])[lv["q_inv"]]

    return level(0, np.asarray(B))
