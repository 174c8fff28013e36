"""Shared helpers for the tests: fixture loading and synthetic matrices (no reference access)."""
import os

import numpy as np
import scipy.sparse as sp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HIER_NAMES = ["p2d_5", "p2d_30", "p2d_64_deep", "p2d_100_tuned", "p3d_12", "cd2d_48", "demo_A", "young1c",
              "p2d_32_symm", "herm_24_symm",  # is_symm factorizations (last level = SYEIG)
              "p2d_30_lup",  # the reference built with HIF_DENSE_MODE=0 (last level = LUP)
              "kkt_26"]  # complex saddle point (BASELINE config 5's generator at 2,028 rows)
LEVEL_KEYS = ["m", "n", "dense_n", "dense_rank", "dense_symm", "spd", "dense_lup", "d", "s", "t", "p", "p_inv", "q", "q_inv", "dense"] + [
    f"{a}_{b}" for a in "LUEF" for b in ("colptr", "rowind", "vals")]


def load_hier(name):
    """-> (levels, data): levels in the oracle.orc format, data = the other fixture arrays."""
    z = np.load(os.path.join(GOLDEN, f"hier_{name}.npz"))
    nl = int(z["nlevels"])
    levels = []
    for l in range(nl):
        lv = {}
        for k in LEVEL_KEYS:
            key = f"L{l}_{k}"
            if key in z.files:
                v = z[key]
                lv[k] = int(v) if v.ndim == 0 else v
        levels.append(lv)
    data = {k: z[k] for k in z.files if not k.startswith("L") or not k[1].isdigit()}
    return levels, data


def poisson2d(nx, ny=None):
    ny = ny or nx
    Tx = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx), format="csr")
    Ty = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(ny, ny), format="csr")
    A = (sp.kron(sp.identity(ny), Tx) + sp.kron(Ty, sp.identity(nx))).tocsr()
    A.sort_indices()
    return A


def stokes_kkt(nx, omega=0.1, eps=1e-8):
    """BASELINE config 5: the SuiteSparse saddle point cannot be fetched offline; its stand-in is the
    complex Stokes-like KKT system

        [ K + i*omega*M    B^T   ]      K = vector Laplacian (5-pt, per velocity component) on an nx x nx grid,
        [ B               -eps*I ]      M = lumped mass (identity), B = discrete divergence (forward differences),

    omega = 0.1, eps = 1e-8: 3 nx^2 rows, complex symmetric, indefinite, with a (nearly) zero (2,2) block -- the
    factorization defers the pressure rows into the Schur complements.  nx = 816 gives 1,997,568 rows."""
    n1 = nx * nx
    I = sp.identity(nx, format="csr")
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx), format="csr")
    lap = sp.kron(I, T) + sp.kron(T, I)
    K = sp.block_diag([lap, lap]).astype(np.complex128) + 1j * omega * sp.identity(2 * n1)
    D = sp.diags([-1.0, 1.0], [0, 1], shape=(nx, nx), format="csr")
    B = sp.hstack([sp.kron(I, D), sp.kron(D, I)]).tocsr()
    A = sp.bmat([[K, B.T], [B, -eps * sp.identity(n1)]], format="csr").astype(np.complex128)
    A.sort_indices()
    return A


def relerr(x, ref):
    return float(np.abs(x - ref).max() / max(np.abs(ref).max(), 1e-300))


# ---- synthetic hierarchies (no factorization produces them): the generators of test_gpu_synthetic.py, test_gpu_ls_band.py and
# test_gpu_variants.py.  dtype=np.complex128 gives every value an imaginary part of its own.
def ccs(A, dtype=np.float64):
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(dtype)


def _imag(A, rng, dtype, scale):
    """A with independent imaginary parts on its pattern (complex dtype), A itself otherwise."""
    A = sp.csr_matrix(A)
    if np.dtype(dtype).kind != "c":
        return A
    return sp.csr_matrix((A.data + 1j * rng.uniform(-scale, scale, A.nnz), A.indices, A.indptr), shape=A.shape)


def synth_level(m, n, L, U, E, F, rng, with_F=True, dtype=np.float64):
    lv = dict(m=m, n=n)
    z = np.dtype(dtype).kind == "c"
    for k, M in (("L", L), ("U", U), ("E", E), ("F", F)):
        if z and not np.iscomplexobj(M.data if sp.issparse(M) else M):  # (triangles from rand_tri already are complex)
            M = _imag(M, rng, dtype, 0.5)
        cp, ri, v = ccs(M, dtype)
        lv[k + "_colptr"], lv[k + "_rowind"], lv[k + "_vals"] = cp, ri, v
    if not with_F:
        lv["F_colptr"], lv["F_rowind"], lv["F_vals"] = np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, dtype)
    lv["d"] = rng.uniform(0.5, 2.0, m) * rng.choice([-1.0, 1.0], m)
    if z:
        lv["d"] = lv["d"] * np.exp(1j * rng.uniform(-1.0, 1.0, m))
    lv["s"], lv["t"] = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n)
    lv["p"] = rng.permutation(n).astype(np.int32)
    lv["q"] = rng.permutation(n).astype(np.int32)
    lv["p_inv"] = np.argsort(lv["p"]).astype(np.int32)
    lv["q_inv"] = np.argsort(lv["q"]).astype(np.int32)
    return lv


def rand_tri(m, density, lower, rng, scale=0.3, dtype=np.float64):
    A = sp.random(m, m, density=density, random_state=np.random.RandomState(rng.integers(1 << 30)), format="csr")
    A.data = rng.uniform(-scale, scale, A.nnz)
    if np.dtype(dtype).kind == "c":
        A = A.astype(np.complex128)
        A.data = A.data + 1j * rng.uniform(-scale, scale, A.nnz)
    return sp.tril(A, -1) if lower else sp.triu(A, 1)


def dense_block(nd, shift, rng, dtype=np.float64, scale=1.0):
    """Column-major values of a dense last level: scale * normal + shift * I."""
    D = rng.normal(size=(nd, nd))
    if scale != 1.0:
        D *= scale
    D = D + shift * np.eye(nd)
    if np.dtype(dtype).kind == "c":
        D = D + 1j * scale * rng.normal(size=(nd, nd))
    return D.astype(dtype).ravel(order="F")


def rand_rhs(rng, shape, dtype=np.float64):
    B = rng.uniform(-1, 1, size=shape)
    if np.dtype(dtype).kind == "c":
        B = B + 1j * rng.uniform(-1, 1, size=shape)
    return B.astype(dtype)


def forest(m, leaves, spine, rng, lower):
    """Strict triangle made of blocks of `leaves` rows without entries and `spine` rows that read 2-3 leaves and 0-2 earlier
    spine rows of their block (now and then a row of an earlier block): components of ~leaves + spine rows, two thirds of
    them pure sources -- the shape of level 0 of a PDE hierarchy, with more sources than one chunk holds."""
    rows, cols = [], []
    blk = leaves + spine
    for b0 in range(0, m, blk):
        nl = min(leaves, m - b0)
        for i in range(b0 + nl, min(m, b0 + blk)):
            src = set(int(b0 + rng.integers(nl)) for _ in range(2 + int(rng.integers(2))))
            if i > b0 + nl:
                src |= set(int(b0 + nl + rng.integers(i - b0 - nl)) for _ in range(int(rng.integers(3))))
            if b0 > 0 and rng.integers(5) == 0:
                src.add(int(rng.integers(b0)))
            for j in src:
                rows.append(i), cols.append(j)
    A = sp.csr_matrix((rng.uniform(-0.4, 0.4, len(rows)), (rows, cols)), shape=(m, m))
    if lower:
        return A
    # the mirrored pattern as a strict upper triangle (row i reads LATER rows)
    P = sp.csr_matrix((np.ones(m), (np.arange(m), m - 1 - np.arange(m))), shape=(m, m))
    return (P @ A @ P).tocsr()


def forest_levels():
    """One level of 7,000 rows (6,300 leading) whose triangles are forests, with E, F and a dense last level."""
    rng = np.random.default_rng(11)
    n0, m0 = 7000, 6300
    nd = n0 - m0
    lv = dict(m=m0, n=n0)
    E = sp.random(nd, m0, density=0.004, random_state=np.random.RandomState(3), format="csr")
    F = sp.random(m0, nd, density=0.002, random_state=np.random.RandomState(4), format="csr")
    for k, M in (("L", forest(m0, 120, 60, rng, True)), ("U", forest(m0, 120, 60, rng, False)), ("E", E), ("F", F)):
        lv[k + "_colptr"], lv[k + "_rowind"], lv[k + "_vals"] = ccs(M)
    lv["d"] = rng.uniform(0.5, 2.0, m0) * rng.choice([-1.0, 1.0], m0)
    lv["s"], lv["t"] = rng.uniform(0.5, 2.0, n0), rng.uniform(0.5, 2.0, n0)
    lv["p"] = rng.permutation(n0).astype(np.int32)
    lv["q"] = rng.permutation(n0).astype(np.int32)
    lv["p_inv"] = np.argsort(lv["p"]).astype(np.int32)
    lv["q_inv"] = np.argsort(lv["q"]).astype(np.int32)
    D = rng.normal(size=(nd, nd)) + 6.0 * np.eye(nd)
    lv["dense_n"], lv["dense"] = nd, D.ravel(order="F")
    return [lv]


def clustered_tri(m, block, per_row, crown, rng, scale=0.15, cross=0.007):
    """Strict lower triangle of independent clusters: row i of a `block`-row cluster reads up to `per_row` earlier rows of its
    cluster (>= 4 nonzeros per row on average, components of `block` rows: what the planner gives dense-own component bands),
    now and then a row of an earlier cluster, and the last `crown` rows read rows from anywhere before them (the merged top
    of an elimination forest: no component holds them, they end up in the block-dense rest / the level's top operator)."""
    rows, cols = [], []
    body = m - crown
    for b0 in range(0, body, block):
        for i in range(b0 + 1, min(body, b0 + block)):
            src = set(int(b0 + x) for x in rng.choice(i - b0, size=min(i - b0, per_row), replace=False))
            if b0 > 0 and rng.random() < cross:
                src.add(int(rng.integers(b0)))
            for j in src:
                rows.append(i), cols.append(j)
    for i in range(body, m):
        for j in set(int(x) for x in rng.integers(i, size=per_row)):
            rows.append(i), cols.append(j)
    return sp.csr_matrix((rng.uniform(-scale, scale, len(rows)), (rows, cols)), shape=(m, m))


def transposed_pattern(L, rng, scale=0.15):
    """Strict upper triangle on the transposed pattern of L (a structurally symmetric pair, as a PDE gives) with values of
    its own."""
    U = sp.csr_matrix(L.T)
    U.data = rng.uniform(-scale, scale, U.nnz)
    return U


def shared_coupling(nrows, ncols, rng, scale=0.1):
    """Coupling block whose rows share columns, and whose columns share rows: every group of 16 rows is dense on one group
    of 16 columns (what the tiled Schur products are built for: >= 8 nonzeros per row and each column of a 16-row block
    used 16 times -- in the block and, for the adjoint apply, in its transpose)."""
    rows, cols = [], []
    for r0 in range(0, nrows, 16):
        c0 = 16 * int(rng.integers(max(1, ncols // 16)))
        for i in range(r0, min(nrows, r0 + 16)):
            for j in range(c0, min(ncols, c0 + 16)):
                rows.append(i), cols.append(j)
    return sp.csr_matrix((rng.uniform(-scale, scale, len(rows)), (rows, cols)), shape=(nrows, ncols))


# ---- shape ladders (test_shape_ladders_host.py checks what the planner makes of them; test_gpu_variants.py, test_gpu_ls_band.py
# and test_gpu_wide_batch.py solve them)
def ladder_tri(sizes, per_row, rng, scale=0.15):
    """Strict lower triangle of independent clusters of the given sizes, one after the other: row i of a cluster reads
    min(i, per_row) earlier rows of it (clustered_tri without crown and cross entries, every cluster a size of its own).
    With scale 0.15 and per_row = 6 a row's absolute sum stays below 0.9: the inverse of every cluster's unit triangle is
    bounded by 1 / (1 - 0.9) = 10, the regime clustered_tri's hierarchies are solved in."""
    rows, cols = [], []
    b0 = 0
    for sz in sizes:
        for i in range(1, sz):
            for x in rng.choice(i, size=min(i, per_row), replace=False):
                rows.append(b0 + i), cols.append(b0 + int(x))
        b0 += sz
    return sp.csr_matrix((rng.uniform(-scale, scale, len(rows)), (rows, cols)), shape=(b0, b0))


LADDER_SIZES = tuple(range(9, 129))


def ladder_levels(dtype=np.float64, seed=51):
    """One level + dense block, 8,520 rows: L is a ladder of 120 clusters of 9, 10, ... 128 rows in shuffled order with up to
    six nonzeros per row, U its transposed pattern -- every strip count, every tile remainder and every operand padding of
    the dense-own component kernels once per triangle."""
    rng = np.random.default_rng(seed)
    sizes = rng.permutation(LADDER_SIZES)
    m0, nd = int(sizes.sum()), 300
    n0 = m0 + nd
    L = ladder_tri(sizes, 6, rng)
    lv = synth_level(m0, n0, L, transposed_pattern(L, rng), shared_coupling(nd, m0, rng),
                     sp.random(m0, nd, density=0.002, random_state=np.random.RandomState(4), format="csr"), rng, dtype=dtype)
    lv["dense_n"], lv["dense"] = nd, dense_block(nd, 6.0, rng, dtype, scale=0.2)
    return [lv]


def shape_forest(shapes, rng, outside=()):
    """Strict lower triangle of components of prescribed shape, in two tiers.  shapes: (ns, nd) pairs, tier 1 -- ns leaves
    (rows without entries) followed by nd spine rows; every leaf is read by some spine row, every spine row but the first
    reads an earlier spine row 1 to 6 rows back (the component stays whole, its depth varies) and up to two more leaves;
    nd = 0 gives ns rows that belong to nothing.  outside: (ns, nd, leaf_out, spine_out) tuples, tier 2 behind tier 1 -- the
    same components, whose leaves read leaf_out >= 1 and whose spine rows read spine_out rows of tier 1.  The first
    outside row of a tier-2 leaf is the deepest row of one of the largest tier-1 components (the tier-2 components take
    them in turn): a planner that merges components up to a row limit cannot place the leaf before that whole component,
    so tier 2 is planned behind tier 1 and its entries into tier 1 are outside entries of the second band.  Values: +-0.4 for rows of at most five entries,
    +-2 / entries beyond (absolute row sums <= 2, no inverses are formed of these triangles).
    -> (L, comps) with comps = [(tier, first row, ns, nd)]."""
    rows, cols, comps = [], [], []
    at = 0
    anchors = []  # (rows, deepest row) of the tier-1 components

    def component(ns, nd, leaf_out, spine_out, tier, m1):
        nonlocal at
        b0 = at
        anchor = big[len(comps) % len(big)] if tier == 2 else None
        owner = [[] for _ in range(nd)]
        for l in range(ns):  # every leaf is read by a spine row: the first ones in turn, the rest at random
            if nd:
                owner[l % nd if l < nd else int(rng.integers(nd))].append(l)
        depth = [0] * (ns + nd)
        for l in range(ns if tier == 2 else 0):
            src = {anchor} | set(int(x) for x in rng.integers(m1, size=leaf_out - 1))
            while len(src) < leaf_out:
                src.add(int(rng.integers(m1)))
            for j in src:
                rows.append(b0 + l), cols.append(j)
        for k in range(nd):
            src = set(owner[k]) | set(int(x) for x in rng.integers(ns, size=int(rng.integers(3))) if ns)
            if k:
                src.add(ns + k - 1 - int(rng.integers(min(k, 6))))
            depth[ns + k] = 1 + max([depth[j] for j in src], default=-1)
            for j in src:
                rows.append(b0 + ns + k), cols.append(b0 + j)
            out = set()
            while tier == 2 and len(out) < spine_out:
                out.add(int(rng.integers(m1)))
            for j in out:
                rows.append(b0 + ns + k), cols.append(j)
        if tier == 1 and nd:
            anchors.append((ns + nd, b0 + int(np.argmax(depth))))
        comps.append((tier, b0, ns, nd))
        at += ns + nd

    for ns, nd in shapes:
        component(ns, nd, 0, 0, 1, 0)
    m1 = at
    big = [row for n, row in anchors if n == max(a[0] for a in anchors)]
    for ns, nd, leaf_out, spine_out in outside:
        component(ns, nd, leaf_out, spine_out, 2, m1)
    cnt = np.bincount(rows, minlength=at)
    vals = np.array([rng.uniform(-1, 1) * (0.4 if cnt[i] <= 5 else 2.0 / cnt[i]) for i in rows])
    return sp.csr_matrix((vals, (rows, cols)), shape=(at, at)), comps


# tier 1 of the shape hierarchy: (sources, dependent rows) by the classes k_band_ls / k_band_us branch on -- dependent rows 0,
# 1, 15, 16, 17, 64, 65; sources 0, 1, 15 mod 16; sources = one 64-row chunk, one more, two chunks; the 192-row ones anchor tier 2
SHAPES_TIER1 = ((40, 0), (31, 1), (17, 1), (33, 15), (15, 15), (48, 16), (16, 16), (1, 16), (47, 17), (64, 17), (64, 64), (65, 64),
                (65, 33), (100, 50), (120, 60), (128, 64), (127, 65), (128, 64), (127, 65), (128, 1), (113, 15), (96, 65))
# tier 2: (sources, dependent rows, outside rows per source, per dependent row) -- 129 ... 144 sources (three chunks of 48),
# wave runs of 4, exactly 64 and 80 outside entries on the sources' side, 80 on the dependent rows' side
SHAPES_TIER2 = ((140, 40, 1, 0), (64, 32, 1, 0), (64, 32, 16, 0), (64, 32, 20, 0), (64, 32, 1, 40), (96, 48, 2, 1), (130, 30, 3, 2),
                (144, 48, 1, 1), (129, 63, 1, 0), (33, 15, 5, 3))


def _fill_shapes(shapes, rows, draw):
    shapes = list(shapes)
    while sum(s[0] + s[1] for s in shapes) < rows:
        shapes.append(draw())
    return shapes


def shapes_levels(dtype=np.float64, seed=52, tier1=4800, tier2=2500, ns_max=(128, 140), classes=(SHAPES_TIER1, SHAPES_TIER2)):
    """One level + dense block: L is a shape_forest of the classes above filled up with random shapes to tier1 + tier2 rows
    (tier 2 has to exceed one block of the dense chain, 2,048 rows, to become a component band), U its transposed
    pattern, thin E and F."""
    rng = np.random.default_rng(seed)

    def draw1():
        ns = int(rng.integers(16, ns_max[0] + 1))
        return ns, int(rng.integers(1, min(64, 192 - ns) + 1))

    def draw2():
        ns = int(rng.integers(32, ns_max[1] + 1))
        return ns, int(rng.integers(8, min(48, 192 - ns) + 1)), int(rng.integers(1, 4)), int(rng.integers(3))

    L, _ = shape_forest(_fill_shapes(classes[0], tier1, draw1), rng, _fill_shapes(classes[1], tier2, draw2) if tier2 else ())
    m0, nd = L.shape[0], 300
    n0 = m0 + nd
    rs = np.random.RandomState
    lv = synth_level(m0, n0, L, transposed_pattern(L, rng, scale=0.4), sp.random(nd, m0, density=0.004, random_state=rs(3), format="csr"),
                     sp.random(m0, nd, density=0.002, random_state=rs(4), format="csr"), rng, dtype=dtype)
    lv["dense_n"], lv["dense"] = nd, dense_block(nd, 6.0, rng, dtype, scale=0.2)
    return [lv]


def short_shapes_levels(ns_top, seed):
    """2,100 rows of one tier with at most ns_top sources per component (one component band per triangle, no second tier):
    the chunk counts of k_band_ls that the 128-source components of shapes_levels cannot reach."""
    tier1 = ((ns_top, 40), (ns_top, 1), (ns_top - 15, 64), (ns_top - 31, 20), (ns_top, 17), (33, 15))
    return shapes_levels(seed=seed, tier1=2100, tier2=0, ns_max=(ns_top, 0), classes=(tier1, ()))
