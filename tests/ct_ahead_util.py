"""The fixture of test_ct_ahead_host.py and test_gpu_ct_ahead.py: one level + a small dense block whose second L band is a
tile band (k_band_ct) with a PRESCRIBED number of coefficient tiles per 16-row strip.

Phase 1 of k_band_ct walks a strip's tiles in batches of BU = 8 / 4 / 2 tiles (one / two / four column tiles per
workgroup), two batches per trip of its loop, the requests running ahead of the products.  What its loop distinguishes is
the tile count T of a strip against the batch size: T in {0, 1, BU - 1, BU, BU + 1, 2 BU - 1, 2 BU, 2 BU + 1, 3 BU + 2}
for the three batch sizes is TILE_COUNTS below.  A strip with T tiles reads D distinct older rows, T = ceil(D / 4); D is
chosen as 4 T - (T mod 4), so that the last tile of most strips is partly empty.

Tier 1 holds independent clusters of 128 rows (the sources; the first band).  Tier 2 holds the components under test, and
the rows of strip s of a component read, between them, exactly D_s distinct rows of tier 1.  How the planner
(host.hpp plan_bands_cd) is made to keep these components and strips as they are laid out here:

 * a row joins the pass being planned if the components of the rows it needs, and itself, stay within 128 rows: a tier-1
   cluster already has 128, so a row with an entry into tier 1 is deferred to the second pass, and with it every row that
   needs it -- the first row of every tier-2 component reads the last row of a tier-1 cluster (util.shape_forest anchors
   its second tier in this way), and every other row of the component reads the first one.  Tier 2 is the second band and
   its entries into tier 1 are the outside entries the tile format is cut from;
 * a component's rows are laid out in dependency-depth order, 16 to a strip: every row of a cluster reads the row before
   it, so depth grows with the row number and strip s is rows 16 s ... 16 s + 15 as numbered here;
 * a band of at most 96 workgroups at the end of L's plan would be taken into the level's top operator, and a band is
   only planned while more than 2,048 rows remain: tier 2 is the component set below three times, with other sources.

Every row reads up to six earlier rows of its cluster (dense-own components: the planner forms their inverses).  Shapes:
single-strip components of 16 and of 9 rows (one per tile count each; the one without tiles has no entry into tier 1 and
joins the first band), three-strip components with an empty strip between two others, 128-row components with eight
strips of different T.  U is the transposed pattern of L."""
import numpy as np
import scipy.sparse as sp

from util import dense_block, synth_level, transposed_pattern

TILE_COUNTS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 14, 15, 16, 17, 26)
BATCH_SIZES = (8, 4, 2)  # NCT = 1, 2, 4


def edge_tile_counts():
    """The tile counts at which a batch size changes what the loop does -- TILE_COUNTS, derived."""
    return sorted({t for bu in BATCH_SIZES for t in (0, 1, bu - 1, bu, bu + 1, 2 * bu - 1, 2 * bu, 2 * bu + 1, 3 * bu + 2)})


def sources_of(t):
    """Distinct older rows of a strip with t tiles: a multiple of four only where t is one (4, 8, 16)."""
    return 4 * t - (t % 4)


# tier 2, one entry per component: (rows, tiles of every strip)
THREE_STRIPS = ((1, 0, 26), (8, 0, 9), (17, 0, 4), (5, 0, 2), (16, 0, 15), (7, 0, 14), (3, 0, 1))
EIGHT_STRIPS = ((1, 0, 2, 3, 4, 5, 7, 8), (9, 14, 15, 16, 17, 26, 1, 0))
COMPONENTS = tuple([(16, (t,)) for t in TILE_COUNTS] + [(9, (t,)) for t in TILE_COUNTS]
                   + [(48 if k % 2 == 0 else 41, ts) for k, ts in enumerate(THREE_STRIPS)] + [(128, ts) for ts in EIGHT_STRIPS])
REPEATS = 3           # the set above, three times
TIER1_CLUSTERS = 16   # clusters of 128 rows
PER_ROW = 6


def ct_ahead_tri(rng):
    """-> (L, comps): the strict lower triangle and [(first row, rows, tiles per strip)] of the tier-2 components."""
    rows, cols, vals = [], [], []

    def cluster(b0, n):
        for i in range(1, n):  # the row before, the first row, and earlier rows at random: up to PER_ROW
            src = {i - 1, 0} | set(int(x) for x in rng.choice(i, size=min(i, PER_ROW - 2), replace=False))
            for x in sorted(src)[:PER_ROW] if len(src) <= PER_ROW else sorted(src):
                rows.append(b0 + i), cols.append(b0 + x), vals.append(rng.uniform(-0.15, 0.15))

    m1 = 128 * TIER1_CLUSTERS
    for c in range(TIER1_CLUSTERS):
        cluster(128 * c, 128)
    at, comps = m1, []
    shapes = [COMPONENTS[k] for _ in range(REPEATS) for k in rng.permutation(len(COMPONENTS))]
    for k, (n, tiles) in enumerate(shapes):
        cluster(at, n)
        anchor = 128 * (k % TIER1_CLUSTERS) + 127  # the last, deepest row of a tier-1 cluster
        for s, t in enumerate(tiles):
            r0, r1 = 16 * s, min(n, 16 * s + 16)
            d = sources_of(t)
            if d == 0:
                continue
            src = [anchor] if s == 0 else []
            while len(src) < d:
                j = int(rng.integers(m1))
                if j not in src:
                    src.append(j)
            # dealt over the strip's rows in turn, every source once (the anchor goes to the strip's first row)
            for q, j in enumerate(src):
                rows.append(at + r0 + q % (r1 - r0)), cols.append(j), vals.append(rng.uniform(-0.3, 0.3))
        comps.append((at, n, tuple(tiles)))
        at += n
    return sp.csr_matrix((vals, (rows, cols)), shape=(at, at)), comps


def ct_ahead_levels(seed=71):
    """One level + dense block (fewer than 6,000 rows).  -> (levels, comps)"""
    rng = np.random.default_rng(seed)
    L, comps = ct_ahead_tri(rng)
    m0, nd = L.shape[0], 200
    n0 = m0 + nd
    rs = np.random.RandomState
    lv = synth_level(m0, n0, L, transposed_pattern(L, rng), sp.random(nd, m0, density=0.004, random_state=rs(5), format="csr"),
                     sp.random(m0, nd, density=0.002, random_state=rs(6), format="csr"), rng)
    lv["dense_n"], lv["dense"] = nd, dense_block(nd, 6.0, rng, scale=0.2)
    assert n0 <= 6000
    return [lv], comps
