"""The group ladder of test_gpu_spmm_ahead.py (GPU) and test_spmm_ahead_host.py (CPU: every count arrives).

k_spmm_tile / k_spmm_tile4 multiply a wave's column groups in batches of BU, two batches per trip of their loop, with
the source ids requested two batches ahead and the operands one batch ahead; the remainder (at most one batch) is
multiplied behind the loop.  What a wave does therefore changes at BU groups (one batch or two) and at 2 BU (the loop
runs or not; with more, whether a remainder is left), and schur_edges_util.G_LADDER was built around other constants
(look-aheads of 3 and 7, trips of 8).  The constants (kernels.hip.hpp SpmmAhead):

    k_spmm_tile   BU = 4 (16-row blocks), 2 (32-row blocks)       a wave walks all of a block's groups
    k_spmm_tile4  BU = 2 (16- and 32-row blocks)                  wave w walks groups w, w + 4, ... of a block

AHEAD_LADDER straddles every c in C = {2, 3, 4, 6, 8} (every BU and 2 BU above, and those of the batch sizes 3 and 4 that
k_spmm_tile4 was also measured with):
 * per block, for the per-wave kernel: c - 1, c, c + 1 groups -- 1 ... 9, all of them;
 * per wave, for k_spmm_tile4: 4 c - 4 and 4 c groups give every wave c - 1 and c, 4 c - 3 and 4 c + 1 give wave 0 one
   group more than the others (c against c - 1, c + 1 against c), 4 c + 4 gives every wave c + 1;
 * 0: the empty block; 1, 2, 3: waves of k_spmm_tile4 without groups; 68: 17 groups per wave, several trips and a remainder.
It has the 24 entries of G_LADDER, so the blocks of schur_edges_util.tiles walk it in the same way: E (385 x 1,169) once
and a one-row block, F (1,169 x 385) three times with paddings 0 ... 3 of the last group."""
import numpy as np

import schur_edges_util as se

BU_TILE = {1: 4, 2: 2}   # k_spmm_tile, by row tiles per block
BU_TILE4 = {1: 2, 2: 2}  # k_spmm_tile4
CONSTANTS = (2, 3, 4, 6, 8)
AHEAD_LADDER = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32, 33, 36, 68)
assert len(AHEAD_LADDER) == len(se.G_LADDER) and max(AHEAD_LADDER) == max(se.G_LADDER)  # (MIN_COEF holds: 272 columns at most)


def wave_groups(G):
    """groups of the four waves of k_spmm_tile4 in a block of G groups (wave w: w, w + 4, ...)"""
    return tuple((G - w + 3) // 4 if G > w else 0 for w in range(4))


def ladder_coupling(nrows, ncols, rng, rb=1, dtype=np.float64):
    """schur_edges_util.ladder_coupling on AHEAD_LADDER: block b (rows 16 rb b ...) has D = 4 G - (b // 24) % 4 distinct
    columns, G = AHEAD_LADDER[b % 24], each kept by every row with probability 0.75, every chosen column with an entry."""
    brows = 16 * rb
    rows, cols = [], []
    for b in range((nrows + brows - 1) // brows):
        G = AHEAD_LADDER[b % len(AHEAD_LADDER)]
        if G == 0:
            continue
        D = 4 * G - (b // len(AHEAD_LADDER)) % 4
        r0, r1 = brows * b, min(nrows, brows * b + brows)
        cs = np.sort(rng.choice(ncols, size=D, replace=False))
        mask = rng.random((r1 - r0, D)) < 0.75
        for j in np.nonzero(~mask.any(axis=0))[0]:
            mask[rng.integers(r1 - r0), j] = True
        ii, jj = np.nonzero(mask)
        rows.extend(r0 + ii)
        cols.extend(cs[jj])
    return se._valued(rows, cols, (nrows, ncols), rng, dtype)


def ahead_levels(rb=1):
    """One level + dense block, 1,554 rows (the sizes of schur_edges_util.tiles): E and F walk AHEAD_LADDER over blocks of
    16 rb rows."""
    rng = np.random.default_rng(81 + rb)
    E = ladder_coupling(se.ND_ONE, se.M_ONE, rng, rb)
    F = ladder_coupling(se.M_ONE, se.ND_ONE, rng, rb)
    return se._one_level(E, F, rng, np.float64)


_cache = {}


def hier(name):
    """levels, the 100-column batch rand_rhs(default_rng(41)) and the oracle's two answers, once per hierarchy and never
    written to: "ahead" / "ahead2" here, every other name from schur_edges_util.hier."""
    if name not in ("ahead", "ahead2"):
        return se.hier(name)
    if name not in _cache:
        from oracle import orc
        from util import rand_rhs

        levels = ahead_levels(2 if name == "ahead2" else 1)
        B = rand_rhs(np.random.default_rng(41), (int(levels[0]["n"]), se.WIDE))
        O = orc.Oracle(levels)
        h = dict(name=name, levels=levels, dtype=np.float64, B=B, Xo=O.solve_batch(B, threads=4),
                 XoT=O.solve_batch(B, threads=4, trans=True))
        for k in ("B", "Xo", "XoT"):
            h[k].setflags(write=False)
        _cache[name] = h
    return _cache[name]
