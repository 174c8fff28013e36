"""CPU: the inputs of test_gpu_schur_edges.py reach the classes that file claims to run, and its reference is pinned.

 * The group ladders (schur_edges_util.tiles): build_spmm_tiles, restated in numpy, makes every group count of G_LADDER
   out of E and F, every padding 0 ... 3 of a block's last group, and both blocks qualify for tiles under the three
   conditions of engine.hip.  E has 25 blocks of 16 rows (13 of 32): at rb = 1 it walks the ladder once on its own, at
   rb = 2 its 13 blocks reach the first 13 values and F (37 blocks of 32 rows) walks all of it, with paddings 0 and 1.
 * The row ladders (rows, long_rows): every class of ROW_NNZ occurs in every laddered block, every ordered pair of
   PAIRS sits in rows (w, w + 16,384) of both long blocks, and no block of these hierarchies qualifies for tiles.
 * No coefficient of any of these blocks is below MIN_COEF in modulus.
 * The oracle (oracle.orc.Oracle.solve_batch, the reference of every GPU assertion) agrees with an independent
   restatement of the apply (schur_edges_util.restate) to 1e-13 per column, ten times under the GPU bar of 1e-12.
   One-level hierarchies: the restatement accumulates in np.longdouble.  Measured: tiles 6.4e-16, tiles2 8.2e-16,
   tilesz 2.5e-15, rows 6.1e-16, rowsz 1.7e-15.  long_rows (triangles of 16,584 rows): float64 with scipy's sparse
   triangular solves holds the same bar; measured 4.2e-16 (real), 5.5e-16 (complex).

These are conditions on the INPUTS and on the reference: a change that moves a class away fails here."""
import numpy as np
import pytest

import schur_edges_util as se

ONE_LEVEL = ("tiles", "tiles2", "tilesz", "rows", "rowsz")
LADDERED = {"rows": ((0, "E"), (0, "F")), "rowsz": ((0, "E"), (0, "F")), "long_rows": ((0, "E"), (1, "F")),
            "long_rowsz": ((0, "E"), (1, "F"))}
NCOLS = 20  # columns of the shared batch the pin runs on


def _blocks(name):
    levels, _ = se.levels_of(name)
    return [(l, w, se.coupling(lv, w)) for l, lv in enumerate(levels) for w in "EF"]


@pytest.mark.parametrize("name,rb", [("tiles", 1), ("tilesz", 1), ("tiles2", 2)])
def test_group_ladder_reaches_every_count(name, rb):
    want = set(se.G_LADDER)
    assert 0 in want
    pads = set()
    for l, w, A in _blocks(name):
        g = se.tile_groups(A, rb)
        print(f"{name} {w}: {A.shape[0]} x {A.shape[1]}, {A.nnz} nonzeros, {len(g)} blocks of {16 * rb} rows, groups {sorted(set(g))}, "
              f"paddings {sorted(set(se.tile_padding(A, rb)))}")
        # (the generator's promise, block by block)
        assert g == [se.G_LADDER[b % 24] for b in range(len(g))]
        assert set(g) == set(se.G_LADDER[:min(24, len(g))])
        if w == "F" or rb == 1:  # (E under rb = 2 has 13 blocks: module docstring)
            assert set(g) == want
        assert se.tile_qualifies(A, rb)
        pads |= set(se.tile_padding(A, rb))
    # (the padding steps every 24 blocks: F's 74 blocks of 16 rows take all four, its 37 blocks of 32 rows the first two)
    assert pads == ({0, 1, 2, 3} if rb == 1 else {0, 1})
    levels, _ = se.levels_of(name)
    assert (int(levels[0]["m"]), int(levels[0]["n"]) - int(levels[0]["m"])) == (se.M_ONE, se.ND_ONE) == (73 * 16 + 1, 24 * 16 + 1)


@pytest.mark.parametrize("name", sorted(LADDERED))
def test_row_ladder_reaches_every_class(name):
    for l, w, A in _blocks(name):
        cnt = np.diff(A.indptr)
        assert not se.tile_qualifies(A, 1) and not se.tile_qualifies(A, 2), (l, w)
        if (l, w) not in LADDERED[name]:
            assert 2 <= cnt.min() and cnt.max() <= 4
            continue
        print(f"{name} level {l} {w}: {A.shape[0]} x {A.shape[1]}, {A.nnz} nonzeros, classes {sorted(set(cnt) - {2, 3, 4})}")
        assert set(se.ROW_NNZ) <= set(cnt) and cnt.max() == 200
        assert A.nnz < 8 * A.shape[0]
        if name.startswith("long"):
            assert A.shape[0] > se.PAIRS_AT + len(se.PAIRS) and A.shape[0] <= 2 * se.PAIRS_AT  # (two rows per wave, never three)
            got = [(int(cnt[i]), int(cnt[se.PAIRS_AT + i])) for i in range(len(se.PAIRS))]
            assert got == list(se.PAIRS) and len(set(se.PAIRS)) == 27
            assert set((a, b) for a in (0, 1, 64, 65, 129) for b in (0, 1, 64, 65, 129)) | {(200, 0), (0, 200)} == set(se.PAIRS)


@pytest.mark.parametrize("name", sorted(se.HIERS))
def test_no_coefficient_is_negligible(name):
    for l, w, A in _blocks(name):
        assert np.abs(A.data).min() >= se.MIN_COEF, (l, w)
        assert np.abs(A.real).sum(axis=1).max() <= 0.5 + 1e-12, (l, w)


@pytest.mark.parametrize("name", sorted(se.HIERS))
def test_oracle_against_restatement(name):
    h = se.hier(name)
    B = np.ascontiguousarray(h["B"][:, :NCOLS])
    Xr = se.restate(h["levels"], B, extended=name in ONE_LEVEL)
    err = se.colerr(h["Xo"][:, :NCOLS], Xr.astype(h["dtype"]))
    print(f"ORACLE-VS-RESTATEMENT {name}: {err:.2e}")
    assert err <= 1e-13
