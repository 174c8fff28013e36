"""GPU (-m gpu): the tiled Schur products out = s[p] b[p] - A x (k_spmm_tile, k_spmm_tile4; A = E: S3, A = F: S5) with
their requests running ahead (the default) and without (HIFIR_AMD_CD_DBG=4096: one more bit of the development switch
that switches nothing off -- the former group loop and epilogue, as a second template instance).

The loop multiplies a wave's column groups in batches of BU, two batches per trip; source ids are requested two batches
ahead, gathers and coefficient tiles one batch ahead, every load unconditional and clamped to the wave's last group; the
remainder is multiplied behind the loop.  The epilogue's operands -- the rows' places p in the level's input, their
scales s and the right-hand sides -- are requested before the last products, rows clamped to the last row and columns to
the batch's last column, zero selected for the columns beyond the batch; only the stores depend on the row.

Fixtures (one level + dense block of 1,554 rows unless said otherwise; E is 385 x 1,169, F 1,169 x 385):
 * schur_edges_util tiles / tiles2: the ladder built around the former loop's constants -- the empty block, blocks of 1-3
   groups, a one-row last block, under 32-row blocks a second row tile beyond the rows;
 * spmm_ahead_util ahead / ahead2: the ladder that straddles the batch sizes of this loop (test_spmm_ahead_host.py asserts
   on the CPU that every count arrives);
 * util.ladder_levels (8,520 rows): E from util.shared_coupling, exactly four groups per block;
 * test_gpu_variants "blocks" (three levels, 6,000 rows, shared couplings on levels 0 and 1): on the child level the
   products read their right-hand sides from the arena (ldb = 64, roff = m).
Each is solved per wave (SPMM_SPLIT=0) and per workgroup, the 32-row fixtures with SPMM_RB=2 as well.

Checks per case, forwards and conjugate-transposed: every column within 1e-12 of the oracle; the census shows the
family; the bits equal those of a handle created under CD_DBG=4096, whose census is the same; the bits of the 64-column
solve hold at widths 1, 15, 16, 17, 32, 33, 48 and 49 (fewer column tiles per block, the column clamp of the early
right-hand-side loads); apply, an all-NaN batch, apply again gives the first bits (no stale register set)."""
import numpy as np
import pytest

import schur_edges_util as se
import spmm_ahead_util as sa
import test_gpu_variants as tv

pytestmark = pytest.mark.gpu

TOL = 1e-12  # (test_gpu_schur_edges.py, test_gpu_variants.py)
WIDTHS = (1, 15, 16, 17, 32, 33, 48, 49)
T0 = {"TAIL_ROWS": "0"}  # (no tail operator in the level's place)
PLAIN = {"CD_DBG": "4096"}
SPLIT0, RB2 = {"SPMM_SPLIT": "0"}, {"SPMM_RB": "2"}
CASES = [
    # name, hierarchy, switches, families the 64-column solve must launch, families it must not
    ("tiles", "tiles", {}, ("spmm_tile4_rb1",), ("spmm_tile_rb1", "spmm_tile_rb2", "spmm_tile4_rb2")),
    ("tiles2", "tiles2", {}, ("spmm_tile4_rb1",), ("spmm_tile_rb1", "spmm_tile_rb2", "spmm_tile4_rb2")),
    ("tiles-split=0", "tiles", SPLIT0, ("spmm_tile_rb1",), ("spmm_tile4_rb1", "spmm_tile4_rb2", "spmm_tile_rb2")),
    ("tiles2-split=0", "tiles2", SPLIT0, ("spmm_tile_rb1",), ("spmm_tile4_rb1", "spmm_tile4_rb2", "spmm_tile_rb2")),
    ("tiles2-rb2", "tiles2", RB2, ("spmm_tile4_rb2",), ("spmm_tile_rb1", "spmm_tile4_rb1", "spmm_tile_rb2")),
    ("tiles2-rb2-split=0", "tiles2", dict(RB2, **SPLIT0), ("spmm_tile_rb2",), ("spmm_tile_rb1", "spmm_tile4_rb1", "spmm_tile4_rb2")),
    ("ahead", "ahead", {}, ("spmm_tile4_rb1",), ("spmm_tile_rb1", "spmm_tile_rb2", "spmm_tile4_rb2")),
    ("ahead-split=0", "ahead", SPLIT0, ("spmm_tile_rb1",), ("spmm_tile4_rb1", "spmm_tile4_rb2", "spmm_tile_rb2")),
    ("ahead2-rb2", "ahead2", RB2, ("spmm_tile4_rb2",), ("spmm_tile_rb1", "spmm_tile4_rb1", "spmm_tile_rb2")),
    ("ahead2-rb2-split=0", "ahead2", dict(RB2, **SPLIT0), ("spmm_tile_rb2",), ("spmm_tile_rb1", "spmm_tile4_rb1", "spmm_tile4_rb2")),
    ("ladder", "ladder", {}, ("spmm_tile4_rb1",), ()),
    ("ladder-split=0", "ladder", SPLIT0, ("spmm_tile_rb1",), ("spmm_tile4_rb1", "spmm_tile4_rb2")),
    ("blocks", "blocks", {}, ("spmm_tile4_rb1",), ()),
    ("blocks-split=0", "blocks", SPLIT0, ("spmm_tile_rb1",), ("spmm_tile4_rb1", "spmm_tile4_rb2")),
]


def _hier(name):
    return tv._hier(name) if name in ("ladder", "blocks") else sa.hier(name)


def _tiles(census):
    return {f: n for f, n in census.items() if f.startswith("spmm_") and n}


@pytest.mark.parametrize("name,hname,env,need,deny", CASES, ids=[c[0] for c in CASES])
def test_spmm_ahead(name, hname, env, need, deny):
    h = _hier(hname)
    env = dict(T0, **env)
    M, M0 = tv._handle(h, env), tv._handle(h, dict(env, **PLAIN))
    for tr in (False, True):
        Xo = h["XoT"] if tr else h["Xo"]
        B = np.ascontiguousarray(h["B"][:, :64])
        X = M.solve_mrhs(B, trans=tr)
        census = M.kernel_census()
        err = se.colerr(X, Xo[:, :64])
        print(f"SPMM_AHEAD {name}{' transposed' if tr else ''}: relerr {err:.2e} (bar {TOL:.0e}), {_tiles(census)}")
        assert err <= TOL, err
        if not tr:  # (the transposed apply runs F^H and E^H, which are no ladders: whatever qualifies there)
            for f in need:
                assert census[f] > 0, (f, census)
            for f in deny:
                assert census[f] == 0, (f, census)
        else:  # (schur_edges_util.tile_qualifies: the engine's three conditions restated)
            rb = int(env.get("SPMM_RB", "1"))
            if any(se.tile_qualifies(A, rb) for lv in h["levels"] for A in se.adjoint_couplings(lv)):
                assert any(census[f] for f in tv.TILE_ANY), census
        # the loop and the epilogue of the parent commit: the same products in the same order
        X0 = M0.solve_mrhs(B, trans=tr)
        assert _tiles(M0.kernel_census()) == _tiles(census)
        assert np.array_equal(X0, X), se.colerr(X0, X)
        # a column's bits do not depend on the batch it travels in
        for width in WIDTHS:
            Xk = M.solve_mrhs(np.ascontiguousarray(h["B"][:, :width]), trans=tr)
            assert np.array_equal(Xk, X[:, :width]), (tr, width, se.colerr(Xk, X[:, :width]))
            X0k = M0.solve_mrhs(np.ascontiguousarray(h["B"][:, :width]), trans=tr)
            assert np.array_equal(X0k, Xk), (tr, width, se.colerr(X0k, Xk))
        # no stale register set
        Xn = M.solve_mrhs(np.full_like(B, np.nan), trans=tr)
        assert np.isnan(Xn).all()
        X2 = M.solve_mrhs(B, trans=tr)
        assert np.array_equal(X2, X), (int(np.isnan(X2).sum()), se.colerr(np.nan_to_num(X2), X))
    M.close()
    M0.close()
