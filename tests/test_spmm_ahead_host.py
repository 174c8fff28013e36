"""CPU: the group ladder of test_gpu_spmm_ahead.py (spmm_ahead_util.py) brings every group count that the batched loops of
k_spmm_tile / k_spmm_tile4 distinguish, counted with schur_edges_util.tile_groups (host.hpp build_spmm_tiles restated).

For every constant c of the loops (each kernel's batch BU and its 2 BU: the loop's trip, and how far the source ids run
ahead):
 * per-wave kernel: blocks of c - 1, c and c + 1 groups;
 * k_spmm_tile4: blocks whose four waves hold c - 1, c and c + 1 groups each, and blocks in which wave 0 holds one group
   more than the others, c against c - 1 and c + 1 against c;
and the empty block, blocks of 1 ... 3 groups (waves without any), a one-row last block, every padding of a last group.
These are conditions on the INPUT: a change of the ladder, or of a batch size, that moves a count away fails here."""
import pytest

import schur_edges_util as se
import spmm_ahead_util as sa


def _constants(bu):
    return sorted({bu, 2 * bu})


@pytest.mark.parametrize("name,rb", [("ahead", 1), ("ahead2", 2)])
def test_ladder_reaches_every_count(name, rb):
    levels = sa.ahead_levels(rb)
    assert (int(levels[0]["m"]), int(levels[0]["n"]) - int(levels[0]["m"])) == (se.M_ONE, se.ND_ONE)
    pads = set()
    for w in "EF":
        A = se.coupling(levels[0], w)
        g = se.tile_groups(A, rb)
        print(f"{name} {w}: {A.shape[0]} x {A.shape[1]}, {A.nnz} nonzeros, {len(g)} blocks of {16 * rb} rows, groups {sorted(set(g))}, "
              f"paddings {sorted(set(se.tile_padding(A, rb)))}")
        assert g == [sa.AHEAD_LADDER[b % 24] for b in range(len(g))]  # (the generator's promise, block by block)
        assert se.tile_qualifies(A, rb)
        assert abs(A.data).min() >= se.MIN_COEF and abs(A).sum(axis=1).max() <= 0.5 + 1e-12
        pads |= set(se.tile_padding(A, rb))
        if w == "E" and rb == 2:  # (13 blocks of 32 rows: the first 13 entries; F walks all of them)
            continue
        have = set(g)
        assert {0, 1, 2, 3} <= have
        # k_spmm_tile: a wave walks the whole block
        for c in _constants(sa.BU_TILE[rb]):
            assert {c - 1, c, c + 1} <= have, (w, c)
        # k_spmm_tile4: wave w of the block walks groups w, w + 4, ...
        per_wave = {sa.wave_groups(G) for G in have}
        for c in _constants(sa.BU_TILE4[rb]):
            for want in ((c - 1,) * 4, (c,) * 4, (c + 1,) * 4, (c, c - 1, c - 1, c - 1), (c + 1, c, c, c)):
                assert want in per_wave, (w, c, want)
        assert 68 in have  # (17 groups per wave of k_spmm_tile4: several trips and a remainder)
    assert pads == ({0, 1, 2, 3} if rb == 1 else {0, 1})
    # the last block of E holds one row (rb = 2: its second row tile lies beyond the rows), that of F one row in its last tile
    assert se.ND_ONE % 16 == 1 and se.M_ONE % 32 == 17


def test_ladder_covers_every_candidate_constant():
    """The ladder does not depend on which batch sizes the kernels ended up with: it straddles 2, 3, 4, 6 and 8."""
    have = set(sa.AHEAD_LADDER)
    per_wave = {sa.wave_groups(G) for G in have}
    for rb in (1, 2):
        assert set(_constants(sa.BU_TILE[rb])) | set(_constants(sa.BU_TILE4[rb])) <= set(sa.CONSTANTS)
    for c in sa.CONSTANTS:
        assert {c - 1, c, c + 1} <= have
        for want in ((c - 1,) * 4, (c,) * 4, (c + 1,) * 4, (c, c - 1, c - 1, c - 1), (c + 1, c, c, c)):
            assert want in per_wave, (c, want)
