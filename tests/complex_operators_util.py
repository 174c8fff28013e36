"""Hierarchies of the complex-operator tests (test_complex_operators_host.py, test_gpu_complex_operators.py): the `blocks`
hierarchy of test_gpu_variants.py with the crown sizes as a parameter, and small two-level hierarchies whose tail has a
chosen number of rows."""
import numpy as np
import scipy.sparse as sp

from util import clustered_tri, dense_block, rand_tri, shared_coupling, synth_level, transposed_pattern

ZOP_TAIL, ZOP_TOP = 1, 2


def blocks_levels(dtype=np.complex128, crowns=(160, 120), seed=32):
    """test_gpu_variants.py `_blocks` (crowns (160, 120), seed 32: the very same arrays, draw for draw): three levels +
    dense block, 6,000 rows; levels 0 and 1 are 24-row clusters under a crown of `crowns` rows that no component holds --
    what the planner closes into the level's top operator."""
    rng = np.random.default_rng(seed)
    n0, m0, m1, m2 = 6000, 3400, 2200, 250
    n1 = n0 - m0
    n2 = n1 - m1
    nd = n2 - m2
    L0, L1 = clustered_tri(m0, 24, 6, crowns[0], rng), clustered_tri(m1, 24, 6, crowns[1], rng)
    lv0 = synth_level(m0, n0, L0, transposed_pattern(L0, rng), shared_coupling(n1, m0, rng),
                      shared_coupling(m0, n1, rng), rng, dtype=dtype)
    lv1 = synth_level(m1, n1, L1, transposed_pattern(L1, rng), shared_coupling(n2, m1, rng),
                      shared_coupling(m1, n2, rng), rng, dtype=dtype)
    lv2 = synth_level(m2, n2, rand_tri(m2, 0.04, True, rng, dtype=dtype), rand_tri(m2, 0.04, False, rng, dtype=dtype),
                      sp.random(nd, m2, density=0.05, random_state=np.random.RandomState(5), format="csr"),
                      sp.random(m2, nd, density=0.05, random_state=np.random.RandomState(6), format="csr"), rng, dtype=dtype)
    lv2["dense_n"], lv2["dense"] = nd, dense_block(nd, 6.0, rng, dtype, scale=0.2)
    return [lv0, lv1, lv2]


def edge_levels(ntail, m0=300, dtype=np.complex128, seed=61):
    """Two sparse levels + dense block: level 0 has m0 leading rows, level 1 -- the tail, with its dense block -- `ntail`
    rows, half of them leading.  Well conditioned by construction: small off-diagonal entries, pivots in [0.5, 2], a
    dense block shifted by 6."""
    rng = np.random.default_rng(seed + 7 * ntail + m0)
    n0 = m0 + ntail
    m1 = max(1, ntail // 2)
    nd = ntail - m1
    rs = np.random.RandomState

    def coupling(r, c, k):
        return sp.random(r, c, density=min(1.0, 6.0 / max(1, c)), random_state=rs(seed + k), format="csr") * 0.3

    lv0 = synth_level(m0, n0, rand_tri(m0, 0.02, True, rng, dtype=dtype), rand_tri(m0, 0.02, False, rng, dtype=dtype),
                      coupling(ntail, m0, 1), coupling(m0, ntail, 2), rng, dtype=dtype)
    lv1 = synth_level(m1, ntail, rand_tri(m1, min(1.0, 4.0 / m1), True, rng, dtype=dtype),
                      rand_tri(m1, min(1.0, 4.0 / m1), False, rng, dtype=dtype), coupling(nd, m1, 3), coupling(m1, nd, 4), rng,
                      dtype=dtype)
    lv1["dense_n"], lv1["dense"] = nd, dense_block(nd, 6.0, rng, dtype, scale=0.2)
    return [lv0, lv1]


def import_levels(levels, dtype=np.complex128, complex_operators=0):
    """add_level / set_dense as HIF.from_levels does, without finalize (no GPU needed)."""
    import hifir_amd

    M = hifir_amd.HIF(dtype, complex_operators=complex_operators)
    for lv in levels:
        M.add_level(lv)
    last = levels[-1]
    if int(last.get("dense_n", 0)) > 0:
        M.set_dense(last["dense"])
    return M
