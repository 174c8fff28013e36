"""GPU (-m gpu): the two software-pipelined matrix-core products of the levels >= 1 at every shape their loops
distinguish.

k_top_gemm (the combined top operators and the tail operator) walks the 64-k chunks of its K split three per loop trip,
the operand fragments two chunks ahead and the right-hand-side panel one chunk ahead, every load unconditional (clamped
chunk and row, zero selected for panel rows behind the operator's K extent).  The fixtures of the suite reach it only at
the chunk and split counts the planner happens to pick; here the tail of a small two-level hierarchy has nt rows, nt
chosen with launch_top_gemm's own formula so that a K split has 1, 2, 3, 4, 5 and 7 chunks (every remainder of the
three-way unroll, with and without a full trip), a shorter last split, and nt / the K extent no multiple of 64.

k_band_ct phase 2 (x = Tinv_c t, the explicit inverse of a component) walks the 32-k operand sets of ALL the strips a
wave owns as one sequence, the requests two sets ahead of the products across strip boundaries.  The ladder hierarchy
has every component size from 9 to 128 rows (every strip count, every set count 1 ... 4, every length of the sequence
modulo three), the blocks hierarchy has component bands below a top operator; BAND_WGS=1 chains several components onto
one workgroup (the requests past a component's last set must not disturb the next component), CT_WIDE / CT_WIDE4 = 0
select the 32- and 64-column instances of the kernel.

Checks per case: every column within 1e-12 of the oracle; the launch census shows the kernel family; the bits of a column
do not depend on the batch width; apply, an all-NaN batch, apply again gives the first bits (no stale panel row, no stale
register set); the operator products agree bit for bit with the handle that sums the K splits in the product kernel
itself (TOP_LAST=1)."""
import numpy as np
import pytest
import scipy.sparse as sp

from test_gpu_variants import TOL, _colerr, _handle, _hier
from util import dense_block, rand_rhs, rand_tri, synth_level

pytestmark = pytest.mark.gpu

_cache = {}


# ---- the operator products --------------------------------------------------------------------------------------------
def top_gemm_chunks(nt):
    """Chunks of 64 k per K split of the operator product over nt rows: engine.hip launch_top_gemm, k_top_gemm."""
    lda = (nt + 31) // 32 * 32
    tiles = (nt + 63) // 64
    nks = max(1, min(8, 256 // max(1, tiles)))
    kper = ((lda + nks - 1) // nks + 63) // 64 * 64
    nks = (lda + kper - 1) // kper
    return [(min(k * kper + kper, lda) - k * kper + 63) // 64 for k in range(nks)]


# nt -> chunks per split.  70: one chunk, two splits, the second 32 wide; 900: a short last split behind splits of two;
# 1,100: exactly one trip of the unrolled loop (the last split 160 wide: its third chunk is half empty); 1,700: a trip and
# one chunk, and a split of three; 2,100: a trip and two; 2,400: two trips and one.  No nt is a multiple of 64.
TAILS = {70: [1, 1], 900: [2] * 7 + [1], 1100: [3] * 6, 1700: [4] * 6 + [3], 2100: [5] * 6 + [3], 2400: [7] * 5 + [3]}


def test_tail_shapes_cover_every_chunk_count():
    for nt, chunks in TAILS.items():
        assert top_gemm_chunks(nt) == chunks, (nt, top_gemm_chunks(nt))
        assert nt % 64 != 0
    counts = {c for chunks in TAILS.values() for c in chunks}
    assert counts >= {1, 2, 3, 4, 5, 7}
    assert {c % 3 for c in counts} == {0, 1, 2}
    assert any(len(set(chunks)) > 1 for chunks in TAILS.values())  # (a shorter last split)


def _tail_levels(nt):
    """Two levels + dense block, the second level (the tail: one operator, nt rows) kept well conditioned: about three
    nonzeros per triangle row whatever its size."""
    rng = np.random.default_rng(600 + nt)
    rs = np.random.RandomState
    m0 = 300
    n0 = m0 + nt
    nd = 30 if nt < 100 else 120
    m1 = nt - nd
    lv0 = synth_level(m0, n0, rand_tri(m0, 0.02, True, rng), rand_tri(m0, 0.02, False, rng),
                      sp.random(nt, m0, density=0.01, random_state=rs(nt + 1), format="csr"),
                      sp.random(m0, nt, density=0.01, random_state=rs(nt + 2), format="csr"), rng)
    dt, de = min(0.2, 6.0 / m1), min(0.05, 25.0 / m1)
    lv1 = synth_level(m1, nt, rand_tri(m1, dt, True, rng), rand_tri(m1, dt, False, rng),
                      sp.random(nd, m1, density=de, random_state=rs(nt + 3), format="csr"),
                      sp.random(m1, nd, density=0.05, random_state=rs(nt + 4), format="csr"), rng)
    lv1["dense_n"], lv1["dense"] = nd, dense_block(nd, 4.0, rng)
    return [lv0, lv1]


def _tail(nt):
    """levels, the 64-column batch, the oracle's answer and the two handles: once per nt, never written to."""
    if nt not in _cache:
        from oracle import orc

        levels = _tail_levels(nt)
        B = rand_rhs(np.random.default_rng(61), (int(levels[0]["n"]), 64))
        h = dict(name=f"tail{nt}", levels=levels, dtype=np.float64, B=B, Xo=orc.Oracle(levels).solve_batch(B, threads=4))
        for a in (h["B"], h["Xo"]):
            a.setflags(write=False)
        h["M"], h["Mlast"] = _handle(h, {}), _handle(h, {"TOP_LAST": "1"})
        _cache[nt] = h
    return _cache[nt]


@pytest.mark.parametrize("width", (64, 16, 33))
@pytest.mark.parametrize("nt", sorted(TAILS))
def test_operator_product_shapes(nt, width):
    h = _tail(nt)
    M, Mlast = h["M"], h["Mlast"]
    se = M.stats_ext()
    assert se["tail_rows"] == nt, se  # (the tail IS one operator of nt rows: the formula above describes its launch)
    B = np.ascontiguousarray(h["B"][:, :width])
    X = M.solve_mrhs(B)
    census = M.kernel_census()
    err = _colerr(X, h["Xo"][:, :width])
    print(f"OPERAND top_gemm nt {nt} chunks {TAILS[nt]} width {width}: relerr {err:.2e}, top_gemm {census['top_gemm']}, "
          f"top_reduce {census['top_reduce']}")
    assert err <= TOL, err
    assert census["top_gemm"] > 0 and census["top_reduce"] > 0, census
    # the K splits summed by the last workgroup to arrive: the same products, the same order
    Xl = Mlast.solve_mrhs(B)
    cl = Mlast.kernel_census()
    assert cl["top_gemm"] > 0 and cl["top_reduce"] == 0, cl
    assert np.array_equal(Xl, X), _colerr(Xl, X)
    # the panel's zero rows and the idle panel buffer hold nothing a later solve can see
    for H in (M, Mlast):
        Xn = H.solve_mrhs(np.full_like(B, np.nan))
        assert np.isnan(Xn).all()
        X2 = H.solve_mrhs(B)
        assert np.array_equal(X2, X), (int(np.isnan(X2).sum()), _colerr(np.nan_to_num(X2), X))


# ---- the inverse product ------------------------------------------------------------------------------------------------
W1 = {"BAND_WGS": "1"}
INVERSE = [
    ("default", {}, ()),
    ("band_wgs=1", W1, ("band_ct1",)),
    ("band_wgs=1-ct_wide=0", dict(W1, CT_WIDE="0"), ("band_ct2",)),
    ("band_wgs=1-ct_wide4=0", dict(W1, CT_WIDE="0", CT_WIDE4="0"), ("band_ct4",)),
]


@pytest.mark.parametrize("hier", ("ladder", "blocks"))
@pytest.mark.parametrize("name,env,need", INVERSE, ids=[r[0] for r in INVERSE])
def test_inverse_product(name, env, need, hier):
    h = _hier(hier)
    M = _handle(h, env)
    if "BAND_WGS" in env:
        assert M.stats_ext()["cd_shared_workgroups"] > 0  # (workgroups that walk several components)
    for tr in (False, True):
        Xo = h["XoT"] if tr else h["Xo"]
        B64 = np.ascontiguousarray(h["B"][:, :64])
        X = M.solve_mrhs(B64, trans=tr)
        census = M.kernel_census()
        err = _colerr(X, Xo[:, :64])
        print(f"OPERAND inverse {name} on {hier}{' transposed' if tr else ''}: relerr {err:.2e}, "
              + " ".join(f"{k}={n}" for k, n in census.items() if k.startswith("band_c") and n))
        assert err <= TOL, err
        assert sum(n for f, n in census.items() if f.startswith("band_ct")) > 0, census
        for f in need:
            assert census[f] > 0, (f, census)
        for k in (16, 49):
            Xk = M.solve_mrhs(np.ascontiguousarray(h["B"][:, :k]), trans=tr)
            ck = M.kernel_census()
            assert sum(n for f, n in ck.items() if f.startswith("band_ct")) > 0, ck
            assert _colerr(Xk, Xo[:, :k]) <= TOL, (k, _colerr(Xk, Xo[:, :k]))
            assert np.array_equal(Xk, X[:, :k]), (tr, k, _colerr(Xk, X[:, :k]))
        M.solve_mrhs(np.full_like(B64, np.nan), trans=tr)
        X2 = M.solve_mrhs(B64, trans=tr)
        assert np.array_equal(X2, X), (tr, int(np.isnan(X2).sum()), _colerr(np.nan_to_num(X2), X))
    M.close()
