"""GPU (-m gpu): phase 1 of k_band_ct (acc = coefficient tiles x gathered source rows, per 16-row strip) at every strip
length its loop distinguishes, with the requests running ahead (the default) and without (HIFIR_AMD_CD_DBG=2048: the one
bit of the development switch that switches nothing off -- the loop of before, as a second template instance).

The loop multiplies a strip's tiles in batches of BU = 8 / 4 / 2 (one / two / four column tiles per workgroup), two
batches per trip; source ids are requested two batches ahead, gathers and coefficient tiles one batch ahead, every load
unconditional and clamped to the strip's last tile.  The fixture (ct_ahead_util.py; test_ct_ahead_host.py checks what the
planner makes of it) has strips of 0, 1, BU - 1, BU, BU + 1, 2 BU - 1, 2 BU, 2 BU + 1 and 3 BU + 2 tiles for each BU,
partly empty last tiles, single-strip components of 16 and 9 rows, an empty strip between two others, and 128-row
components of eight different strips; BAND_WGS=1 chains up to 17 components on one workgroup (a request past a
component's last tile must not disturb the next), CT_WIDE / CT_WIDE4 select the 16-, 32- and 64-column instances.

Checks per case: every column within 1e-12 of the oracle; the launch census shows the instance; the bits equal those of
the handle created under HIFIR_AMD_CD_DBG=2048 (the same sums in the same order); the bits of a column do not depend on
the batch width; apply, an all-NaN batch, apply again gives the first bits (no stale register set).  The ladder of
util.py (every component size 9 ... 128) is solved under both settings of the switch as well, bit for bit."""
import numpy as np
import pytest

from ct_ahead_util import ct_ahead_levels
from test_gpu_variants import TOL, _colerr, _handle, _hier
from util import rand_rhs

pytestmark = pytest.mark.gpu

_cache = {}
W1 = {"BAND_WGS": "1", "TOP_ROWS": "0"}  # (a band of eight workgroups would otherwise be taken into the level's top operator)
WIDE2, WIDE4 = {"CT_WIDE": "0"}, {"CT_WIDE": "0", "CT_WIDE4": "0"}
NARROW = {"CT_WIDE": "1000000"}
PLAIN = {"CD_DBG": "2048"}  # gathers in front of their own products
CASES = [
    ("default", {}, ("band_ct1",)),                 # 105 workgroups: one 16-column slice per workgroup
    ("ct_wide=0", WIDE2, ("band_ct2",)),
    ("ct_wide4=0", WIDE4, ("band_ct4",)),
    ("ct_wide=off", NARROW, ("band_ct1",)),         # (CT_WIDE4's opposite: no band takes more than one column tile)
    ("band_wgs=1", W1, ("band_ct1",)),
    ("band_wgs=1-ct_wide=0", dict(W1, **WIDE2), ("band_ct2",)),
    ("band_wgs=1-ct_wide4=0", dict(W1, **WIDE4), ("band_ct4",)),
]
WIDTHS = (64, 16, 33)


def _fixture():
    """levels, the 64-column batch and the oracle's two answers: once, never written to."""
    if "h" not in _cache:
        from oracle import orc

        levels, _ = ct_ahead_levels()
        B = rand_rhs(np.random.default_rng(72), (int(levels[0]["n"]), 64))
        O = orc.Oracle(levels)
        h = dict(name="ct_ahead", levels=levels, dtype=np.float64, B=B, Xo=O.solve_batch(B, threads=4),
                 XoT=O.solve_batch(B, trans=True, threads=4))
        for a in (h["B"], h["Xo"], h["XoT"]):
            a.setflags(write=False)
        _cache["h"] = h
    return _cache["h"]


def _ct(census):
    return {f: n for f, n in census.items() if f.startswith("band_ct") and n}


@pytest.mark.parametrize("name,env,need", CASES, ids=[c[0] for c in CASES])
def test_strip_lengths(name, env, need):
    h = _fixture()
    M, M0 = _handle(h, env), _handle(h, dict(env, **PLAIN))
    if "BAND_WGS" in env:
        assert M.stats_ext()["cd_shared_workgroups"] > 0  # (workgroups that walk several components)
    for tr in (False, True):
        Xo = h["XoT"] if tr else h["Xo"]
        bits = {}
        for width in WIDTHS:
            B = np.ascontiguousarray(h["B"][:, :width])
            X = M.solve_mrhs(B, trans=tr)
            census = M.kernel_census()
            err = _colerr(X, Xo[:, :width])
            print(f"CT_AHEAD {name}{' transposed' if tr else ''} width {width}: relerr {err:.2e}, {_ct(census)}")
            assert err <= TOL, err
            if width == 64:  # (a narrower batch has fewer column tiles: it may take a narrower instance)
                for f in need:
                    assert census[f] > 0, (f, census)
            assert _ct(census), census
            # the loop of the parent commit: the same products in the same order
            X0 = M0.solve_mrhs(B, trans=tr)
            assert _ct(M0.kernel_census()) == _ct(census)
            assert np.array_equal(X0, X), (width, _colerr(X0, X))
            # no stale register set, no stale LDS row
            Xn = M.solve_mrhs(np.full_like(B, np.nan), trans=tr)
            assert np.isnan(Xn).all()
            X2 = M.solve_mrhs(B, trans=tr)
            assert np.array_equal(X2, X), (width, int(np.isnan(X2).sum()), _colerr(np.nan_to_num(X2), X))
            bits[width] = X
        for width in WIDTHS[1:]:  # a column's bits do not depend on the batch it travels in
            assert np.array_equal(bits[width], bits[64][:, :width]), (tr, width, _colerr(bits[width], bits[64][:, :width]))
    M.close()
    M0.close()


@pytest.mark.parametrize("name,env", [(c[0], c[1]) for c in CASES[:3]], ids=[c[0] for c in CASES[:3]])
def test_ladder_same_bits(name, env):
    """Every component size 9 ... 128 (util.ladder_levels), both settings of the switch."""
    h = _hier("ladder")
    M, M0 = _handle(h, env), _handle(h, dict(env, **PLAIN))
    for tr in (False, True):
        Xo = h["XoT"] if tr else h["Xo"]
        B = np.ascontiguousarray(h["B"][:, :64])
        X = M.solve_mrhs(B, trans=tr)
        census = M.kernel_census()
        err = _colerr(X, Xo[:, :64])
        print(f"CT_AHEAD ladder {name}{' transposed' if tr else ''}: relerr {err:.2e}, {_ct(census)}")
        assert err <= TOL, err
        assert _ct(census), census
        X0 = M0.solve_mrhs(B, trans=tr)
        assert _ct(M0.kernel_census()) == _ct(census)
        assert np.array_equal(X0, X), _colerr(X0, X)
    M.close()
    M0.close()
