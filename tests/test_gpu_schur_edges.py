"""GPU (-m gpu): the Schur coupling products out = s[p] b[p] - A x (A = E: S3, A = F: S5) at their group, pipeline and row
edges, against the oracle.

The kernels (kernels.hip.hpp): k_spmm_tile<RB, NCT>, k_spmm_tile4<RB, NCT>, k_spmm_tile_z, k_spmm_epi (at 64 columns:
spmm_stream_r64), k_spmm_epi_narrow, k_spmm_prod, and the grouping behind the tiled ones, host.hpp build_spmm_tiles.  The
other small-size files feed them one shape each: util.shared_coupling gives every 16-row block exactly four groups (one
trip of the 8-group loop, one group per wave of k_spmm_tile4, no clamp, no padding, no empty block), sp.random gives rows of
about 18 nonzeros (one item of the stream), and no coupling block has more than 16,384 rows (no wave of k_spmm_epi takes a
second row).  Here the inputs are the ladders of schur_edges_util.py; test_schur_edges_host.py asserts on the CPU that they
reach the classes, and pins the oracle to an independent restatement to 1e-13.

Every row of the table creates its handle as test_gpu_variants.py does (BASE + the row's switches, TAIL_ROWS=0 so that no
tail operator replaces the level) and passes the same four checks on the batch rand_rhs(default_rng(41), (n, 100)):

 1. width 100, forwards and conjugate-transposed, every column within 1e-12 of the oracle; on the one-level hierarchies
    M.mmultiply likewise against the oracle's product (k_spmm_prod);
 2. widths 1, 15, 16, 17, 32, 33, 48, 49 reproduce the bits of the 64-column solve (NCT = 1 ... 4 of the tiled kernels,
    k_spmm_epi_narrow at 16 and 32 lanes against the stream);
 3. apply, apply an all-NaN batch, apply again: the third result has the bits of the first;
 4. the launch census: required families > 0, forbidden == 0, and where the row says so the EXACT number of k_spmm_epi
    launches: one per coupling block that has no tiles, two blocks per level (launch_spmm is called once for S3 and,
    with FUSE_F=0, once for S5 in engine.hip enqueue_level).

The conjugate-transposed apply runs the same kernels on F^H and E^H (import.hpp adjoint_level), which are not ladders: what
they must launch is derived from schur_edges_util.tile_qualifies, the engine's three conditions restated -- so the census
also checks that restatement in both directions.

`same` rows: the bits of another row's handle at 64 columns, forwards and transposed (with check 2 that is every width).
Default-environment rows (whatever the planner then chooses, the tail operator included) check accuracy only.

Not reached here: the grid-stride loops of k_spmm_tile / k_spmm_tile_z (more than 16,384 blocks) and of
k_spmm_epi_narrow, a wave's third row, the F product fused into the band kernels (test_gpu_variants.py), any timing."""
import numpy as np
import pytest

import schur_edges_util as se
import test_gpu_variants as tv

pytestmark = pytest.mark.gpu

TOL = 1e-12  # (test_gpu_parity.py, test_gpu_variants.py)
WIDTHS = (1, 15, 16, 17, 32, 33, 48, 49)
T0 = {"TAIL_ROWS": "0"}
TILE_ANY = tv.TILE_ANY + ("spmm_tile_z",)
ONE_LEVEL = ("tiles", "tiles2", "tilesz", "rows", "rowsz")


class Row:
    """env: switches on top of BASE and TAIL_ROWS=0 (default=True: BASE alone, accuracy only); need / deny: census families
    at width 64; need16 / need32 / deny16: at widths 16 / 32 / 16; exact: assert the exact number of spmm_epi launches at
    width 64; census=False: checks 1-3 only; same: the name of the row whose bits this one has; rb: the block height the
    handle's tiles are built with; tiles: the handle builds tiles at all."""

    def __init__(self, name, hier, env, need=(), deny=(), need16=(), need32=(), deny16=(), exact=False, census=True, same=None,
                 rb=1, tiles=True, default=False):
        self.name, self.hier, self.env = name, hier, dict(env if default else dict(T0, **env))
        self.need, self.deny, self.need16, self.need32, self.deny16 = need, deny, need16, need32, deny16
        self.exact, self.census, self.same, self.rb, self.tiles, self.default = exact, census, same, rb, tiles, default


F0 = {"FUSE_F": "0"}
ROWS = [
    Row("tiles", "tiles", {}, need=("spmm_tile4_rb1",), deny=("spmm_epi", "spmm_tile_rb1", "spmm_tile_rb2")),
    Row("tiles-split=0", "tiles", {"SPMM_SPLIT": "0"}, need=("spmm_tile_rb1",), deny=("spmm_tile4_rb1", "spmm_tile4_rb2")),
    Row("tiles2-rb2", "tiles2", {"SPMM_RB": "2"}, need=("spmm_tile4_rb2",), deny=("spmm_tile_rb1", "spmm_tile4_rb1"), rb=2),
    Row("tiles2-rb2-split=0", "tiles2", {"SPMM_RB": "2", "SPMM_SPLIT": "0"}, need=("spmm_tile_rb2",),
        deny=("spmm_tile4_rb1", "spmm_tile4_rb2"), rb=2),
    Row("tiles-narrow_tiles=0", "tiles", {"NARROW_TILES": "0"}, need=("spmm_tile4_rb1",), need16=("spmm_tile4_rb1",), same="tiles"),
    Row("tilesz", "tilesz", {}, need=("spmm_tile_z",), deny=("spmm_epi",)),
    Row("tiles-spmm_tiles=0", "tiles", {"SPMM_TILES": "0"}, need=("spmm_epi",), need16=("spmm_epi_narrow",), deny=TILE_ANY, tiles=False),
    Row("tilesz-spmm_tiles_z=0", "tilesz", {"SPMM_TILES_Z": "0"}, need=("spmm_epi",), need16=("spmm_epi_narrow",), deny=TILE_ANY,
        tiles=False),
    Row("rows-fuse_f=0", "rows", F0, need=("spmm_epi",), need16=("spmm_epi_narrow",), need32=("spmm_epi_narrow",), deny=TILE_ANY,
        exact=True),
    Row("rowsz-fuse_f=0", "rowsz", F0, need=("spmm_epi",), need16=("spmm_epi_narrow",), need32=("spmm_epi_narrow",), deny=TILE_ANY,
        exact=True),
    Row("rows-fuse_f=0-narrow_spmm=0", "rows", dict(F0, NARROW_SPMM="0"), need=("spmm_epi",), need16=("spmm_epi",),
        deny=("spmm_epi_narrow",), deny16=("spmm_epi_narrow",), exact=True, same="rows-fuse_f=0"),
    Row("long_rows-fuse_f=0", "long_rows", F0, need=("spmm_epi",), deny=TILE_ANY, exact=True),
    Row("long_rowsz-fuse_f=0", "long_rowsz", F0, need=("spmm_epi",), deny=TILE_ANY, exact=True),
    # whichever kernel takes F (the second L solve where the plan allows): checks 1-3
    Row("rows-fuse_f", "rows", {}, census=False),
    Row("long_rows-fuse_f", "long_rows", {}, census=False),
] + [Row(f"default-{h}", h, {}, default=True, census=False) for h in sorted(se.HIERS)]
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)

_cache = {}


def _handle(h, env):
    import hifir_amd

    with tv._Env(env):
        return hifir_amd.HIF.from_levels(h["levels"], max_nrhs=64, dtype=h["dtype"])


def _epi_launches(row, h, trans):
    """(coupling products that launch_spmm runs, those of them on tiles) in one apply: two blocks per level."""
    total = tiled = 0
    for lv in h["levels"]:
        for A in (se.adjoint_couplings(lv) if trans else (se.coupling(lv, "E"), se.coupling(lv, "F"))):
            total += 1
            tiled += bool(row.tiles and se.tile_qualifies(A, 1 if h["dtype"] == np.complex128 else row.rb))
    return total, tiled


def measure(row):
    """Everything the checks look at, as plain data: once per row (a `same` row reads its partner's)."""
    if row.name in _cache:
        return _cache[row.name]
    h = se.hier(row.hier, products=row.hier in ONE_LEVEL and not row.default)
    M = _handle(h, row.env)
    B = h["B"]
    r = dict(width_bits=[], replay_bits=[], census={})
    r["err"] = se.colerr(M.solve_mrhs(B), h["Xo"])
    r["errT"] = se.colerr(M.solve_mrhs(B, trans=True), h["XoT"])
    if "Yo" in h and not row.default:
        r["perr"] = se.colerr(M.mmultiply(B, rank=-1), h["Yo"])
        r["prod"] = M.kernel_census()["prod"]
        r["perrT"] = se.colerr(M.mmultiply(B, trans=True, rank=-1), h["YoT"])
        r["prodT"] = M.kernel_census()["prod"]
    if row.hier.startswith("long"):
        r["rows_E0"] = M.level_stats(0)["n"] - M.level_stats(0)["m"]
        r["rows_F1"] = M.level_stats(1)["m"]
    B64 = np.ascontiguousarray(B[:, :64])
    for tr in (False, True):
        if row.default:
            break
        X = M.solve_mrhs(B64, trans=tr)
        r["X64", tr] = X
        r["census"][64, tr] = M.kernel_census()
        for k in WIDTHS:
            Xk = M.solve_mrhs(np.ascontiguousarray(B[:, :k]), trans=tr)
            if k in (16, 32):
                r["census"][k, tr] = M.kernel_census()
            if not np.array_equal(Xk, X[:, :k]):
                r["width_bits"].append((tr, k, se.colerr(Xk, X[:, :k])))
        M.solve_mrhs(np.full_like(B64, np.nan), trans=tr)
        X3 = M.solve_mrhs(B64, trans=tr)
        if not np.array_equal(X3, X):
            r["replay_bits"].append((tr, int(np.isnan(X3).sum()), se.colerr(np.nan_to_num(X3), X)))
    M.close()
    _cache[row.name] = r
    return r


def _fmt(c):
    return " ".join(f"{k}={n}" for k, n in c.items() if n)


@pytest.mark.parametrize("row", [pytest.param(r, id=r.name) for r in ROWS])
def test_schur_edges(row):
    r = measure(row)
    h = se.hier(row.hier)
    print(f"SCHUR-EDGES {row.name}: relerr {r['err']:.2e} transposed {r['errT']:.2e}"
          + (f" product {r['perr']:.2e} transposed {r['perrT']:.2e}" if "perr" in r else "") + f" (bar {TOL:.0e})")
    for key, c in r["census"].items():
        print(f"  census width {key[0]}{' transposed' if key[1] else ''}: {_fmt(c)}")
    # 1. accuracy
    assert r["err"] <= TOL and r["errT"] <= TOL, (r["err"], r["errT"])
    if "perr" in r:
        assert r["perr"] <= TOL and r["perrT"] <= TOL, (r["perr"], r["perrT"])
        assert r["prod"] > 0 and r["prodT"] > 0, "the product ran none of its own kernels (k_spmm_prod among them)"
    if row.hier.startswith("long"):  # (the condition under which a wave of k_spmm_epi takes a second row)
        assert r["rows_E0"] > 16384 and r["rows_F1"] > 16384, (r["rows_E0"], r["rows_F1"])
    if row.default:
        return
    # 2. width independence, 3. replay
    assert not r["width_bits"], r["width_bits"]
    assert not r["replay_bits"], r["replay_bits"]
    # 4. census
    for tr in (False, True) if row.census else ():
        total, tiled = _epi_launches(row, h, tr)
        if not tr:  # (the ladders themselves: every block is what the row is about)
            assert tiled == (total if row.tiles and row.hier.startswith("tiles") else 0), (total, tiled)
        runs = {f: (tiled > 0 if f in TILE_ANY else total - tiled > 0) for f in TILE_ANY + ("spmm_epi", "spmm_epi_narrow")}
        print(f"  {'transposed' if tr else 'forward'}: {total} coupling products, {tiled} on tiles")
        c64, c16, c32 = r["census"][64, tr], r["census"][16, tr], r["census"][32, tr]
        for f in row.need:
            assert not runs[f] or c64[f] > 0, (tr, 64, f, "never launched")
        for f in row.deny:
            assert (f == "spmm_epi" and total > tiled) or c64[f] == 0, (tr, 64, f, c64[f])
        for f in row.need16:
            assert not runs[f] or c16[f] > 0, (tr, 16, f, "never launched")
        for f in row.need32:
            assert not runs[f] or c32[f] > 0, (tr, 32, f, "never launched")
        for f in row.deny16:
            assert c16[f] == 0 and c32[f] == 0, (tr, f, c16[f], c32[f])
        if row.exact:
            assert c64["spmm_epi"] == total - tiled, (tr, c64["spmm_epi"], total, tiled)
            assert total == 2 * len(h["levels"])
    # the bits of the row without the switch
    if row.same:
        ref = measure(BY_NAME[row.same])
        for tr in (False, True):
            assert np.array_equal(r["X64", tr], ref["X64", tr]), (tr, se.colerr(r["X64", tr], ref["X64", tr]))
