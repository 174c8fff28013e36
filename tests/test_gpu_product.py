"""GPU (-m gpu): the multilevel products y = M x and y = M^H x (HIFAMD_M / HIFAMD_MH, engine.hip enqueue_prod_level) under
every kernel variant, against the oracle.

The product shares the engine's band, top-operator and dense-block kernels with the solve: the Schur coupling term of
every level is launch_ldu(st, L, logR, count) -- the PLAIN entry of those kernels (no FirstL, no LastU, no F product taken
along, no row skipping) on a plan built with all those fusions on.  A default solve enters most band kernels only with
one of the fusions, so the product is the only default-configuration user of that mode.  Around it the product has five
kernels of its own (k_gather_div, k_prod_rows, k_spmm_prod, k_vec_op, k_scatter_div: the census family `prod`), each of
which pads or masks the lanes beyond nrhs in its own way.

This file is test_gpu_variants.py's table once more for the two products: the same machinery (tv.HIERS, tv._handle,
tv._Env, tv._colerr, tv.V), the same band / top / dense-block expectations row by row (the plan is the same, so the same
families must appear in a product's census), and per (row, hierarchy), each for M and M^H:

 1. width 72 (one full tile and one of 8 columns, two lanes): every column within PROD_TOL of the oracle's column
    (Oracle.mmultiply, rank = -1 on both sides);
 2. a column's bits do not depend on the batch width: widths 1, 16, 17, 32, 33, 48, 49 against the 64-column product, and
    columns 40:48 on their own;
 3. product, product of an all-NaN batch of the same shape, product again: the third result has the bits of the first;
 4. solves and products interleaved on one handle (they share the w / v arena, the graph cache, the census and the twin
    engine): solve, product, transposed solve, transposed product, solve -- the two solves have identical bits, the
    products the bits of check 2's 64-column results; this runs after the width sweep, which captures more graphs than the
    cache holds, and a last 64-column product afterwards has those bits too;
 5. the census at width 64 (at width 16 where the row says so): prod > 0, the row's `need` families > 0, its `deny`
    families == 0, and in every product the families of the stages the product has kernels of its own for (NEVER) == 0;
 6. the bits of the handle created without the switch, where the solve's tests already claim them and the switch touches
    nothing but kernels under launch_ldu or the execution mode (same_bits rows).

What differs from the solve's census, and why (launch_trsv / launch_band_cd):
 - gather_scale, scatter_scale, scatter_scale_list, spmm_epi*, spmm_tile*: stages S1 / S3 / S5 / S7 of the solve; the
   product runs k_gather_div / k_spmm_prod / k_scatter_div there.  Every `need` of those families in tv.VARIANTS is
   dropped here, and all of them are denied in every product (NEVER).
 - the tail operator (launch_tail) replaces the solve's recursion below a level; the product always recurses through
   enqueue_prod_level.  So top_gemm / top_reduce / strip_gemm4 launches that come from the tail operator are absent: the
   `default-tail` row has no counterpart, top_gemm=1 launches strip_gemm only (its strip_gemm4 was the tail's), and with
   TOP_ROWS=0 no top_gemm runs at all.  The level top operators (launch_top) do run: the `blocks` rows.
 - with_f is never set: a dense-own L band whose solve takes the F product along (band_cd, coefficient tiles excluded)
   runs on coefficient tiles in the product.  Expectations that named band_cd for that reason do not occur in the rows
   below (they were `lower` columns of TAIL_ROWS=0 rows).

Switches without rows: HIFIR_AMD_TAIL_ROWS (the product never uses the tail operator), SPMM_* and NARROW_* (launch_spmm is
the solve's), FUSE_S1 / FUSE_F / FUSE_S7 taken singly, LIST_EARLY and SKIP_ROWS (they select entries of the band kernels that
the product never asks for; all three fusions off together change the plan and are a row) do not change a product's launches.

PROD_TOL = 1e-11.  The project's bar for the product is 1e-10 (test_gpu_parity.py).  Measured over every case of
this table on an MI355X with the bar at 1e-10, the largest column error against the oracle is 8.1e-14 (`default` on `herm`,
M^H; M: 8.09e-14 -- the SYEIG last level of the complex Hermitian fixture; `symm`, the real one: 2.9e-14); every other
hierarchy stays at or below 6.0e-15 (`kkt`), under every row.  PROD_TOL is the smallest power of ten that is at least 100
times the measured maximum -- the margin the solve's 1e-12 has over its measured 8e-15 -- and never above 1e-10."""
import numpy as np
import pytest

import test_gpu_variants as tv
from test_gpu_variants import CT_ANY, NOCD, NOFUSE, SPARSE_OWN, V, W1, _u
from util import load_hier, rand_rhs

PROD_TOL = 1e-11
MEASURED_MAX = (8.1e-14, "default", "herm", "M^H")  # the run PROD_TOL comes from (module docstring)

WIDTHS = tv.WIDTHS
NEVER = ("gather_scale", "scatter_scale", "scatter_scale_list", "spmm_epi", "spmm_epi_narrow")  # + every spmm_tile* family


# ---- hierarchies: tv.HIERS and the dense kinds of launch_dense_mul that they lack -----------------------------------------
def _lup(name):
    levels = [dict(lv) for lv in load_hier(name)[0]]
    levels[-1]["dense_lup"] = 1  # (the block handed over as an LUP block, as test_gpu_parity.py::test_lup_last_level does)
    return levels


EXTRA = {
    "symm": lambda: load_hier("p2d_32_symm")[0],    # real, is_symm factorization: SYEIG last level
    "herm": lambda: load_hier("herm_24_symm")[0],   # complex Hermitian: SYEIG last level
    "lup": lambda: load_hier("p2d_30_lup")[0],      # real, LUP last level
    "younglup": lambda: _lup("young1c"),            # complex, LUP last level
}
HIER_NAMES = tuple(tv.HIERS) + tuple(EXTRA)


def _levels(name):
    if name in tv.HIERS:
        return tv._levels(name)
    key = ("levels", name)
    if key not in tv._cache:
        levels = EXTRA[name]()
        z = any(np.iscomplexobj(lv["L_vals"]) or np.iscomplexobj(lv["d"]) for lv in levels)
        tv._cache[key] = (levels, np.complex128 if z else np.float64)
    return tv._cache[key]


def _hier(name):
    """levels, the 72-column batch and the oracle's two products: once per hierarchy, never written to."""
    key = ("prod", name)
    if key not in tv._cache:
        from oracle import orc

        levels, dtype = _levels(name)
        n = int(levels[0]["n"])
        X = rand_rhs(np.random.default_rng(43), (n, 72), dtype)
        O = orc.Oracle(levels, dtype=dtype)
        h = dict(name=name, levels=levels, dtype=dtype, X=X, Yo=O.mmultiply_batch(X, rank=-1),
                 YoH=O.mmultiply_batch(X, rank=-1, trans=True))
        O.close()
        for a in (h["X"], h["Yo"], h["YoH"]):
            a.setflags(write=False)
        tv._cache[key] = h
    return tv._cache[key]


# ---- the table --------------------------------------------------------------------------------------------------------
# tv.V: name, env, on, need / deny (width 64), need16 / deny16 (width 16), same_bits + ref, also (further hierarchies that run
# the row for everything but `need`).  The expectations are those of the tv.VARIANTS row of the same name unless a comment
# says otherwise; families of NEVER are left out of `need` (module docstring).
SLICED = ("tuned", "forest", "leaves", "shapes")
STREAMED = ("leaves", "shapes", "forest")
PLAN = ("blocks", "deep", "tuned")
EXEC = ("deep", "blocks", "kkt")

ROWS = [
    # -- default: every hierarchy, every dense kind of launch_dense_mul (QRCP, SYEIG, LUP; real and complex) in batch
    V("default", {}, ("deep", "tuned", "forest", "synth", "kkt", "young", "symm", "herm", "lup", "younglup")),
    V("default-blocks", {}, ("blocks",), need=("band_ct1", "top_gemm", "top_reduce")),
    V("default-leaves", {}, ("leaves",), need=("band_ls", "band_us"), need16=("band_cs_sparse",)),
    V("default-blocksz", {}, ("blocksz",), need=("band_cd_z", "zcombine"), need16=("band_cs_z",)),
    V("default-synthz", {}, ("synthz",), need=("band_cs_z",)),
    V("default-ladder", {}, ("ladder",), need=("band_ct1",)),
    V("default-shapes", {}, ("shapes",), need=("band_ls", "band_us"), need16=("band_cs_sparse",)),
    V("default-ladderz", {}, ("ladderz",), need=("band_cd_z",), need16=("band_cs_z",)),
    V("default-shapesz", {}, ("shapesz",), need=("band_cs_z",)),
    # -- coefficient tiles (widths <= 16 always take one tile: the width check compares ct1 with ct2 / ct4 bit for bit)
    V("ct=0", {"CT": "0"}, ("blocks", "ladder"), need=("band_cd",), deny=CT_ANY, need16=("band_cs",), deny16=CT_ANY),
    V("ct_wide=0", {"CT_WIDE": "0"}, ("blocks", "ladder"), need=("band_ct2",), deny=("band_ct1", "band_ct4"), need16=("band_ct1",),
      deny16=("band_ct2", "band_ct4"), same_bits=True),
    V("ct_wide4=0", {"CT_WIDE": "0", "CT_WIDE4": "0"}, ("blocks", "ladder"), need=("band_ct4",), deny=("band_ct1", "band_ct2"),
      need16=("band_ct1",), deny16=("band_ct2", "band_ct4"), same_bits=True),
    V("ct_real=0", {"CT_REAL": "0"}, ("blocks", "ladder"), need=("band_cd",), deny=CT_ANY),
    # -- column slices
    V("cs=0", {"CS": "0"}, SLICED, need16=("band_cd_sparse",), deny16=("band_cs", "band_cs_sparse"), same_bits=True, also=("blocks",)),
    V("cs=0-ct=0", {"CS": "0", "CT": "0"}, ("blocks",), need16=("band_cd",), deny16=("band_cs", "band_cs_sparse"), same_bits=True,
      ref={"CT": "0"}),
    V("cs_max_wgs", {"CS_MAX_WGS": "100000"}, ("tuned", "forest", "leaves"), need=("band_cs_sparse",),
      deny=("band_cd_sparse", "band_us", "band_ls"), same_bits=True),
    V("cs_max_wgs-ct=0", {"CS_MAX_WGS": "100000", "CT": "0"}, ("blocks",), need=("band_cs",), deny=("band_cd",), same_bits=True,
      ref={"CT": "0"}),
    V("cs_sparse", {"CS_SPARSE": "1", "CD_SPARSE_MIN_ROWS": "0"}, SLICED, need=("band_cs_sparse",),
      deny=("band_us", "band_ls", "band_cd_sparse"), also=("blocks",)),
    # -- streamed sparse-own bands (LS / LS_CHUNK: the same bits are test_gpu_ls_band.py's claim for the solve)
    V("us=0", {"US": "0"}, STREAMED, need=("band_cd_sparse",), deny=("band_us",)),
    V("ls=0", {"LS": "0"}, STREAMED, need=("band_cd_sparse",), deny=("band_ls",), same_bits=True),
    # (forest runs band_ls forwards only, whatever the chunk: the adjoint engine's L is U^H, whose components put their
    #  dependent rows first and are no candidates for streamed sources -- its census shows band_cd_sparse there by default too)
    V("ls_chunk=32", {"LS_CHUNK": "32"}, ("leaves", "shapes"), need=("band_ls",), same_bits=True, also=("forest",)),
    V("cd_sparse_rows=0", {"CD_SPARSE_ROWS": "0"}, STREAMED, need=("trsv_band_p",), deny=SPARSE_OWN),
    # -- the band planner
    V("cd_rows=0", {"CD_ROWS": "0"}, ("blocks", "tuned"), need=("trsv_band_p",), deny=CT_ANY + SPARSE_OWN + ("band_cd", "band_cs"),
      also=("deep",)),
    V("flag-bands", NOCD, PLAN, need=("trsv_band_p",), deny=CT_ANY),
    V("band_pipe=0-flag-bands", _u(NOCD, {"BAND_PIPE": "0"}), PLAN, need=("trsv_band",), deny=("trsv_band_p",) + CT_ANY),
    # (BAND_FUSE / CARRY_WGS decide who runs a band's carried prefix: the extra workgroups of the band kernel before it)
    V("band_fuse=0", {"BAND_FUSE": "0"}, ("blocks",), need=("band_ct1",), also=("deep", "tuned")),
    V("carry_wgs=1", {"CARRY_WGS": "1"}, ("blocks",), need=("band_ct1",), also=("deep", "tuned")),
    # (tv: top_gemm == 1 at width 64, the tail operator's -- the product has none, and without level tops no top_gemm at all)
    V("top_rows=0", {"TOP_ROWS": "0"}, ("blocks",), need=("tri_gemm",), deny=("top_gemm", "top_reduce"), also=("deep", "tuned")),
    V("cd_split_min=1", {"CD_SPLIT_MIN": "1", "CT": "0"}, ("blocks",), need=("band_split_prefix", "band_cd"), also=("deep", "tuned")),
    V("cd_nnz=200", {"CD_NNZ": "200"}, ("blocks",), need=("band_ct1",), also=("deep", "tuned")),
    V("gemm_waves=4", {"GEMM_WAVES": "4", "CD_ROWS": "0", "DENSE_BLOCK": "256"}, ("deep", "tuned"), need=("tri_gemm", "thin_update"),
      also=("blocks",)),
    # -- fusions off: another plan, the same product (tv asks for gather_scale / scatter_scale here: NEVER in a product)
    V("fusions=0", NOFUSE, ("blocks", "leaves"), need=("band_ct1",), also=("synth",)),
    V("fusions=0-z", NOFUSE, ("blocksz",), need=("band_cd_z",)),
    # -- operator products inside the L solve (launch_top; strip_gemm4 under TOP_GEMM=1 was the tail operator's in tv)
    V("top_gemm=1", {"TOP_GEMM": "1"}, ("blocks",), need=("strip_gemm",), deny=("top_gemm", "top_reduce", "strip_gemm4")),
    V("top_gemm=2", {"TOP_GEMM": "2"}, ("blocks",), need=("strip_gemm4",), deny=("top_gemm", "top_reduce", "strip_gemm")),
    V("top_gemm=3", {"TOP_GEMM": "3"}, ("blocks",), need=("strip_gemm4",), deny=("top_gemm", "top_reduce", "strip_gemm")),
    V("top_last", {"TOP_LAST": "1"}, ("blocks",), need=("top_gemm",), deny=("top_reduce",), same_bits=True),
    # -- workgroups that own several components (the same bits on ladder only: the comment in tv.VARIANTS)
    V("band_wgs=1", W1, ("blocks", "ladder"), need=("band_ct1",), same_bits=("ladder",)),
    V("band_wgs=1-sparse", W1, ("leaves", "shapes"), need=("band_cd_sparse",), deny=("band_ls", "band_us"), need16=("band_cs_sparse",)),
    V("band_wgs=1-z", W1, ("blocksz", "ladderz"), need=("band_cd_z",), need16=("band_cs_z",)),
    V("band_wgs=1-ct=0", _u(W1, {"CT": "0"}), ("blocks", "ladder"), need=("band_cd",), deny=CT_ANY, need16=("band_cs",),
      same_bits=("ladder",), ref={"CT": "0"}, also=("leaves", "shapes", "blocksz", "ladderz")),
    # -- complex handles
    V("ct_z", {"CT_Z": "1"}, ("blocksz", "ladderz"), need=("band_ct_z",), deny=("band_cd_z",), need16=("band_ct_z",), also=("kkt",)),
    V("cd_rows_z=48", {"CD_ROWS_Z": "48"}, ("blocksz", "ladderz"), need=("band_cd_z",), need16=("band_cs_z",), also=("kkt",)),
    V("cs=0-z", {"CS": "0"}, ("blocksz", "ladderz"), need16=("band_cd_z",), deny16=("band_cs_z",), also=("kkt",)),
    V("gemm_waves=4-z", {"GEMM_WAVES": "4"}, ("kkt", "blocksz"), need=("tri_gemm", "zcombine"), also=("ladderz",)),
    # -- execution
    V("twin=0", {"TWIN": "0"}, EXEC, same_bits=True),
    V("xcd=0", {"XCD": "0"}, EXEC, same_bits=True),
    V("no_graph", {"NO_GRAPH": "1"}, EXEC, same_bits=True),
    V("device_inverses=0", {"DEVICE_INVERSES": "0"}, EXEC, same_bits=True),
]


# ---- measurements -------------------------------------------------------------------------------------------------------
def _reference(h, env):
    """The two 64-column products of the handle without the row's switch: once per (hierarchy, environment)."""
    key = ("prodref", h["name"], tuple(sorted(env.items())))
    if key not in tv._cache:
        M = tv._handle(h, env)
        X64 = np.ascontiguousarray(h["X"][:, :64])
        tv._cache[key] = dict(Y=M.mmultiply(X64, rank=-1), YH=M.mmultiply(X64, trans=True, rank=-1))
        M.close()
    return tv._cache[key]


def _differs(A, B):
    """None when A has the bits of B, else (NaNs in A, largest relative column difference)"""
    if np.array_equal(A, B):
        return None
    return int(np.isnan(A).sum()), tv._colerr(np.nan_to_num(A), B)


def measure(v, hier):
    """Everything the six checks look at, as plain data (nothing is asserted here)."""
    h = _hier(hier)
    M = tv._handle(h, v.env)
    X = h["X"]
    r = dict(variant=v.name, hier=hier, width_bits=[], replay_bits=[], mixed_bits=[])
    # 1. against the oracle, width 72
    r["err"] = tv._colerr(M.mmultiply(X, rank=-1), h["Yo"])
    r["errH"] = tv._colerr(M.mmultiply(X, trans=True, rank=-1), h["YoH"])
    X64 = np.ascontiguousarray(X[:, :64])
    nan = np.full_like(X64, np.nan)
    for tr in (False, True):
        s = "H" if tr else ""
        Y = M.mmultiply(X64, trans=tr, rank=-1)
        r["Y64" + s] = Y
        r["census64" + s] = M.kernel_census()
        # 2. width independence
        for k in WIDTHS:
            Yk = M.mmultiply(np.ascontiguousarray(X[:, :k]), trans=tr, rank=-1)
            if k == 16:
                r["census16" + s] = M.kernel_census()
            d = _differs(Yk, Y[:, :k])
            if d:
                r["width_bits"].append((s, k) + d)
        d = _differs(M.mmultiply(np.ascontiguousarray(X[:, 40:48]), trans=tr, rank=-1), Y[:, 40:48])
        if d:
            r["width_bits"].append((s, "40:48") + d)
        # 3. replay and stale state
        M.mmultiply(nan, trans=tr, rank=-1)
        d = _differs(M.mmultiply(X64, trans=tr, rank=-1), Y)
        if d:
            r["replay_bits"].append((s,) + d)
    # 4. solves and products interleaved (after the sweep above: more graphs were captured than the cache keeps)
    S1 = M.solve_mrhs(X64)
    P = M.mmultiply(X64, rank=-1)
    M.solve_mrhs(X64, trans=True)
    PH = M.mmultiply(X64, trans=True, rank=-1)
    S2 = M.solve_mrhs(X64)
    for what, A, B in (("solve", S2, S1), ("product", P, r["Y64"]), ("productH", PH, r["Y64H"]),
                       ("product again", M.mmultiply(X64, rank=-1), r["Y64"]),
                       ("productH again", M.mmultiply(X64, trans=True, rank=-1), r["Y64H"])):
        d = _differs(A, B)
        if d:
            r["mixed_bits"].append((what,) + d)
    M.close()
    return r


def judge(v, r, tol=None):
    tol = PROD_TOL if tol is None else tol
    h = _hier(r["hier"])
    print(f"PRODUCT {v.name} on {r['hier']}: relerr {r['err']:.2e} transposed {r['errH']:.2e}")
    for k in ("census64", "census64H", "census16", "census16H"):
        print(f"  {k}: {tv._fmt(r[k])}")
    for k in ("width_bits", "replay_bits", "mixed_bits"):
        if r[k]:
            print(f"  {k}: {r[k]}")
    assert r["err"] <= tol and r["errH"] <= tol, (r["err"], r["errH"])
    assert not r["width_bits"], r["width_bits"]
    assert not r["replay_bits"], r["replay_bits"]
    assert not r["mixed_bits"], r["mixed_bits"]
    reach = r["hier"] in v.on  # (an `also` hierarchy: the deny lists only)
    for c in ("census64", "census64H", "census16", "census16H"):
        wide = c.startswith("census64")
        assert r[c]["prod"] > 0, (c, "prod", "never launched")
        for f in (v.need if wide else v.need16) if reach else ():
            assert r[c][f] > 0, (c, f, "never launched")
        for f in v.deny if wide else v.deny16:
            assert r[c][f] == 0, (c, f, r[c][f])
        for f in r[c]:
            if f in NEVER or f.startswith("spmm_tile"):
                assert r[c][f] == 0, (c, f, r[c][f], "a kernel of the solve's S1 / S3 / S5 / S7 stages in a product")
    if v.same_bits is True or (v.same_bits and r["hier"] in v.same_bits):
        ref = _reference(h, v.ref)
        assert np.array_equal(r["Y64"], ref["Y"]), tv._colerr(r["Y64"], ref["Y"])
        assert np.array_equal(r["Y64H"], ref["YH"]), tv._colerr(r["Y64H"], ref["YH"])


CASES = [pytest.param(v, hier, id=f"{v.name}-{hier}") for v in ROWS for hier in v.on + v.also]


@pytest.mark.gpu
@pytest.mark.parametrize("v,hier", CASES)
def test_product(v, hier):
    judge(v, measure(v, hier))


# ---- the table guard (CPU) ----------------------------------------------------------------------------------------------
def test_table_is_well_formed():
    names = [v.name for v in ROWS]
    assert len(names) == len(set(names))
    for v in ROWS:
        assert v.on and set(v.on + v.also) <= set(HIER_NAMES), v.name
        assert not (v.lower or v.count64 or v.bands or v.xfail), (v.name, "columns of tv.V this table does not read")
        assert set(v.env) <= tv.switches_in_table() | {"LS", "LS_CHUNK"}, v.name
        for f in v.need + v.need16:
            assert f not in NEVER and not f.startswith("spmm_tile"), (v.name, f)
    covered = {hier for v in ROWS if not v.env for hier in v.on}
    assert covered == set(HIER_NAMES), sorted(set(HIER_NAMES) - covered)
