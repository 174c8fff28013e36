"""GPU (-m gpu): every kernel variant the engine can choose, at small size, against the oracle.

The engine picks kernels by problem size and by the HIFIR_AMD_* switches a handle is created under.  On the committed
fixtures (at most 10,000 rows) the default mode never launches several kernels the 1M-row workloads spend their time in:
the recursion below level 0 (replaced by the tail operator), the per-wave tiled Schur product, the wide coefficient tiles,
the RB = 2 instantiations, and whatever a switch selects.  This file is one table of variants: the environment of the
handle, the hierarchies it runs on, the kernel families that must (and must not) have been launched according to the
launch census (HIF.kernel_census), and five checks per (variant, hierarchy):

 1. width 100 (one full tile and one of 36 columns, two lanes), forwards and conjugate-transposed, every column within
    1e-12 of the oracle (TOL of test_gpu_parity.py; the same bar for every variant);
 2. a column's bits do not depend on the batch width: widths 1, 16, 17, 32, 33, 48, 49 against the 64-column solve, and
    columns 40:48 on their own (this compares the one-tile kernels with the wide ones, the sliced bands with the full
    ones and the narrow Schur product with the wide one bit for bit);
 3. apply, apply an all-NaN batch of the same shape, apply again: the third result has the bits of the first;
 4. the census: required families > 0, forbidden families == 0 at width 64 (and at width 16 where the row says so) --
    a row whose kernel does not run FAILS, so a planner threshold cannot move a test into vacuity unseen;
 5. the bits of the handle without the switch, only where the project claims them (SAME_BITS rows).

The oracle's answers do not depend on the environment: they are computed once per hierarchy and shared.

The SHAPE of the work varies too: `ladder` / `ladderz` give the dense-own component kernels every component size from 9 to
128 rows (every strip count, tile remainder and operand padding), `shapes` / `shapesz` give the sparse-own ones components
by source / dependent-row class in two tiers with outside entries (util.py; test_shape_ladders_host.py asserts on the CPU
which classes arrive), and the band_wgs=1 rows chain several components onto every workgroup (the kernels' loop over a
workgroup's components, which a default plan enters only with more than 8,192 components in a band).

Not reached here: the grid cap of the per-wave Schur product (k_spmm_tile with more than 16,384 blocks, i.e. more than
262,144 rows in one coupling block) stays with test_gpu_fullsize.py.  Every tiled coupling block of this table comes from
util.shared_coupling (exactly four column groups per 16-row block) and every other one from sp.random (about 18 nonzeros per
row, at most 4,500 rows): blocks of 0 ... 68 groups with padded last groups, rows of 0 ... 200 nonzeros and a wave's second
row in k_spmm_epi are test_gpu_schur_edges.py's subject, which also holds the bits claimed by the narrow_tiles=0 and
narrow_spmm=0 rows on those shapes.

test_every_switch_has_a_row (CPU) keeps the table honest: every HIFIR_AMD_* name the engine reads is either in a row or
in NOT_VARIANTS with a reason, and is listed in the README's knob paragraph."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from util import (clustered_tri, dense_block, forest, forest_levels, ladder_levels, load_hier, rand_rhs, rand_tri, shapes_levels,
                  shared_coupling, synth_level, transposed_pattern)

TOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PFX = "HIFIR_AMD_"
BASE = {"DENSE_BLOCK": "2048", "MIN_LOGR": "6"}
WIDTHS = (1, 16, 17, 32, 33, 48, 49)


# ---- hierarchies ------------------------------------------------------------------------------------------------------
def _synth(dtype):
    """Three levels + dense block, 6,000 rows: level 0 random thin triangles, level 1 forests of 64-row components with E
    and F (dense-own component bands below level 0 with the fused F product -- no golden fixture has them), level 2."""
    rng = np.random.default_rng(31)
    n0, m0, m1, m2 = 6000, 4500, 1100, 250
    n1 = n0 - m0
    n2 = n1 - m1
    nd = n2 - m2
    rs = np.random.RandomState

    def coupling(r, c, density, seed):
        return sp.random(r, c, density=density, random_state=rs(seed), format="csr")

    lv0 = synth_level(m0, n0, rand_tri(m0, 0.001, True, rng, dtype=dtype), rand_tri(m0, 0.001, False, rng, dtype=dtype),
                      coupling(n1, m0, 0.004, 1), coupling(m0, n1, 0.004, 2), rng, dtype=dtype)
    lv1 = synth_level(m1, n1, forest(m1, 40, 24, rng, True), forest(m1, 40, 24, rng, False),
                      coupling(n2, m1, 0.02, 3), coupling(m1, n2, 0.02, 4), rng, dtype=dtype)
    lv2 = synth_level(m2, n2, rand_tri(m2, 0.04, True, rng, dtype=dtype), rand_tri(m2, 0.04, False, rng, dtype=dtype),
                      coupling(nd, m2, 0.05, 5), coupling(m2, nd, 0.05, 6), rng, dtype=dtype)
    lv2["dense_n"], lv2["dense"] = nd, dense_block(nd, 6.0, rng, dtype, scale=0.2)
    return [lv0, lv1, lv2]


def _blocks(dtype):
    """Three levels + dense block, 6,000 rows, built for the kernels no golden fixture reaches: levels 0 and 1 have more
    than 2,048 rows of 24-row clusters with five nonzeros per row (dense-own component bands of more than 96 components,
    on level 1 with F present), a crown of rows no component holds (the level's top operator) and coupling blocks whose
    rows share columns (the tiled Schur products on level 0 too)."""
    rng = np.random.default_rng(32)
    n0, m0, m1, m2 = 6000, 3400, 2200, 250
    n1 = n0 - m0
    n2 = n1 - m1
    nd = n2 - m2
    L0, L1 = clustered_tri(m0, 24, 6, 160, rng), clustered_tri(m1, 24, 6, 120, rng)
    lv0 = synth_level(m0, n0, L0, transposed_pattern(L0, rng), shared_coupling(n1, m0, rng),
                      shared_coupling(m0, n1, rng), rng, dtype=dtype)
    lv1 = synth_level(m1, n1, L1, transposed_pattern(L1, rng), shared_coupling(n2, m1, rng),
                      shared_coupling(m1, n2, rng), rng, dtype=dtype)
    lv2 = synth_level(m2, n2, rand_tri(m2, 0.04, True, rng, dtype=dtype), rand_tri(m2, 0.04, False, rng, dtype=dtype),
                      sp.random(nd, m2, density=0.05, random_state=np.random.RandomState(5), format="csr"),
                      sp.random(m2, nd, density=0.05, random_state=np.random.RandomState(6), format="csr"), rng, dtype=dtype)
    lv2["dense_n"], lv2["dense"] = nd, dense_block(nd, 6.0, rng, dtype, scale=0.2)
    return [lv0, lv1, lv2]


def _leaves(dtype):
    """Two levels + dense block, 7,000 rows, every triangle ONE band of independent clusters (no rest, no top, no carried
    prefix) and thin F blocks: the plans whose second L solve takes the F product along (with_f).  Level 0: 4,400 rows with
    two nonzeros per row (sparse-own components), level 1: 2,300 rows with five (dense-own components, F present)."""
    rng = np.random.default_rng(33)
    n0, m0, m1 = 7000, 4400, 2300
    n1 = n0 - m0
    nd = n1 - m1
    rs = np.random.RandomState
    L0, L1 = clustered_tri(m0, 24, 2, 0, rng, cross=0.0), clustered_tri(m1, 24, 6, 0, rng, cross=0.0)
    lv0 = synth_level(m0, n0, L0, transposed_pattern(L0, rng), shared_coupling(n1, m0, rng),
                      sp.random(m0, n1, density=0.001, random_state=rs(2), format="csr"), rng, dtype=dtype)
    lv1 = synth_level(m1, n1, L1, transposed_pattern(L1, rng), shared_coupling(nd, m1, rng),
                      sp.random(m1, nd, density=0.01, random_state=rs(4), format="csr"), rng, dtype=dtype)
    lv1["dense_n"], lv1["dense"] = nd, dense_block(nd, 6.0, rng, dtype, scale=0.2)
    return [lv0, lv1]


HIERS = {
    "deep": lambda: load_hier("p2d_64_deep")[0],     # 4,096 rows, three levels + dense block, real
    "tuned": lambda: load_hier("p2d_100_tuned")[0],  # 10,000 rows, three levels, real
    "forest": forest_levels,                         # 7,000 rows, one level of 180-row components + dense block, real
    "synth": lambda: _synth(np.float64),
    "blocks": lambda: _blocks(np.float64),
    "leaves": lambda: _leaves(np.float64),
    "kkt": lambda: load_hier("kkt_26")[0],           # complex, 2,028 rows
    "young": lambda: load_hier("young1c")[0],        # complex, 841 rows
    "synthz": lambda: _synth(np.complex128),
    "blocksz": lambda: _blocks(np.complex128),
    # the shape ladders (util.py; test_shape_ladders_host.py asserts on the CPU what the planner makes of them)
    "ladder": ladder_levels,                         # 8,520 rows, one level: dense-own components of 9 ... 128 rows, each size once
    "shapes": shapes_levels,                         # 7,731 rows, one level: sparse-own components by source / dependent-row class, two tiers
    "ladderz": lambda: ladder_levels(np.complex128),
    "shapesz": lambda: shapes_levels(np.complex128),
}
REAL = ("deep", "tuned", "forest", "synth", "blocks", "leaves")
CPLX = ("kkt", "young", "synthz", "blocksz")

_cache = {}


def _levels(name):
    """levels and their value type: once per hierarchy (test_gpu_product.py builds its own batch on the same levels)."""
    key = ("levels", name)
    if key not in _cache:
        levels = HIERS[name]()
        z = any(np.iscomplexobj(lv["L_vals"]) or np.iscomplexobj(lv["d"]) for lv in levels)
        _cache[key] = (levels, np.complex128 if z else np.float64)
    return _cache[key]


def _hier(name):
    """levels, the 100-column batch and the oracle's two answers: once per hierarchy, never written to."""
    key = ("hier", name)
    if key not in _cache:
        from oracle import orc

        levels, dtype = _levels(name)
        n = int(levels[0]["n"])
        B = rand_rhs(np.random.default_rng(41), (n, 100), dtype)
        O = orc.Oracle(levels, dtype=dtype)
        h = dict(name=name, levels=levels, dtype=dtype, B=B, Xo=O.solve_batch(B, threads=4),
                 XoT=O.solve_batch(B, threads=4, trans=True))
        for a in (h["B"], h["Xo"], h["XoT"]):
            a.setflags(write=False)
        _cache[key] = h
    return _cache[key]


# ---- the table --------------------------------------------------------------------------------------------------------
class V:
    """One variant.  env: the switches (without the HIFIR_AMD_ prefix) on top of BASE; on: the hierarchies that reach the
    kernel; need / deny: census families that must be > 0 / == 0 at width 64; need16 / deny16: the same at width 16; lower:
    families that must run on a level >= 1; count64: exact launch counts at width 64; also: further hierarchies that run the
    variant for checks 1-3 and 5 and the deny lists (whatever kernels they reach: need / lower / count64 are not asked); same_bits: the handle has the bits of the handle created under `ref` (the environment without the
    switch), a claim of DESIGN.md, a code comment or an existing test -- True: on every hierarchy of the row, a tuple: on
    those hierarchies only; bands: the switch changes the band count of the
    plan (stats()["bands"]; or the statistic named) against `ref`; xfail: a finding that is not fixed yet (strict)."""

    def __init__(self, name, env, on, need=(), deny=(), need16=(), deny16=(), lower=(), count64=None, same_bits=False, ref=None,
                 bands=False, also=(), xfail=None):
        self.name, self.env, self.on, self.also, self.count64 = name, dict(env), tuple(on), tuple(also), dict(count64 or {})
        self.need, self.deny, self.need16, self.deny16, self.lower = need, deny, need16, deny16, lower
        self.same_bits, self.ref, self.bands, self.xfail = same_bits, dict(ref or {}), bands, xfail


T0 = {"TAIL_ROWS": "0"}
W1 = {"BAND_WGS": "1"}  # eight workgroups per component band: every band of more than eight components chains them (c_first .. c_last)
NOFUSE = {"FUSE_S1": "0", "FUSE_F": "0", "FUSE_S7": "0"}
NOCD = {"CD_ROWS": "0", "TOP_ROWS": "0"}  # the depth-cut flag bands of round 1 everywhere
TILE_ANY = ("spmm_tile_rb1", "spmm_tile_rb2", "spmm_tile4_rb1", "spmm_tile4_rb2")
CT_ANY = ("band_ct1", "band_ct2", "band_ct4")
SPARSE_OWN = ("band_cd_sparse", "band_cs_sparse", "band_us", "band_ls")
GOLD = ("deep", "tuned")
ALLR = ("deep", "tuned", "forest", "synth", "blocks", "leaves")


def _u(*ds):
    out = {}
    for d in ds:
        out.update(d)
    return out


VARIANTS = [
    V("default", {}, REAL + CPLX),
    # (the tail operator is formed and used: a probe that refuses it at finalize would leave the recursion, silently right)
    V("default-tail", {}, GOLD + ("synth",), need=("top_gemm", "top_reduce"), lower=("top_gemm", "top_reduce")),
    V("default-blocks", {}, ("blocks",), need=("band_ct1", "spmm_tile4_rb1", "top_gemm", "top_reduce", "scatter_scale_list")),
    V("default-leaves", {}, ("leaves",), need=("band_ls", "band_us", "spmm_tile4_rb1"), need16=("band_cs_sparse",)),
    V("default-blocksz", {}, ("blocksz",), need=("band_cd_z", "spmm_tile_z", "zcombine"), need16=("band_cs_z",), lower=("band_cd_z",)),
    V("default-synthz", {}, ("synthz",), need=("band_cs_z",)),
    # (the shape ladders: every dense-own component size 9 ... 128, the sparse-own shapes of test_shape_ladders_host.py)
    V("default-ladder", {}, ("ladder",), need=("band_ct1",)),
    V("default-shapes", {}, ("shapes",), need=("band_ls", "band_us"), need16=("band_cs_sparse",)),
    V("default-ladderz", {}, ("ladderz",), need=("band_cd_z",), need16=("band_cs_z",)),
    V("default-shapesz", {}, ("shapesz",), need=("band_cs_z",)),
    # -- the recursion through every level (the tail operator off)
    V("tail0", T0, ("deep", "blocks"), lower=("spmm_tile4_rb1", "trsv_wide", "tri_gemm"), also=("tuned", "synth", "leaves", "ladder")),
    V("tail0-blocks", T0, ("blocks",), need=("top_gemm", "top_reduce"),
      lower=("band_ct1", "spmm_tile4_rb1", "top_gemm", "top_reduce", "scatter_scale_list")),
    # (leaves: the second L solve of both levels takes F along -- one Schur product per level and direction is left)
    V("tail0-leaves", T0, ("leaves",), need=("spmm_tile4_rb1",), lower=("band_cd", "band_ct1"), count64={"spmm_epi": 0}),
    V("tail0-top0-cdnnz0", _u(T0, {"TOP_ROWS": "0", "CD_NNZ": "0"}), ("deep", "blocks", "tuned", "synth"),
      deny=("top_gemm", "top_reduce"), lower=("trsv_wide", "tri_gemm"), also=("leaves",)),
    V("tail0-z", T0, ("blocksz",), lower=("spmm_tile_z", "band_cd_z"), also=("synthz",)),
    # -- fusions off
    V("tail0-fuse_s1=0", _u(T0, {"FUSE_S1": "0"}), ("deep", "blocks", "synth", "leaves"), need=("gather_scale",), lower=("gather_scale",)),
    V("tail0-fuse_f=0", _u(T0, {"FUSE_F": "0"}), ("leaves",), need=("spmm_epi",), lower=("spmm_epi", "band_ct1"), deny=("band_cd",),
      also=("deep", "blocks", "synth", "forest")),
    V("tail0-fuse_s7=0", _u(T0, {"FUSE_S7": "0"}), ("deep", "blocks", "synth", "leaves"), need=("scatter_scale",),
      deny=("scatter_scale_list",), lower=("scatter_scale",)),
    V("tail0-fusions=0", _u(T0, {"FUSE_S1": "0", "FUSE_F": "0", "FUSE_S7": "0"}), ("deep", "tuned", "blocks", "synth", "leaves"),
      need=("gather_scale", "scatter_scale"), deny=("scatter_scale_list",), lower=("gather_scale", "scatter_scale")),
    V("tail0-list_early", _u(T0, {"LIST_EARLY": "1"}), ("blocks", "synth"), need=("scatter_scale_list",), also=("deep", "leaves")),
    V("fusions=0-z", {"FUSE_S1": "0", "FUSE_F": "0", "FUSE_S7": "0"}, ("kkt", "synthz", "blocksz"),
      need=("gather_scale", "scatter_scale"), deny=("scatter_scale_list",)),
    # -- wide coefficient tiles (widths <= 16 always take one tile: the width check compares ct1 with ct2 / ct4 bit for bit)
    V("ct_wide=0", {"CT_WIDE": "0"}, ("blocks", "ladder"), need=("band_ct2",), deny=("band_ct1", "band_ct4"), need16=("band_ct1",),
      deny16=("band_ct2", "band_ct4"), same_bits=True, also=GOLD),
    V("ct_wide4=0", {"CT_WIDE": "0", "CT_WIDE4": "0"}, ("blocks", "ladder"), need=("band_ct4",), deny=("band_ct1", "band_ct2"),
      need16=("band_ct1",), deny16=("band_ct2", "band_ct4"), same_bits=True, also=GOLD),
    V("tail0-ct_wide=0", _u(T0, {"CT_WIDE": "0"}), ("blocks", "leaves"), need=("band_ct2",), lower=("band_ct2",), same_bits=True,
      ref=T0, also=("deep",)),
    V("tail0-ct_wide4=0", _u(T0, {"CT_WIDE": "0", "CT_WIDE4": "0"}), ("blocks", "leaves"), need=("band_ct4",), lower=("band_ct4",),
      same_bits=True, ref=T0, also=("deep",)),
    V("ct=0", {"CT": "0"}, ("blocks", "ladder"), need=("band_cd",), deny=CT_ANY, need16=("band_cs",), deny16=CT_ANY, also=GOLD),
    V("tail0-ct=0", _u(T0, {"CT": "0"}), ("blocks", "leaves"), deny=CT_ANY, lower=("band_cd",)),
    V("ct_real=0", {"CT_REAL": "0"}, ("blocks",), need=("band_cd",), deny=CT_ANY),
    # -- Schur products
    V("spmm_split=0", {"SPMM_SPLIT": "0"}, ("blocks", "leaves"), need=("spmm_tile_rb1",), deny=("spmm_tile4_rb1",),
      need16=("spmm_tile_rb1",), also=GOLD + ("forest",)),
    V("spmm_split_blocks=0", {"SPMM_SPLIT_BLOCKS": "0"}, ("blocks", "leaves"), need=("spmm_tile_rb1",), deny=("spmm_tile4_rb1",),
      also=GOLD),
    V("spmm_split=0-rb2", {"SPMM_SPLIT": "0", "SPMM_RB": "2"}, ("blocks", "leaves"), need=("spmm_tile_rb2",),
      deny=("spmm_tile_rb1", "spmm_tile4_rb1", "spmm_tile4_rb2"), need16=("spmm_tile_rb2",), also=GOLD),
    V("spmm_split_blocks=0-rb2", {"SPMM_SPLIT_BLOCKS": "0", "SPMM_RB": "2"}, ("blocks", "leaves"), need=("spmm_tile_rb2",),
      deny=("spmm_tile_rb1", "spmm_tile4_rb1", "spmm_tile4_rb2"), also=GOLD),
    V("spmm_rb2", {"SPMM_RB": "2"}, ("blocks", "leaves"), need=("spmm_tile4_rb2",), deny=("spmm_tile4_rb1",), need16=("spmm_tile4_rb2",),
      also=GOLD),
    V("tail0-spmm_split=0", _u(T0, {"SPMM_SPLIT": "0"}), ("deep", "blocks"), need=("spmm_tile_rb1",), deny=("spmm_tile4_rb1",),
      lower=("spmm_tile_rb1",)),
    V("tail0-spmm_split=0-rb2", _u(T0, {"SPMM_SPLIT": "0", "SPMM_RB": "2"}), ("deep", "blocks"), need=("spmm_tile_rb2",),
      lower=("spmm_tile_rb2",)),
    V("tail0-spmm_rb2", _u(T0, {"SPMM_RB": "2"}), ("deep", "blocks"), need=("spmm_tile4_rb2",), lower=("spmm_tile4_rb2",)),
    V("spmm_tiles=0", {"SPMM_TILES": "0"}, ("blocks", "leaves", "blocksz"), need=("spmm_epi",), deny=TILE_ANY + ("spmm_tile_z",),
      need16=("spmm_epi_narrow",), also=GOLD + ("kkt",)),
    V("spmm_tiles_z=0", {"SPMM_TILES_Z": "0"}, ("blocksz",), need=("spmm_epi",), deny=("spmm_tile_z",), also=("kkt", "young", "synthz")),
    V("narrow_spmm=0", {"NARROW_SPMM": "0"}, ("deep", "tuned", "kkt"), need16=("spmm_epi",), deny16=("spmm_epi_narrow",),
      same_bits=True, also=("blocks", "leaves")),
    V("narrow_tiles=0", {"NARROW_TILES": "0"}, ("blocks", "leaves"), need=("spmm_tile4_rb1",), need16=("spmm_tile4_rb1",),
      same_bits=True, also=GOLD),
    V("tail0-narrow_tiles=0-split=0", _u(T0, {"NARROW_TILES": "0", "SPMM_SPLIT": "0"}), ("deep", "blocks"), need16=("spmm_tile_rb1",),
      same_bits=True, ref=_u(T0, {"SPMM_SPLIT": "0"})),
    # -- column slices
    V("cs=0", {"CS": "0"}, ("tuned", "forest", "leaves", "shapes"), need16=("band_cd_sparse",), deny16=("band_cs", "band_cs_sparse"),
      same_bits=True, also=("blocks", "shapesz")),
    V("cs=0-ct=0", {"CS": "0", "CT": "0"}, ("blocks",), need16=("band_cd",), deny16=("band_cs", "band_cs_sparse"), same_bits=True,
      ref={"CT": "0"}),
    V("cs_max_wgs", {"CS_MAX_WGS": "100000"}, ("tuned", "forest", "leaves"), need=("band_cs_sparse",), deny=("band_cd_sparse", "band_us", "band_ls"),
      same_bits=True),
    V("cs_max_wgs-ct=0", {"CS_MAX_WGS": "100000", "CT": "0"}, ("blocks",), need=("band_cs",), deny=("band_cd",), same_bits=True,
      ref={"CT": "0"}),
    V("tail0-cs_max_wgs", _u(T0, {"CS_MAX_WGS": "100000"}), ("leaves",), need=("band_cs", "band_cs_sparse"), lower=("band_cs",),
      same_bits=True, ref=T0),
    V("cs_sparse", {"CS_SPARSE": "1", "CD_SPARSE_MIN_ROWS": "0"}, ("deep", "tuned", "forest", "leaves", "shapes"), need=("band_cs_sparse",),
      deny=("band_us", "band_ls", "band_cd_sparse"), also=("shapesz",)),
    V("us=0", {"US": "0"}, ("tuned", "forest", "leaves", "shapes"), need=("band_cd_sparse",), deny=("band_us",), also=("shapesz",)),
    V("cd_sparse_min_rows=0", {"CD_SPARSE_MIN_ROWS": "0"}, ("deep", "shapes"), need=("band_us", "band_ls"), need16=("band_cs_sparse",),
      also=("shapesz",)),
    # -- operator products
    V("top_gemm=1", {"TOP_GEMM": "1"}, ("blocks",), need=("strip_gemm", "strip_gemm4"), deny=("top_gemm", "top_reduce"), also=GOLD),
    V("top_gemm=2", {"TOP_GEMM": "2"}, ("blocks",) + GOLD, need=("strip_gemm4",), deny=("top_gemm", "top_reduce", "strip_gemm")),
    V("top_gemm=3", {"TOP_GEMM": "3"}, ("blocks",) + GOLD, need=("strip_gemm4",), deny=("top_gemm", "top_reduce", "strip_gemm")),
    V("tail0-top_gemm=1", _u(T0, {"TOP_GEMM": "1"}), ("blocks",), need=("strip_gemm",), deny=("top_gemm", "top_reduce", "strip_gemm4"),
      lower=("strip_gemm",)),
    V("tail0-top_gemm=2", _u(T0, {"TOP_GEMM": "2"}), ("blocks",), need=("strip_gemm4",), deny=("top_gemm", "top_reduce", "strip_gemm"),
      lower=("strip_gemm4",)),
    V("tail0-top_gemm=3", _u(T0, {"TOP_GEMM": "3"}), ("blocks",), need=("strip_gemm4",), deny=("top_gemm", "top_reduce", "strip_gemm"),
      lower=("strip_gemm4",)),
    V("top_last", {"TOP_LAST": "1"}, ("blocks",) + GOLD, need=("top_gemm",), deny=("top_reduce",), same_bits=True),
    V("tail0-top_last", _u(T0, {"TOP_LAST": "1"}), ("blocks",), need=("top_gemm",), deny=("top_reduce",), lower=("top_gemm",),
      same_bits=True, ref=T0),
    V("tail0-top_wgs=0", _u(T0, {"TOP_WGS": "0"}), ("blocks",), also=("deep", "tuned", "synth", "leaves")),
    V("tail0-top_wgs=big", _u(T0, {"TOP_WGS": "100000"}), ("blocks",), need=("top_gemm",), lower=("top_gemm",),
      also=("deep", "tuned", "synth", "leaves")),
    V("gemm_waves=4", {"GEMM_WAVES": "4", "CD_ROWS": "0", "DENSE_BLOCK": "256"}, GOLD, need=("tri_gemm", "thin_update"), also=("blocks",)),
    V("gemm_waves=8", {"GEMM_WAVES": "8", "CD_ROWS": "0", "DENSE_BLOCK": "256"}, GOLD, need=("tri_gemm", "thin_update"), also=("blocks",)),
    V("gemm_waves=4-z", {"GEMM_WAVES": "4"}, ("kkt", "young", "blocksz"), need=("tri_gemm", "zcombine")),
    # (several blocks per thin band on a complex handle: the blocks behind a band's first take their right-hand side from
    # k_thin_update -- at the default block size every band of the complex fixtures is one block)
    V("dense_block=256-z", {"DENSE_BLOCK": "256"}, ("kkt",), need=("tri_gemm", "thin_update", "zcombine")),
    # -- the band planner
    V("band_pipe=0", {"BAND_PIPE": "0"}, ("blocks", "leaves") + GOLD, need=("gather_scale",), deny=("trsv_band_p",)),
    V("band_pipe=0-flag-bands", _u(NOCD, {"BAND_PIPE": "0"}), ("blocks",) + GOLD, need=("trsv_band",), deny=("trsv_band_p",) + CT_ANY),
    V("cd_rows=0", {"CD_ROWS": "0"}, ("tuned", "forest", "blocks", "leaves"), need=("trsv_band_p",),
      deny=CT_ANY + SPARSE_OWN + ("band_cd", "band_cs"), bands=True, also=("deep",)),
    V("flag-bands", NOCD, ("blocks",) + GOLD, need=("trsv_band_p",), deny=CT_ANY),
    V("band_fuse=0", {"BAND_FUSE": "0"}, ("blocks", "forest") + GOLD),
    V("band_fuse=0-flag-bands", _u(NOCD, {"BAND_FUSE": "0"}), ("blocks",) + GOLD, need=("trsv_band_p",)),
    V("cd_sparse_rows=0", {"CD_SPARSE_ROWS": "0"}, ("tuned", "forest", "leaves"), need=("trsv_band_p",), deny=SPARSE_OWN),
    V("carry_wgs=1", {"CARRY_WGS": "1"}, ("blocks", "forest") + GOLD),
    V("cd_fuse_wgs=0", {"CD_FUSE_WGS": "0"}, ("blocks", "forest") + GOLD),
    V("band_fuse_wgs=1", {"BAND_FUSE_WGS": "1"}, ("blocks",) + GOLD),
    V("band_fuse_wgs=1-flag-bands", _u(NOCD, {"BAND_FUSE_WGS": "1"}), ("blocks",) + GOLD),
    V("thin_rows=8", _u(NOCD, {"THIN_ROWS": "8"}), ("blocks",) + GOLD, bands=True, ref=NOCD),
    V("band_depth=4", _u(NOCD, {"BAND_DEPTH": "4"}), ("blocks",) + GOLD, bands=True, ref=NOCD),
    V("band_weight=16", _u(NOCD, {"BAND_WEIGHT": "16"}), ("blocks",) + GOLD, bands=True, ref=NOCD),
    V("band_wgs=4", _u(NOCD, {"BAND_WGS": "4"}), ("blocks",) + GOLD, bands="band_workgroups", ref=NOCD),
    V("cd_split_min=1", {"CD_SPLIT_MIN": "1", "CT": "0"}, ("blocks",), need=("band_split_prefix", "band_cd"), also=GOLD),
    V("cd_split_wgs=0", {"CD_SPLIT_MIN": "1", "CT": "0", "CD_SPLIT_WGS": "0"}, ("blocks",), need=("band_cd",), deny=("band_split_prefix",),
      same_bits=True, ref={"CT": "0"}),
    V("cd_nnz=0", {"CD_NNZ": "0"}, ("blocks",) + GOLD),
    V("cd_nnz=200", {"CD_NNZ": "200"}, ("blocks",), need=("band_ct1",), bands=True),
    V("cd_rows=16", {"CD_ROWS": "16"}, ("blocks",), need=("band_ct1",), bands="band_workgroups"),
    # (the largest components: the LDS layouts are built for 256 rows, and k_band_ct with two column tiles then needs more
    # than 64 KB -- every instance gets its limit from the layouts, not from a list kept by hand)
    V("cd_rows=240-ct_wide=0", {"CD_ROWS": "240", "CT_WIDE": "0"}, ("blocks",), need=("band_ct2",)),
    V("cd_rows=240", {"CD_ROWS": "240"}, ("blocks",), need=("band_ct1",)),
    V("top_rows=0", {"TOP_ROWS": "0"}, ("blocks",), need=("tri_gemm",), count64={"top_gemm": 1}, also=GOLD),
    V("device_inverses=0", {"DEVICE_INVERSES": "0"}, ("deep", "blocks", "kkt", "blocksz"), same_bits=True),
    # -- the band planner, complex handles
    V("cd_rows_z=48", {"CD_ROWS_Z": "48"}, ("blocksz", "ladderz"), need=("band_cd_z",), need16=("band_cs_z",), also=("kkt", "young", "synthz")),
    V("cd_rows_z=16", {"CD_ROWS_Z": "16"}, ("blocksz",), need=("band_cd_z",), bands="band_workgroups"),
    V("cd_sparse_rows_z=64", {"CD_SPARSE_ROWS_Z": "64"}, ("synthz",), need=("band_cs_z",), bands="band_workgroups", also=("kkt", "young", "blocksz")),
    # (an odd row count: the LDS layout of k_band_cs_z is built for the next even one, so that its own values stay 8-byte aligned)
    V("cd_sparse_rows_z=63", {"CD_SPARSE_ROWS_Z": "63"}, ("synthz",), need=("band_cs_z",), also=("shapesz",)),
    V("cd_nnz_z", {"CD_NNZ_Z": "200"}, ("blocksz",), need=("band_cd_z",), bands="band_workgroups", also=("kkt", "young", "synthz")),
    V("ct_z", {"CT_Z": "1"}, ("blocksz",), need=("band_ct_z",), deny=("band_cd_z",), need16=("band_ct_z",), lower=("band_ct_z",),
      also=("kkt", "young", "synthz")),
    V("ct_z-cd_rows_z=48", {"CT_Z": "1", "CD_ROWS_Z": "48"}, ("blocksz",), need=("band_ct_z",), also=("kkt", "young")),
    V("ct_z-cd_sparse_rows_z=64", {"CT_Z": "1", "CD_SPARSE_ROWS_Z": "64"}, ("blocksz",), need=("band_ct_z",), also=("synthz", "kkt")),
    V("ct_z-cd_nnz_z", {"CT_Z": "1", "CD_NNZ_Z": "200"}, ("blocksz",), need=("band_ct_z",), also=("kkt", "young")),
    V("cs=0-z", {"CS": "0"}, ("blocksz",), need16=("band_cd_z",), deny16=("band_cs_z",), also=("kkt", "young")),
    V("tail0-ct_z", _u(T0, {"CT_Z": "1"}), ("blocksz",), lower=("band_ct_z", "spmm_tile_z")),
    V("ct_z-ladderz", {"CT_Z": "1"}, ("ladderz",), need=("band_ct_z",), deny=("band_cd_z",), need16=("band_ct_z",)),
    # -- workgroups that own several components (the kernels' loop c_first .. c_last with LDS reused from one component to
    # the next; by default only a band of more than 8,192 components has them).  test_band_wgs_rows_share_workgroups asserts
    # for every hierarchy of these rows that the plan does chain components; test_shape_ladders_host.py that EVERY component
    # band of blocks, leaves, forest, ladder and shapes does (so the streamed kernels, one component per workgroup by
    # construction, must step aside: the deny list of the sparse row).
    # The bits of the handle without the switch are claimed on ladder only.  There the switch moves whole components
    # between workgroups and nothing else: one band per triangle, no outside entries, no top operator, no carried prefix,
    # and a row's sum is its right-hand side and the inverse product over the component's local rows from k = 0 -- the
    # component's place in the slot order enters none of it.  Elsewhere the sums do change, and the oracle bar alone
    # holds: on shapes, leaves, forest and tuned a band with chained components no longer qualifies for the streamed
    # kernels, so host.hpp ls_reorder_own leaves its rows' own entries in CSR order instead of sources first (measured on
    # shapes: 9e-16 between the two handles); on blocks the workgroup count of a band also decides what the combined top
    # takes (HIFIR_AMD_TOP_WGS) and which bands carry a prefix (HIFIR_AMD_CD_FUSE_WGS), and the slot order of the sources
    # orders the coefficient tiles.
    V("band_wgs=1", W1, ("blocks", "ladder"), need=("band_ct1",), same_bits=("ladder",), also=("tuned",)),
    V("band_wgs=1-sparse", W1, ("leaves", "forest", "shapes"), need=("band_cd_sparse",), deny=("band_ls", "band_us"),
      need16=("band_cs_sparse",)),
    V("band_wgs=1-ct=0", _u(W1, {"CT": "0"}), ("blocks", "ladder"), need=("band_cd",), deny=CT_ANY, need16=("band_cs",),
      same_bits=("ladder",), ref={"CT": "0"}),
    V("band_wgs=1-ct_wide=0", _u(W1, {"CT_WIDE": "0"}), ("blocks", "ladder"), need=("band_ct2",), deny=("band_ct1", "band_ct4"),
      need16=("band_ct1",), same_bits=True, ref=W1),
    V("band_wgs=1-ct_wide4=0", _u(W1, {"CT_WIDE": "0", "CT_WIDE4": "0"}), ("blocks", "ladder"), need=("band_ct4",),
      deny=("band_ct1", "band_ct2"), need16=("band_ct1",), same_bits=True, ref=W1),
    V("tail0-band_wgs=1", _u(T0, W1), ("blocks",), lower=("band_ct1", "spmm_tile4_rb1")),
    V("tail0-band_wgs=1-leaves", _u(T0, W1), ("leaves",), need=("band_cd_sparse",), lower=("band_cd", "band_ct1")),
    V("band_wgs=1-fusions=0", _u(W1, NOFUSE), ("blocks", "leaves", "shapes"), need=("gather_scale", "scatter_scale"),
      deny=("scatter_scale_list", "band_ls", "band_us")),
    V("band_wgs=1-z", W1, ("blocksz", "ladderz"), need=("band_cd_z",), need16=("band_cs_z",)),
    V("band_wgs=1-z-sparse", W1, ("shapesz",), need=("band_cs_z",)),  # (sparse-own complex components run the slice kernel at every width)
    V("band_wgs=1-ct_z", _u(W1, {"CT_Z": "1"}), ("blocksz", "ladderz"), need=("band_ct_z",), deny=("band_cd_z",), need16=("band_ct_z",)),
    # -- execution
    V("twin=0", {"TWIN": "0"}, ("deep", "tuned", "blocks", "kkt", "blocksz"), same_bits=True),
    V("xcd=0", {"XCD": "0"}, ("deep", "tuned", "forest", "blocks", "leaves", "kkt", "blocksz"), same_bits=True),
    V("no_graph", {"NO_GRAPH": "1"}, ("deep", "tuned", "forest", "blocks", "leaves", "kkt", "blocksz"), same_bits=True),
    V("tail0-no_graph", _u(T0, {"NO_GRAPH": "1"}), ("deep", "blocks", "leaves"), same_bits=True, ref=T0),
]

# switches the engine reads that are no row of the table, and why
NOT_VARIANTS = {
    "CD_DBG": "development probe: switches phases of the band kernels off, the results are wrong on purpose",
    "PLAN_DUMP": "development probe: prints the band plan",
    "FINALIZE_DUMP": "development probe: prints finalize timings",
    "PROBE_OUT": "development probe (make PROBE=1 builds only)",
    "CSPROBE_OUT": "development probe (make CSPROBE=1 builds only)",
    "TAIL_PROBE_TOL": "guard of the tail operator: test_gpu_synthetic.py (ill-conditioned coarse level)",
    "TAIL_GROWTH": "guard of the tail operator: test_gpu_synthetic.py (rank-deficient / ill-conditioned tails)",
    "THREADS": "host threads of the analysis: no kernel depends on it (test_abi_and_host.py)",
    "LS": "test_gpu_ls_band.py: the same bits as every row in LDS, on three hierarchies",
    "LS_CHUNK": "test_gpu_ls_band.py: the same bits at every chunk size",
    "SKIP_ROWS": "test_gpu_ls_band.py: the row flags do not change a bit",
    "LOAD_ANALYSIS": "hifamd_load only: test_abi_and_host.py / test_gpu_parity.py save-load round trips",
    "DENSE_BLOCK": "BASE of every row; the exact mode (0) is test_gpu_parity.py's and smoke()'s subject",
    "MIN_LOGR": "BASE of every row (the arena is always 64 columns wide); narrower arenas: test_gpu_parity.py",
}


def switches_in_table():
    names = set(BASE)
    for v in VARIANTS:
        names |= set(v.env)
    return names


# ---- handles ----------------------------------------------------------------------------------------------------------
class _Env:
    """The environment a handle is created under: BASE + the row's switches, every other switch of the table unset."""

    def __init__(self, env):
        self.kw = {PFX + k: v for k, v in dict(BASE, **env).items()}

    def __enter__(self):
        names = {PFX + k for k in switches_in_table()} | set(self.kw)
        self.keep = {k: os.environ.get(k) for k in names}
        for k in names:
            os.environ.pop(k, None)
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _handle(h, env):
    """A handle is what its creation-time environment made it: every solve below runs after the environment is restored
    (the adjoint engine and the second lane are built on first use and must still follow the handle's switches)."""
    import hifir_amd

    with _Env(env):
        return hifir_amd.HIF.from_levels(h["levels"], max_nrhs=64, dtype=h["dtype"])


def _reference(h, env):
    """Bits and band count of the handle without the row's switch: once per (hierarchy, environment)."""
    key = ("ref", h["name"], tuple(sorted(env.items())))
    if key not in _cache:
        M = _handle(h, env)
        B64 = np.ascontiguousarray(h["B"][:, :64])
        _cache[key] = dict(X=M.solve_mrhs(B64), XT=M.solve_mrhs(B64, trans=True), stats=M.stats())
        M.close()
    return _cache[key]


def _colerr(X, Xo):
    """largest relative error of a column against the same column of the oracle"""
    return float(max(np.abs(X[:, c] - Xo[:, c]).max() / max(np.abs(Xo[:, c]).max(), 1e-300) for c in range(X.shape[1])))


def measure(v, hier):
    """Everything the five checks look at, as plain data (nothing is asserted here)."""
    h = _hier(hier)
    M = _handle(h, v.env)
    B = h["B"]
    r = dict(variant=v.name, hier=hier, stats=M.stats(), width_bits=[], replay_bits=[])
    r["bands"] = r["stats"]["bands"]
    # 1. against the oracle, width 100
    r["err"] = _colerr(M.solve_mrhs(B), h["Xo"])
    r["errT"] = _colerr(M.solve_mrhs(B, trans=True), h["XoT"])
    B64 = np.ascontiguousarray(B[:, :64])
    for tr in (False, True):
        X = M.solve_mrhs(B64, trans=tr)
        r["X64T" if tr else "X64"] = X
        r["census64T" if tr else "census64"] = M.kernel_census()
        r["lowerT" if tr else "lower"] = M.kernel_census(lower=True)
        # 2. width independence
        for k in WIDTHS:
            Xk = M.solve_mrhs(np.ascontiguousarray(B[:, :k]), trans=tr)
            if k == 16:
                r["census16T" if tr else "census16"] = M.kernel_census()
            if not np.array_equal(Xk, X[:, :k]):
                r["width_bits"].append((tr, k, _colerr(Xk, X[:, :k])))
        Xs = M.solve_mrhs(np.ascontiguousarray(B[:, 40:48]), trans=tr)
        if not np.array_equal(Xs, X[:, 40:48]):
            r["width_bits"].append((tr, "40:48", _colerr(Xs, X[:, 40:48])))
        # 3. replay and stale state
        M.solve_mrhs(np.full_like(B64, np.nan), trans=tr)
        X3 = M.solve_mrhs(B64, trans=tr)
        if not np.array_equal(X3, X):
            r["replay_bits"].append((tr, int(np.isnan(X3).sum()), _colerr(np.nan_to_num(X3), X)))
    M.close()
    return r


def _fmt(c):
    return " ".join(f"{k}={n}" for k, n in c.items() if n)


def judge(v, r):
    h = _hier(r["hier"])
    print(f"VARIANT {v.name} on {r['hier']}: relerr {r['err']:.2e} transposed {r['errT']:.2e} bands {r['bands']:.0f}")
    for k in ("census64", "census64T", "census16", "census16T", "lower"):
        print(f"  {k}: {_fmt(r[k])}")
    assert r["err"] <= TOL and r["errT"] <= TOL, (r["err"], r["errT"])
    assert not r["width_bits"], r["width_bits"]
    assert not r["replay_bits"], r["replay_bits"]
    reach = r["hier"] in v.on  # (an `also` hierarchy: the deny lists only)
    for c in ("census64", "census64T"):
        for f in v.need if reach else ():
            assert r[c][f] > 0, (c, f, "never launched")
        for f in v.deny:
            assert r[c][f] == 0, (c, f, r[c][f])
        for f, n in v.count64.items() if reach and c == "census64" else ():  # (the forward apply)
            assert r[c][f] == n, (c, f, r[c][f], n)
    for c in ("census16", "census16T"):
        for f in v.need16 if reach else ():
            assert r[c][f] > 0, (c, f, "never launched")
        for f in v.deny16:
            assert r[c][f] == 0, (c, f, r[c][f])
    for c in ("lower", "lowerT"):
        for f in v.lower if reach else ():
            assert r[c][f] > 0, (c, f, "never launched on a level >= 1")
    if v.same_bits or v.bands:
        ref = _reference(h, v.ref)
        if v.same_bits is True or (v.same_bits and r["hier"] in v.same_bits):
            assert np.array_equal(r["X64"], ref["X"]), _colerr(r["X64"], ref["X"])
            assert np.array_equal(r["X64T"], ref["XT"]), _colerr(r["X64T"], ref["XT"])
        if v.bands and reach:
            stat = v.bands if isinstance(v.bands, str) else "bands"
            assert r["stats"][stat] != ref["stats"][stat], (stat, r["stats"][stat])


CASES = [pytest.param(v, hier, id=f"{v.name}-{hier}",
                      marks=[pytest.mark.xfail(strict=True, reason=v.xfail)] if v.xfail else [])
         for v in VARIANTS for hier in v.on + v.also]


@pytest.mark.gpu
@pytest.mark.parametrize("v,hier", CASES)
def test_variant(v, hier):
    judge(v, measure(v, hier))


@pytest.mark.gpu
@pytest.mark.parametrize("v,hier", [pytest.param(v, hier, id=f"{v.name}-{hier}") for v in VARIANTS if v.env.get("BAND_WGS") == "1"
                                    for hier in v.on + v.also])
def test_band_wgs_rows_share_workgroups(v, hier):
    """No band_wgs=1 row is vacuous: the handle's plan has workgroups that own several components, and has none without
    the switch (hifamd_stats_ext slots 26 / 27)."""
    h = _hier(hier)
    for env, shared in ((v.env, True), ({k: x for k, x in v.env.items() if k != "BAND_WGS"}, False)):
        M = _handle(h, env)
        se = M.stats_ext()
        M.close()
        print(f"VARIANT {v.name} on {hier}, BAND_WGS={env.get('BAND_WGS')}: components {se['cd_components']:.0f} "
              f"cd_shared_workgroups {se['cd_shared_workgroups']:.0f}")
        assert se["cd_components"] > 0 and (se["cd_shared_workgroups"] > 0) == shared, se


# ---- the table guard (CPU) ----------------------------------------------------------------------------------------------
def test_every_switch_has_a_row():
    read = set()
    for f in ("engine.hip", "host.hpp", "options.hpp"):
        with open(os.path.join(ROOT, "hifir_amd", "csrc", f)) as fh:
            read |= set(re.findall(PFX + r"([A-Z0-9_]+)", fh.read()))
    table = switches_in_table()
    undecided = sorted(n for n in read if n not in table and n not in NOT_VARIANTS)
    assert not undecided, f"switches without a row in VARIANTS or a reason in NOT_VARIANTS: {undecided}"
    both = sorted(n for n in NOT_VARIANTS if n in table and n not in BASE)
    assert not both, both
    stale = sorted(n for n in (table | set(NOT_VARIANTS)) if n not in read)
    assert not stale, f"rows for switches the engine does not read: {stale}"
    with open(os.path.join(ROOT, "README.md")) as fh:
        readme = fh.read()
    para = readme[readme.index("Environment knobs"):]
    para = para[:para.index("\n\n")]
    missing = sorted(n for n in read if f"`{PFX}{n}`" not in para)
    assert not missing, f"switches the README's knob paragraph does not list: {missing}"
    names = [v.name for v in VARIANTS]
    assert len(names) == len(set(names))
