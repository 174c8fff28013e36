"""CPU: the shape ladders of util.py reach the classes the GPU tests claim to run (test_gpu_variants.py rows on `ladder`,
`shapes`, the band_wgs=1 rows; test_gpu_ls_band.py; test_gpu_wide_batch.py).  The host planner (tests/cpp/plan_model.cpp: the
engine's analyze_level, no GPU) is run on every hierarchy under the environment the GPU test uses, and its output must show

 * the dense ladder: one component band per triangle that holds every component size 9 ... 128 once (every count of 16-row
   strips, every remainder mod 16, every operand padding); every size 9 ... 96 under the complex handles' 96-row limit;
 * the shape forest: components that arrive intact in every class k_band_ls branches on -- dependent rows 0 / 1 / 15 / 16 /
   17 / 64 / 65, sources 0 / 1 / 15 mod 16, sources = C, C + 1, 2 C for the 64-row chunk, a band of its own with 129 ... 144
   sources (chunk 48, three chunks), longest wave runs of 0, 1 ... 63, exactly 64 and more than 64 outside entries;
 * shared workgroups: with HIFIR_AMD_BAND_WGS=1 every component band of every hierarchy the band_wgs=1 rows run on chains
   several components onto a workgroup, and none does without it.

These are conditions on the INPUTS: a planner change that moves a class away fails here, and is answered by choosing other
shapes, not by dropping the class."""
import json
import os
import subprocess

import numpy as np
import pytest

import hifir_amd
from test_gpu_variants import HIERS
from util import LADDER_SIZES, short_shapes_levels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PFX = "HIFIR_AMD_"


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """plan(name, **switches) -> the plan model's records of a hierarchy (saved once)"""
    tmp = tmp_path_factory.mktemp("plan_model")
    exe = str(tmp / "plan_model")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "hifir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "plan_model.cpp"), "-o", exe])
    files = {}

    def plan(name, **switches):
        if name not in files:
            levels = HIERS[name]() if name in HIERS else short_shapes_levels(*name)
            M = hifir_amd.HIF(dtype=np.float64)
            for lv in levels:
                M.add_level(lv)
            M.set_dense(levels[-1]["dense"])
            files[name] = str(tmp / f"{len(files)}.hifamd")
            M.save(files[name])
            M.close()
        env = {k: v for k, v in os.environ.items() if not k.startswith(PFX)}
        env[PFX + "DENSE_BLOCK"] = "2048"  # (BASE of test_gpu_variants.py)
        env.update({PFX + k: str(v) for k, v in switches.items()})
        out = subprocess.check_output([exe, files[name]], env=env).decode()
        return [json.loads(line) for line in out.splitlines()]

    return plan


def _cd_bands(records, tri=None):
    return [r for r in records if r.get("cd") == 1 and (tri is None or r["tri"] == tri)]


def test_dense_ladder_holds_every_size(model):
    for tri in "LU":
        bands = _cd_bands(model("ladder"), tri)
        assert len(bands) == 1 and bands[0]["sparse"] == 0, bands
        sizes = sorted(c[0] for c in bands[0]["comps"])
        print(f"ladder {tri}: {len(sizes)} dense-own components of {sizes[0]} ... {sizes[-1]} rows, each size once")
        assert sizes == list(LADDER_SIZES) == list(range(9, 129))
        # the complex handles' plan (96 rows per component)
        sizes96 = set(c[0] for b in _cd_bands(model("ladder", CD_ROWS=96), tri) if not b["sparse"] for c in b["comps"])
        print(f"ladder {tri}, 96-row components: sizes {min(sizes96)} ... {max(sizes96)}")
        assert set(range(9, 97)) <= sizes96 and max(sizes96) == 96


def _ls_components(records):
    """(chunk rows, chunks of the band, band, sources, dependent rows, longest wave run) of every component of a band k_band_ls takes"""
    return [(16 * b["ls_cw"], b["ls_nch"], b["band"], c[0] - s[0], s[0], s[1])
            for b in _cd_bands(records, "L") if b["sparse"] and b["ls"] for c, s in zip(b["comps"], b["streams"])]


def test_shape_forest_reaches_every_class(model):
    rec = model("shapes")
    assert all(b["sparse"] == 1 for b in _cd_bands(rec)) and len(_cd_bands(rec, "L")) == 2 and len(_cd_bands(rec, "U")) == 2
    comps = _ls_components(rec)
    nds = set(c[4] for c in comps)
    print("dependent rows:", sorted(nds))
    assert {0, 1, 15, 16, 17, 64, 65} <= nds
    rem = set(c[3] % 16 for c in comps if c[4] > 0)
    print("sources mod 16 (components with dependent rows):", sorted(rem))
    assert {0, 1, 15} <= rem
    ns64 = set(c[3] for c in comps if c[0] == 64 and c[4] > 0)
    print("sources of the components in 64-row-chunk bands:", sorted(ns64))
    assert {64, 65, 128} <= ns64 and max(ns64) == 128
    b48 = set(c[2] for c in comps if c[0] == 48 and c[1] == 3)
    assert len(b48) == 1 and not any(c[0] == 64 and c[2] in b48 for c in comps), b48
    ns48 = sorted(c[3] for c in comps if c[2] in b48)
    print("sources of the components of the 48-row-chunk band (three chunks):", ns48)
    assert 129 <= ns48[-1] <= 144
    runs = sorted(set(c[5] for c in comps))
    print("longest wave run per component (outside entries):", runs)
    assert 0 in runs and any(1 <= r <= 63 for r in runs) and 64 in runs and any(r >= 65 for r in runs)
    # the U bands (k_band_us): black rows and runs, for the record
    for b in _cd_bands(rec, "U"):
        print(f"U band {b['band']}: black rows {sorted(set(s[0] for s in b['streams']))}, longest run {max(s[1] for s in b['streams'])}")
    # under the chunk settings of test_gpu_ls_band.py: which instantiation every band takes
    for chunk, want in ((48, {(3, 3)}), (32, {(2, 4)})):
        got = set((b["ls_cw"], max(2, b["ls_nch"])) for b in _cd_bands(model("shapes", LS_CHUNK=chunk), "L") if b["ls"])
        print(f"LS_CHUNK={chunk}: k_band_ls<CW, NCH> =", sorted(got))
        assert got == want
    assert set((b["ls_cw"], max(2, b["ls_nch"])) for b in _cd_bands(rec, "L") if b["ls"]) == {(4, 2), (3, 3)}


@pytest.mark.parametrize("top,seed,want", [(96, 53, {0: (4, 2), 48: (3, 2), 32: (2, 3)}), (64, 54, {0: (4, 2), 48: (3, 2), 32: (2, 2)})])
def test_short_shape_forests_reach_the_other_chunk_counts(model, top, seed, want):
    for chunk, inst in want.items():
        bands = _cd_bands(model((top, seed), LS_CHUNK=chunk, CD_SPARSE_MIN_ROWS=0), "L")
        assert len(bands) == 1 and bands[0]["ls"] == 1, bands
        got = (bands[0]["ls_cw"], max(2, bands[0]["ls_nch"]))
        print(f"{top} sources at most, LS_CHUNK={chunk}: k_band_ls<{got[0]}, {got[1]}>, most sources", max(c[0] - s[0] for c, s in zip(bands[0]["comps"], bands[0]["streams"])))
        assert got == inst


@pytest.mark.parametrize("name", ["blocks", "leaves", "forest", "ladder", "shapes"])
def test_band_wgs_1_shares_workgroups(model, name):
    one = _cd_bands(model(name))
    assert one and all(max(b["wg_comps"]) == 1 for b in one), [(b["tri"], b["band"], max(b["wg_comps"])) for b in one]
    shared = _cd_bands(model(name, BAND_WGS=1))
    print(name, "components per workgroup under BAND_WGS=1:", [(b["level"], b["tri"], b["band"], max(b["wg_comps"])) for b in shared])
    assert shared and all(max(b["wg_comps"]) > 1 for b in shared)
