"""CPU: the fixture of test_gpu_ct_ahead.py (ct_ahead_util.py) reaches the strip lengths it claims.  The host planner
(tests/cpp/plan_model.cpp: the engine's analyze_level and build_ct_tiles, no GPU) is run on the saved hierarchy, as
test_shape_ladders_host.py runs it, and its records must show

 * the tier-2 components as ONE tile band of L, each component with the rows it was given and the tile count that was
   prescribed for it -- for a single-strip component that is the tile count of its strip;
 * every tile count of {0, 1, BU - 1, BU, BU + 1, 2 BU - 1, 2 BU, 2 BU + 1, 3 BU + 2}, BU = 8, 4, 2, as the length of a
   single strip of 16 rows and of one of 9 rows (T = 0: a component of the first band; inside the tile band the empty
   strips are the middle ones of the three-strip components);
 * the same components under HIFIR_AMD_BAND_WGS=1 (with TOP_ROWS=0: a band of eight workgroups would otherwise be taken
   into the level's top operator), several of them chained on one workgroup.

These are conditions on the INPUT: a planner change that moves a class away fails here, and is answered by other shapes."""
import json
import os
import subprocess

import numpy as np
import pytest

import hifir_amd
from ct_ahead_util import BATCH_SIZES, COMPONENTS, REPEATS, TILE_COUNTS, ct_ahead_levels, edge_tile_counts, sources_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PFX = "HIFIR_AMD_"


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """plan(**switches) -> the plan model's records of the fixture (saved once)"""
    tmp = tmp_path_factory.mktemp("ct_ahead_plan")
    exe = str(tmp / "plan_model")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "hifir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "plan_model.cpp"), "-o", exe])
    levels, comps = ct_ahead_levels()
    M = hifir_amd.HIF(dtype=np.float64)
    for lv in levels:
        M.add_level(lv)
    M.set_dense(levels[-1]["dense"])
    path = str(tmp / "ct_ahead.hifamd")
    M.save(path)
    M.close()

    def plan(**switches):
        env = {k: v for k, v in os.environ.items() if not k.startswith(PFX)}
        env[PFX + "DENSE_BLOCK"] = "2048"  # (BASE of test_gpu_variants.py)
        env.update({PFX + k: str(v) for k, v in switches.items()})
        out = subprocess.check_output([exe, path], env=env).decode()
        return [json.loads(line) for line in out.splitlines()]

    return plan, levels, comps


def test_tile_counts_are_the_batch_edges():
    assert list(TILE_COUNTS) == edge_tile_counts() == [0, 1, 2, 3, 4, 5, 7, 8, 9, 14, 15, 16, 17, 26]
    assert BATCH_SIZES == (8, 4, 2)
    for t in TILE_COUNTS:
        assert (sources_of(t) + 3) // 4 == t
    assert sum(sources_of(t) % 4 != 0 for t in TILE_COUNTS) >= 9  # (a partly empty last tile)
    assert {len(ts) for _, ts in COMPONENTS} == {1, 3, 8}
    assert all(ts[1] == 0 and ts[0] > 0 and ts[2] > 0 for _, ts in COMPONENTS if len(ts) == 3)
    assert all(len(set(ts)) >= 7 for n, ts in COMPONENTS if n == 128)


def _tile_bands(records, tri):
    return [r for r in records if r.get("tri") == tri and r.get("cd") == 1 and r.get("ct_tiles", 0) > 0]


@pytest.mark.parametrize("switches", [{}, {"BAND_WGS": 1, "TOP_ROWS": 0}], ids=["default", "band_wgs=1"])
def test_planner_keeps_the_prescribed_strips(model, switches):
    plan, levels, comps = model
    assert int(levels[0]["n"]) <= 6000 and len(comps) == REPEATS * len(COMPONENTS)
    rec = plan(**switches)
    bands = _tile_bands(rec, "L")
    assert len(bands) == 1 and bands[0]["sparse"] == 0, [{k: v for k, v in b.items() if k != "comps"} for b in bands]
    band = bands[0]
    # [rows, walked entries, distinct sources, tiles of 16-row strips, ...] per component against (rows, tiles) as laid out
    got = sorted((c[0], c[3]) for c in band["comps"])
    want = sorted((n, sum(ts)) for _, n, ts in comps if sum(ts) > 0)
    print(f"L tile band: {len(got)} components, {band['ct_tiles']} tiles, longest wave chain {band['ct_wave_max']}")
    assert got == want
    assert band["ct_tiles"] == sum(t for _, t in want)
    assert not any(r.get("top_band") for r in rec if r.get("tri"))  # (no band was taken into a top operator)
    # the components without an entry into tier 1 are components of the first band, whole
    first = [r for r in rec if r.get("tri") == "L" and r.get("cd") == 1 and r.get("ct_tiles", 0) == 0]
    assert len(first) == 1
    sizes0 = sorted(c[0] for c in first[0]["comps"])
    assert sizes0.count(16) == REPEATS and sizes0.count(9) == REPEATS and sizes0.count(128) == len(sizes0) - 2 * REPEATS
    # every tile count is the length of ONE strip: a 16-row and a 9-row single-strip component each
    for rows in (16, 9):
        single = sorted(set(t for n, t in got if n == rows))
        print(f"single-strip components of {rows} rows: tiles {single}")
        assert single == [t for t in TILE_COUNTS if t > 0]
    shared = max(band["wg_comps"])
    print("components per workgroup:", shared)
    assert (shared > 1) == ("BAND_WGS" in switches)
    # U (the transposed pattern): the tier-1 clusters read tier 2 -- a tile band of 128-row components, for the record
    ub = _tile_bands(rec, "U")
    assert len(ub) == 1
    print(f"U tile band: {len(ub[0]['comps'])} components, tiles per component {sorted(c[3] for c in ub[0]['comps'])}, "
          f"longest wave chain {ub[0]['ct_wave_max']}")
    assert all(c[0] == 128 and c[3] >= 8 * 8 for c in ub[0]["comps"] if c[3] > 0)  # (eight strips, more than a batch each on average)
