"""GPU (-m gpu): sparse-own L bands with streamed sources (kernel k_band_ls, host.hpp build_ls_plan) on the golden hierarchies
whose level 0 plans components of their own and on a synthetic hierarchy whose components exceed one chunk: against the
oracle, against the kernel that keeps every row in LDS (HIFIR_AMD_LS=0: the same per-row order, the same bits), at every
batch width, with and without the first solve's row flags, on graph replay, and transposed.

`shapes` (util.shapes_levels) gives the kernel every class of component it branches on -- test_shape_ladders_host.py asserts
on the CPU which: dependent rows 0 ... 65, sources 0 / 1 / 15 mod 16 and 64 / 65 / 128, a band of 129 ... 144 sources that
takes three chunks of 48, wave runs of 0 / 4 / 64 / 80 outside entries.  Its two bands and the two short forests at the end
launch all six instantiations k_band_ls<CW, NCH>: the handle's statistics say which (the chunk in rows = 16 CW, the most
chunks of one component; a launch takes NCH = max(2, chunks))."""
import os

import numpy as np
import pytest

import hifir_amd
from oracle import orc
from util import forest_levels, load_hier, relerr, shapes_levels, short_shapes_levels

pytestmark = pytest.mark.gpu

TOL = 1e-12
BASE_ENV = {"HIFIR_AMD_CD_SPARSE_MIN_ROWS": "0", "HIFIR_AMD_DENSE_BLOCK": "2048", "HIFIR_AMD_MIN_LOGR": "6"}
SWITCHES = ("HIFIR_AMD_LS", "HIFIR_AMD_SKIP_ROWS", "HIFIR_AMD_LS_CHUNK")


def _levels(name):
    if name == "shapes":
        return shapes_levels()
    return forest_levels() if name == "synthetic" else load_hier(name)[0]


# shapes: (rows of the largest chunk, most chunks of one component) per HIFIR_AMD_LS_CHUNK -- by default the first tier runs
# k_band_ls<4, 2> (128 sources at most) and the second <3, 3> (144 sources); at 48 both run <3, 3>; at 32 the first tier
# runs <2, 4> and the second, five chunks, keeps k_band_cd
SHAPES_CHUNKS = {"": (64.0, 3.0), "48": (48.0, 3.0), "32": (32.0, 4.0)}


class _Env:
    def __init__(self, **kw):
        self.kw = dict(BASE_ENV, **kw)

    def __enter__(self):
        self.keep = {k: os.environ.get(k) for k in list(self.kw) + list(SWITCHES)}
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _handle(levels, **env):
    with _Env(**env):
        return hifir_amd.HIF.from_levels(levels, max_nrhs=64)


@pytest.fixture(scope="module", params=["p2d_64_deep", "p2d_100_tuned", "synthetic", "shapes"])
def case(request):
    levels = _levels(request.param)
    n = int(levels[0]["n"])
    B = np.random.default_rng(21).uniform(-1, 1, size=(n, 64))
    M = _handle(levels)
    se = M.ls_stats()
    # the fixture does run through the kernel under test, with sources streamed and rows kept in LDS
    assert se["ls_chunk_rows"] in (32.0, 48.0, 64.0) and se["ls_streamed_sources"] > 0 and se["ls_lds_rows"] > 0, se
    print(request.param, "k_band_ls:", se)
    if request.param == "shapes":
        assert (se["ls_chunk_rows"], se["ls_max_chunks"]) == SHAPES_CHUNKS[""], se
    return dict(name=request.param, levels=levels, B=B, M=M, X=M.solve_mrhs(B), XT=M.solve_mrhs(B, trans=True))


def test_against_the_oracle(case):
    O = orc.Oracle(case["levels"])
    Xo = O.solve_batch(case["B"], threads=4)
    err = relerr(case["X"], Xo)
    print(case["name"], "relerr vs oracle", err)
    assert err <= TOL
    for c in range(3):  # transposed apply at the existing bar (test_gpu_synthetic._check)
        errt = relerr(case["XT"][:, c], O.solve(case["B"][:, c].copy(), trans=True))
        print(case["name"], "transposed column", c, errt)
        assert errt <= TOL * 10


def test_same_bits_as_every_row_in_lds(case):
    M0 = _handle(case["levels"], HIFIR_AMD_LS="0")
    se = M0.ls_stats()
    assert se["ls_chunk_rows"] == 0 and se["ls_streamed_sources"] == 0
    assert np.array_equal(M0.solve_mrhs(case["B"]), case["X"])
    assert np.array_equal(M0.solve_mrhs(case["B"], trans=True), case["XT"])


@pytest.mark.parametrize("chunk", ["32", "48"])
def test_same_bits_at_every_chunk_size(case, chunk):
    Mc = _handle(case["levels"], HIFIR_AMD_LS_CHUNK=chunk)
    se = Mc.ls_stats()
    print(case["name"], "LS_CHUNK", chunk, se)
    if case["name"] == "synthetic":  # (components of 120 sources: three chunks of 48, four of 32)
        assert (se["ls_chunk_rows"], se["ls_max_chunks"]) == (float(chunk), {"48": 3.0, "32": 4.0}[chunk]), se
    if case["name"] == "shapes":
        assert (se["ls_chunk_rows"], se["ls_max_chunks"]) == SHAPES_CHUNKS[chunk], se
    assert np.array_equal(Mc.solve_mrhs(case["B"]), case["X"])
    if case["name"] in ("synthetic", "shapes"):
        assert Mc.kernel_census()["band_ls"] > 0


def test_column_bits_do_not_depend_on_the_width(case):
    M, B = case["M"], case["B"]
    for tr, X in ((False, case["X"]), (True, case["XT"])):
        for k in (1, 8, 16, 48, 64):
            Xk = M.solve_mrhs(np.ascontiguousarray(B[:, :k]), trans=tr)
            assert np.array_equal(Xk, X[:, :k]), (tr, k, relerr(Xk, X[:, :k]))


def test_row_flags_do_not_change_a_bit(case):
    M, B = case["M"], case["B"]
    M1 = _handle(case["levels"], HIFIR_AMD_SKIP_ROWS="0")
    assert M1.stats_ext()["rows_not_stored_L"] == 0
    assert np.array_equal(M1.solve_mrhs(B), case["X"])
    assert np.array_equal(M1.solve_mrhs(B, trans=True), case["XT"])
    # non-finite values parked in the rows the first solve does not store: a batch of NaNs, then the batch again
    M.solve_mrhs(np.full_like(B, np.nan))
    assert np.array_equal(M.solve_mrhs(B), case["X"])
    M.solve_mrhs(np.full_like(B, np.inf), trans=True)
    assert np.array_equal(M.solve_mrhs(B, trans=True), case["XT"])


def test_graph_replay(case):
    M, B = case["M"], case["B"]
    for _ in range(3):  # (the batch shape's graph was captured by the fixture's first apply: these replay it)
        assert np.array_equal(M.solve_mrhs(B), case["X"])
        assert np.array_equal(M.solve_mrhs(B, trans=True), case["XT"])


@pytest.mark.parametrize("top,seed,want", [(96, 53, {"": (4, 2), "48": (3, 2), "32": (2, 3)}), (64, 54, {"": (4, 1), "48": (3, 2), "32": (2, 2)})])
def test_short_forests_run_the_other_instantiations(top, seed, want):
    """One band of components with at most 96 / 64 sources: <3, 2> and <2, 3> / <2, 2> (a band of one chunk runs NCH = 2)."""
    levels = short_shapes_levels(top, seed)
    n = int(levels[0]["n"])
    B = np.random.default_rng(22).uniform(-1, 1, size=(n, 64))
    Xo = orc.Oracle(levels).solve_batch(B, threads=4)
    M0 = _handle(levels, HIFIR_AMD_LS="0")
    X0 = M0.solve_mrhs(B)
    assert M0.kernel_census()["band_ls"] == 0
    for chunk, (cw, nch) in want.items():
        M = _handle(levels, **({"HIFIR_AMD_LS_CHUNK": chunk} if chunk else {}))
        se = M.ls_stats()
        X = M.solve_mrhs(B)
        err = relerr(X, Xo)
        print(f"{top} sources at most, LS_CHUNK={chunk or 'unset'}: k_band_ls<{cw}, {max(2, nch)}> {se} relerr {err:.2e}")
        assert (se["ls_chunk_rows"], se["ls_max_chunks"]) == (16.0 * cw, float(nch)), se
        assert M.kernel_census()["band_ls"] > 0
        assert err <= TOL
        assert np.array_equal(X, X0)
        assert np.array_equal(M.solve_mrhs(np.ascontiguousarray(B[:, :16])), X[:, :16])
