"""GPU (-m gpu): sparse-own L bands with streamed sources (kernel k_band_ls, host.hpp build_ls_plan) on the golden hierarchies
whose level 0 plans components of their own and on a synthetic hierarchy whose components exceed one chunk: against the
oracle, against the kernel that keeps every row in LDS (HIFIR_AMD_LS=0: the same per-row order, the same bits), at every
batch width, with and without the first solve's row flags, on graph replay, and transposed."""
import os

import numpy as np
import pytest

import hifir_amd
from oracle import orc
from util import forest_levels, load_hier, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-12
BASE_ENV = {"HIFIR_AMD_CD_SPARSE_MIN_ROWS": "0", "HIFIR_AMD_DENSE_BLOCK": "2048", "HIFIR_AMD_MIN_LOGR": "6"}
SWITCHES = ("HIFIR_AMD_LS", "HIFIR_AMD_SKIP_ROWS", "HIFIR_AMD_LS_CHUNK")


def _levels(name):
    return forest_levels() if name == "synthetic" else load_hier(name)[0]


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


@pytest.fixture(scope="module", params=["p2d_64_deep", "p2d_100_tuned", "synthetic"])
def case(request):
    levels = _levels(request.param)
    n = int(levels[0]["n"])
    B = np.random.default_rng(21).uniform(-1, 1, size=(n, 64))
    M = _handle(levels)
    se = M.ls_stats()
    # the fixture does run through the kernel under test, with sources streamed and rows kept in LDS
    assert se["ls_chunk_rows"] in (32.0, 48.0, 64.0) and se["ls_streamed_sources"] > 0 and se["ls_lds_rows"] > 0, se
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
    assert np.array_equal(Mc.solve_mrhs(case["B"]), case["X"])


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
