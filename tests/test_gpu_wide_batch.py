"""GPU (-m gpu): batches wider than one 64-column tile, against the oracle and against their own tiles.

An apply of more than 64 columns is cut into 64-column tiles; tile t runs on lane t % 2 (the engine and its twin, each with
an arena and a captured graph of its own), so from 129 columns on a lane's graph holds several tiles back to back on one
arena (enqueue_apply with a tile stride of 2, the column offset added to the slot pointers, one census per lane summed over
its tiles).  The README's headline figures are for 128 and 256 columns; before this file no test checked a column beyond
the hundredth.  Per hierarchy and width (65, 127, 128, 129, 192, 256, 257), forwards and conjugate-transposed:

 1. every column within 1e-12 of the oracle (TOL of test_gpu_parity.py / test_gpu_variants.py);
 2. tile k of the wide result has the bits of columns 64 k ... solved as a batch of their own (the project's claim that a
    column's bits do not depend on the batch it travels in, for wide batches);
 3. the launch census of the wide apply is the sum of the censuses of its tiles solved alone;
 4. HIFIR_AMD_TWIN=0 (every tile on one lane, up to five back to back) gives the bits of 2., and so does the device entry
    point with row strides larger than the width;
 5. wide apply, an all-NaN batch of the same shape, the wide apply again: the bits of the first.

Hierarchies: p2d_100_tuned (sparse-own components, three levels), blocks (dense-own components, tiled Schur products, top
operator), kkt_26 (complex) and ladder (every dense-own component size); one oracle batch of 257 columns each, cached."""
import numpy as np
import pytest

from test_gpu_variants import HIERS, TOL, _colerr, _handle
from util import rand_rhs

pytestmark = pytest.mark.gpu

WIDE = (65, 127, 128, 129, 192, 256, 257)
NAMES = ("tuned", "blocks", "kkt", "ladder")
_cache = {}


def _wide(name):
    """levels, the 257-column batch, the oracle's two answers and the two handles: once per hierarchy, never written to."""
    if name not in _cache:
        from oracle import orc

        levels = HIERS[name]()
        z = any(np.iscomplexobj(lv["L_vals"]) or np.iscomplexobj(lv["d"]) for lv in levels)
        dtype = np.complex128 if z else np.float64
        B = rand_rhs(np.random.default_rng(43), (int(levels[0]["n"]), max(WIDE)), dtype)
        O = orc.Oracle(levels, dtype=dtype)
        h = dict(name=name, levels=levels, dtype=dtype, B=B, Xo=O.solve_batch(B, threads=4), XoT=O.solve_batch(B, threads=4, trans=True))
        for a in (h["B"], h["Xo"], h["XoT"]):
            a.setflags(write=False)
        h["M"], h["M1"] = _handle(h, {}), _handle(h, {"TWIN": "0"})
        _cache[name] = h
    return _cache[name]


def _add(total, census):
    for k, n in census.items():
        total[k] = total.get(k, 0) + n
    return total


@pytest.mark.parametrize("width", WIDE)
@pytest.mark.parametrize("name", NAMES)
def test_wide_batch(name, width):
    import torch

    h = _wide(name)
    M, M1 = h["M"], h["M1"]
    B = h["B"][:, :width].copy()
    for tr in (False, True):
        X = M.solve_mrhs(B, trans=tr)
        wide = M.kernel_census()
        err = _colerr(X, (h["XoT"] if tr else h["Xo"])[:, :width])
        print(f"WIDE {name} width {width}{' transposed' if tr else ''}: relerr {err:.2e}, launches {sum(wide.values())}")
        assert err <= TOL, err  # 1.
        tiles = {}
        for c0 in range(0, width, 64):
            Xk = M.solve_mrhs(np.ascontiguousarray(B[:, c0:c0 + 64]), trans=tr)
            _add(tiles, M.kernel_census())
            assert np.array_equal(Xk, X[:, c0:c0 + 64]), (tr, c0, _colerr(Xk, X[:, c0:c0 + 64]))  # 2.
        assert wide == tiles, {k: (wide[k], tiles[k]) for k in wide if wide[k] != tiles[k]}  # 3.
        # 4. one lane; the device entry point with padded rows (ldb = width + 5, ldx = width + 3)
        X1 = M1.solve_mrhs(B, trans=tr)
        assert np.array_equal(X1, X), (tr, "TWIN=0", _colerr(X1, X))
        assert M1.kernel_census() == wide
        Bd = torch.full((B.shape[0], width + 5), float("nan"), dtype=torch.from_numpy(B).dtype, device="cuda")
        Bd[:, :width] = torch.from_numpy(B).cuda()
        Xd = torch.full((B.shape[0], width + 3), 7.0, dtype=Bd.dtype, device="cuda")
        torch.cuda.synchronize()  # (torch fills the blocks on ITS stream; the handle's stream knows nothing of it)
        M.solve_mrhs(Bd[:, :width], Xd[:, :width], trans=tr)
        M.sync()
        torch.cuda.synchronize()
        Xh = Xd.cpu().numpy()
        assert np.array_equal(Xh[:, :width], X), (tr, "device pointers", _colerr(Xh[:, :width], X))
        assert np.all(Xh[:, width:] == 7.0)  # (nothing is written beyond the batch's columns)
        # 5. replay and stale state
        M.solve_mrhs(np.full_like(B, np.nan), trans=tr)
        X3 = M.solve_mrhs(B, trans=tr)
        assert np.array_equal(X3, X), (tr, "replay", int(np.isnan(X3).sum()))
