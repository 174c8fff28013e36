"""CPU: the oracle's product agrees with the oracle's solve on every hierarchy of test_gpu_product.py's table.

The restatement of prec_prod / prec_prod_tran is pinned to the real reference on the golden fixtures only
(test_oracle_golden.py::test_mmultiply_and_roundtrip); the product table leans on it for synthetic hierarchies it was never
run on.  With rank = -1 the product is the exact inverse of the solve, so M (M^{-1} b) = b and M^{-1} (M b) = b, forwards and
conjugate-transposed, to the project's round-trip bar of 1e-10 relative to max|b| (measured: 1.7e-13 on `herm`, a few 1e-14
on the synthetic hierarchies -- the reference alone stays far inside the bar).

One pair is no identity in the reference itself: a COMPLEX hierarchy whose last level is LUP (`younglup`).  Its transposed
solve runs ?getrs 'T' on the block (LUP.hpp:150: the plain transpose) while its transposed product multiplies by the block's
conjugate transpose (LUP.hpp:187: 'C'), and the oracle restates both literally (orc.lup: op 2 / op 3).  The two are inverses
of one another only for real data: measured 3.8 relative on `younglup`.  There the transposed product is tied to the forward
product instead, which the forward round trip has just tied to the solve: y^H (M x) = (M^H y)^H x.  That identity is asserted
on every hierarchy; each side is a sum of n products of numbers the 1e-10 bar already covers, so it gets the same bar relative
to the sum of the absolute products."""
import numpy as np
import pytest

import test_gpu_product as tp
from oracle import orc
from util import rand_rhs

BAR = 1e-10


@pytest.mark.parametrize("name", tp.HIER_NAMES)
def test_product_inverts_solve(name):
    levels, dtype = tp._levels(name)
    O = orc.Oracle(levels, dtype=dtype)
    B = rand_rhs(np.random.default_rng(47), (int(levels[0]["n"]), 2), dtype)
    tran_lup_z = np.dtype(dtype).kind == "c" and int(levels[-1].get("dense_lup", 0)) == 1  # (module docstring)
    for tr in (False, True):
        for c in range(2):
            b = np.ascontiguousarray(B[:, c])
            e1 = np.abs(O.mmultiply(O.solve(b, rank=-1, trans=tr), rank=-1, trans=tr) - b).max() / np.abs(b).max()
            e2 = np.abs(O.solve(O.mmultiply(b, rank=-1, trans=tr), rank=-1, trans=tr) - b).max() / np.abs(b).max()
            print(f"{name} {'transposed ' if tr else ''}column {c}: M M^-1 b {e1:.2e}  M^-1 M b {e2:.2e}")
            if tr and tran_lup_z:
                assert min(e1, e2) > 1e-3, "the reference's 'T' solve and 'C' product of a complex LUP block became inverses?"
            else:
                assert e1 <= BAR and e2 <= BAR, (tr, c, e1, e2)
    x, y = np.ascontiguousarray(B[:, 0]), np.ascontiguousarray(B[:, 1])
    Mx, MHy = O.mmultiply(x, rank=-1), O.mmultiply(y, rank=-1, trans=True)
    ea = abs(np.vdot(y, Mx) - np.vdot(MHy, x)) / (np.abs(y) @ np.abs(Mx))
    print(f"{name} adjoint identity: {ea:.2e}")
    assert ea <= BAR
    O.close()
