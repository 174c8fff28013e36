"""CPU: the small-matrix arithmetic of the block CG driver (hifir_amd/csrc/blockcg_small.hpp, what k_bcg_small runs in one
workgroup) as a plain C++ program under the address and undefined sanitizers: tests/cpp/blockcg_small_test.cpp sums,
factors and inverts the Grams written here, and its pivots, ranks, factors and verdicts are held to numpy's
(blockcg_util.pchol).  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

from blockcg_util import DEFTOL, _herm, pchol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gram(rng, n, m, rank=None, cplx=False):
    X = rng.uniform(-1, 1, (n, m)) + (1j * rng.uniform(-1, 1, (n, m)) if cplx else 0)
    if rank is not None and rank < m:
        X[:, rank:] = X[:, :rank] @ (rng.integers(-2, 3, (rank, m - rank)) / 2.0)
    X = X / np.linalg.norm(X, axis=0)
    return X.conj().T @ X


def _cases():
    """name -> (partials [nb][m][m], deftol, pivoted, expectation: dict of what must hold besides agreement with numpy)"""
    rng = np.random.default_rng(61)
    out = {}
    out["rank0"] = (np.zeros((1, 8, 8)), DEFTOL, True, dict(r=0, bad=False))
    v = rng.uniform(-1, 1, 8)
    out["rank1"] = (np.outer(v, v)[None], DEFTOL, True, dict(r=1, bad=False, piv=[int(np.argmax(v * v))]))
    out["rank5of8"] = (_gram(rng, 40, 8, rank=5)[None], DEFTOL, True, dict(r=5, bad=False))
    G = _gram(rng, 200, 64)
    P = rng.uniform(-1, 1, (3, 64, 64))
    P[2] = G - P[0] - P[1]  # three partials that sum to G up to rounding
    out["full64"] = (P, DEFTOL, True, dict(r=64, bad=False))
    out["ties"] = (np.array([[[2.0, 1, 1], [1, 2, 1], [1, 1, 2]]]), DEFTOL, True, dict(r=3, bad=False, piv=[0, 1, 2]))
    out["ties_diag"] = (np.diag([1.0, 3, 3, 1, 3])[None], DEFTOL, True, dict(r=5, bad=False, piv=[1, 2, 4, 0, 3]))
    out["left_m1e-20"] = (np.diag([1.0, -1e-20, 0.5])[None], DEFTOL, True, dict(r=2, bad=False, piv=[0, 2], dropped=-1e-20))
    out["left_m1e-3"] = (np.diag([1.0, -1e-3, 0.5])[None], DEFTOL, True, dict(r=2, bad=True))
    G = _gram(rng, 30, 6)
    G[2, 4] = G[4, 2] = np.nan
    out["nan"] = (G[None], DEFTOL, True, dict(r=0, bad=True))
    out["nan_unpivoted"] = (G[None], DEFTOL, False, dict(r=0, bad=True))
    out["indefinite"] = (np.array([[[1.0, 2], [2, 1]]]), DEFTOL, False, dict(r=1, bad=True))
    out["negative"] = (-_gram(rng, 30, 6)[None], DEFTOL, False, dict(r=0, bad=True))
    out["spd_unpivoted"] = (_gram(rng, 90, 33)[None], DEFTOL, False, dict(r=33, bad=False, piv=list(range(33))))
    out["z_rank3of5"] = (_gram(rng, 30, 5, rank=3, cplx=True)[None], DEFTOL, True, dict(r=3, bad=False))
    out["z_spd_unpivoted"] = (_gram(rng, 50, 17, cplx=True)[None], DEFTOL, False, dict(r=17, bad=False))
    out["loose_deftol"] = (np.diag([1.0, 1e-3, 1e-5])[None], 1e-4, True, dict(r=2, bad=False, piv=[0, 1]))
    return out


def _fmt(v):
    return "%s %s" % (repr(float(np.real(v))), repr(float(np.imag(v))))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bcg") / "blockcg_small_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "hifir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "blockcg_small_test.cpp"), "-o", exe])
    return exe


def test_small_matrix_program(program, tmp_path):
    cases = _cases()
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for name, (P, deftol, pivoted, _) in cases.items():
            f.write("%s %d %r %d %d %d\n" % (name, P.shape[1], deftol, int(pivoted), int(np.iscomplexobj(P)), P.shape[0]))
            f.write(" ".join(_fmt(v) for v in P.ravel()) + "\n")
    out = subprocess.check_output([program, path]).decode()
    lines = [ln for ln in out.splitlines() if ln.startswith("case ")]
    assert out.strip().endswith("cases %d OK" % len(cases)) and len(lines) == len(cases), out
    for ln, (name, (P, deftol, pivoted, want)) in zip(lines, cases.items()):
        head, piv, S, errs = (part.split() for part in ln.split("|"))
        assert head[1] == name
        r, bad, kept, dropped = int(head[2]), bool(int(head[3])), float(head[4]), float(head[5])
        piv = [int(p) for p in piv]
        m = P.shape[1]
        G = P[0].copy()
        for b in range(1, P.shape[0]):
            G = G + P[b]
        G = _herm(G)
        Sn, pn, rn, bn, kn, dn = pchol(G, deftol, pivoted)
        assert (r, bad) == (rn, bn) == (want["r"], want["bad"]), (name, r, bad, rn, bn)
        assert piv == [int(p) for p in pn] and piv == want.get("piv", piv), (name, piv, pn)
        if bad:
            continue
        if r:
            assert abs(kept - kn) <= 1e-12 * kn, name
        assert abs(dropped - dn) <= 1e-14, (name, dropped, dn)
        if "dropped" in want:
            assert dropped == want["dropped"], (name, dropped)
        vals = np.array([float(v) for v in S]).reshape(r, m, 2)
        Sc = vals[..., 0] + 1j * vals[..., 1]
        assert np.abs(Sc - Sn).max(initial=0.0) <= 1e-12, name
        # reconstruction on the pivot rows and columns, by numpy and by the program; inverse, selection, quadratic forms
        if r:
            assert np.abs(G[np.ix_(piv, piv)] - (Sc.conj().T @ Sc)[np.ix_(piv, piv)]).max() <= 1e-13, name
            # (inverse: the bound scales with the condition of S[:, piv], 1 / sqrt(smallest kept pivot) at the worst)
            rec, inv, sel, quad = (float(v) for v in errs)
            assert rec <= 1e-13 and max(inv, sel, quad) <= 1e-12 / kept, (name, rec, inv, sel, quad)
