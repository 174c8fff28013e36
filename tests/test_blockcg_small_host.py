"""CPU: the small-matrix arithmetic and the decisions of the block CG driver (hifir_amd/csrc/blockcg_small.hpp, what k_bcg_beta
and k_bcg_small run in one workgroup) as plain C++ programs under the address and undefined sanitizers.
tests/cpp/blockcg_small_test.cpp sums, factors and inverts the Grams written here, and its pivots, ranks, factors and verdicts
are held to numpy's (blockcg_util.pchol).  A numpy model of bcg::start_columns and the four modes (Model) drives whole tiles
the way Engine::bcg_tile does -- it agrees with blockcg_util.bcg_restated -- and records every mode's input;
tests/cpp/blockcg_tile_test.cpp replays the inputs with a team of one on its own state, and what it prints after every mode
(control words, ranks, flags, iterations, residual ratios, E1, E2, C) is held to the model's.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import scipy.sparse as sp

import blockcg_util as U
from blockcg_util import DEFTOL, _herm, _select, _tri_inv, pchol
from lockstep_edges_util import MARGIN

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


def _build(tmp_path_factory, name):
    exe = str(tmp_path_factory.mktemp("bcg") / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "hifir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory, "blockcg_small_test")


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


# ---- the decisions: whole tiles, mode by mode ------------------------------------------------------------------------------
def _quad_forms(H, C):
    """sqrt(max(0, c_j^H H c_j)) for the columns of C with the sums in bcg::quad_forms' own order (H C with l ascending, then
    the rows ascending; complex products written out).  Where a column's residual has left the block's space the form is
    what cancellation leaves of terms near 1, and its square root moves by several per cent with the order of the sums:
    only the same order reproduces it."""
    Hr, Hi, Cr, Ci = np.real(H), np.imag(H), np.real(C), np.imag(C)
    ar, ai = np.zeros(C.shape), np.zeros(C.shape)
    with np.errstate(all="ignore"):
        for l in range(C.shape[0]):
            hr, hi, cr, ci = Hr[:, l:l + 1], Hi[:, l:l + 1], Cr[l:l + 1, :], Ci[l:l + 1, :]
            ar, ai = ar + (hr * cr - hi * ci), ai + (hr * ci + hi * cr)
        tot = np.zeros(C.shape[1])
        for i in range(C.shape[0]):
            tot = tot + (Cr[i] * ar[i] + Ci[i] * ai[i])
        return np.sqrt(np.where(tot > 0.0, tot, 0.0))


class Model:
    """the state of a tile of s columns, bcg::start_columns and the four modes of blockcg_small.hpp; ops collects
    (kind, k, values, snapshot)"""

    def __init__(self, s, rtol, deftol, maxit, dtype):
        self.s, self.rtol, self.deftol, self.maxit = s, rtol, deftol, maxit
        self.C, self.E1, self.E2 = (np.zeros((s, s), dtype) for _ in range(3))
        self.ctl = [0, 0, 0, 0]
        self.ops = []

    def _snap(self, kind, k, values):
        self.ops.append((kind, k, np.array(values), dict(
            ctl=list(self.ctl), flag=self.flag.copy(), iter=self.iter.copy(), active=self.active.copy(), bnorm=self.bnorm.copy(),
            relres=self.relres.copy(), E1=self.E1.copy(), E2=self.E2.copy(), C=self.C.copy())))

    def _end(self, miss, done):
        self.flag[self.active] = np.where(self.relres[self.active] <= self.rtol, 0, miss)
        self.iter[self.active] = done
        self.ctl[0] = 0

    def _pad(self, M):
        out = np.zeros_like(self.C)
        out[:M.shape[0], :M.shape[1]] = M
        return out

    def start_columns(self, b2):
        b2 = np.asarray(b2, float)
        self.active = (b2 != 0) & np.isfinite(b2)
        self.bnorm = np.where(self.active, np.sqrt(np.where(self.active, b2, 1.0)), 0.0)
        self.flag = np.where((b2 == 0) | self.active, 0, 1)
        self.iter = np.zeros(self.s, int)
        self.relres = np.full(self.s, np.inf)
        self.ctl = [1, 0, 0, self.s]
        self._snap(0, 0, b2)

    def start(self, G):
        if self.ctl[0]:
            self.E1[:], self.E2[:] = 0, 0
            S, piv, r, bad, _, _ = pchol(_herm(G.copy()), self.deftol)
            if bad:
                self._end(1, 0)
            elif r == 0:
                self.ctl[0] = 0  # every column zero or excluded: the flags stay
            else:
                self.E1, self.C = self._pad(_select(S, piv, self.s)), self._pad(S)
                self.ctl[1:] = [r, r, r]
        self._snap(1, 0, G)

    def alpha(self, k, G):
        if self.ctl[0]:
            r = self.ctl[3]
            self.E1[:], self.E2[:] = 0, 0
            Uf, _, _, bad, _, _ = pchol(_herm(G[:r, :r].copy()), self.deftol, pivoted=False)
            if bad:
                self._end(1, k - 1)
            else:
                Ti = _tri_inv(Uf)
                al = Ti @ Ti.conj().T
                self.E2 = self._pad(al)
                self.E1 = self._pad((al @ self.C[:r, :]) * np.where(self.active, self.bnorm, 0.0)[None, :])
                self.ctl[2] = r
        self._snap(2, k, G)

    def test(self, k, G):
        if self.ctl[0]:
            r = self.ctl[3]
            H = _herm(G[:r, :r].copy())
            self.relres = _quad_forms(H, self.C[:r, :])
            if (self.relres[self.active] <= self.rtol).all() or k >= self.maxit:
                self._end(2, k)
        self._snap(3, k, G)

    def next(self, k, G):
        if self.ctl[0]:
            r = self.ctl[3]
            self.E1[:], self.E2[:] = 0, 0
            S, piv, r1, bad, _, _ = pchol(_herm(G[:r, :r].copy()), self.deftol)
            if bad or r1 == 0:
                self._end(1, k)
            else:
                self.E1, self.E2, self.C = self._pad(_select(S, piv, r)), self._pad(S.conj().T), self._pad(S @ self.C[:r, :])
                self.ctl[3] = r1
        self._snap(4, k, G)


def _run(A, B, minv, rtol, maxit, deftol=DEFTOL):
    """a whole batch as ONE tile in the launch order of Engine::bcg_tile, M^{-1} = diag(minv) -> (X, flags, iters, ranks, model)"""
    n, s = B.shape
    M = Model(s, rtol, deftol, maxit, B.dtype)
    with np.errstate(all="ignore"):
        M.start_columns([np.vdot(B[:, j], B[:, j]).real for j in range(s)])
    X, P = np.zeros_like(B), np.zeros_like(B)
    Q = np.where(M.active[None, :], B / np.where(M.active, M.bnorm, 1.0)[None, :], 0)
    W = minv[:, None] * Q
    M.start(Q.conj().T @ W)
    Q, P = Q @ M.E1, W @ M.E1 + P @ M.E2
    for k in range(1, maxit + 1):
        if M.ctl[0] == 0:
            break
        Tm = A @ P
        M.alpha(k, P.conj().T @ Tm)
        X, Q = X + P @ M.E1, Q - Tm @ M.E2
        M.test(k, Q.conj().T @ Q)
        if M.ctl[0] == 0:
            break
        W = minv[:, None] * Q
        M.next(k, Q.conj().T @ W)
        Q, P = Q @ M.E1, W @ M.E1 + P @ M.E2
    return X, M.flag, M.iter, [M.ctl[1], M.ctl[2]], M


def _spd(n, s, seed, lo=1.0, hi=10.0, cplx=False):
    rng = np.random.default_rng(seed)
    A = np.diag(rng.uniform(lo, hi, n))
    B = rng.uniform(-1, 1, (n, s))
    if cplx:
        H = rng.uniform(-1, 1, (n, n)) + 1j * rng.uniform(-1, 1, (n, n))
        A = A + 0.05 * (H + H.conj().T)
        B = B + 1j * rng.uniform(-1, 1, (n, s))
    return A, B


def _tiles():
    """name -> (A, B, minv, rtol, maxit, expected flags): the smallest inputs that take each branch"""
    out = {}
    _, A, B = U.tiny_case()
    out["tiny"] = (A, B, np.ones(3), U.RTOL, U.MAXIT, [0] * 5)  # n = 3 < 5 columns
    _, A, B = U.rank_loss_case()
    out["rank_loss"] = (A, B, np.ones(B.shape[0]), U.RTOL, U.MAXIT, [0] * 5)  # loses two directions in step 1
    rng = np.random.default_rng(5)
    A, _ = _spd(40, 8, 5)
    minv = 1.0 / rng.uniform(1, 3, 40)
    # rank 5 of 8, a diagonal M^{-1}  (seed: one whose dependent column leaves a pivot below decisions_ok's 1e-16)
    out["deflation"] = (A, U.deflation_batch(40, seed=53), minv, U.RTOL, U.MAXIT, [0] * 8)
    A, B = _spd(12, 4, 6)
    B[:, 1] = 0.0
    B[3, 2] = np.nan
    out["nan_and_zero"] = (A, B, np.ones(12), U.RTOL, U.MAXIT, [0, 0, 1, 0])
    A, B = _spd(5, 3, 7)
    out["all_zero"] = (A, np.zeros_like(B), np.ones(5), U.RTOL, U.MAXIT, [0] * 3)  # mode 1 with r == 0: the flags stay
    A, B = _spd(30, 3, 8)
    B[:, 0] = 0.0
    B[0, 0] = 1.0  # an eigenvector: converged after one step, whatever the others do
    out["maxit1"] = (A, B, np.ones(30), U.RTOL, 1, [0, 2, 2])
    out["maxit3"] = (A, B, np.ones(30), U.RTOL, 3, [0, 2, 2])
    A = np.diag([1.0, 2.0, -3.0, 4.0])
    out["indefinite"] = (A, _spd(4, 4, 9)[1], np.ones(4), U.RTOL, U.MAXIT, [1] * 4)  # P spans everything: P^H A P is A's congruent
    A, B = _spd(20, 1, 11)
    out["width1"] = (A, B, np.ones(20), U.RTOL, U.MAXIT, [0])
    A, B = _spd(400, 64, 11, lo=1.0, hi=2.0)  # (five steps of full rank: n is large enough that the space is not exhausted)
    out["width64"] = (A, B, np.ones(400), 1e-4, U.MAXIT, [0] * 64)
    A, B = _spd(60, 5, 16, cplx=True)  # (seed: the dependent column's leftover pivot stays below decisions_ok's 1e-16)
    B[:, 3] = (2 - 1j) * B[:, 1]
    out["z_deflated"] = (A, B, np.ones(60), U.RTOL, U.MAXIT, [0] * 5)
    return out


def _hand_cases():
    """modes on hand-made Grams: the breakdowns that no small tile reaches -> name -> model with its ops"""
    out = {}
    G = np.array([[1.0, 0.5, 0], [0.5, 1.0, 0], [0, 0, 1.0]])

    def fresh(maxit=9):
        M = Model(3, 1e-6, DEFTOL, maxit, np.float64)
        M.start_columns([1.0, 4.0, 16.0])
        return M

    M = fresh()
    M.start(np.where(np.eye(3) > 0, 1.0, np.nan))  # a Gram that is not finite: flag 1, 0 iterations
    M.alpha(1, G)  # (a tile that is over is left alone)
    out["nan_at_start"] = M
    M = fresh()
    M.start(np.diag([1.0, -1e-3, 0.5]))
    out["negative_leftover_at_start"] = M
    M = fresh()
    M.start(G)
    M.alpha(1, G)
    M.test(1, np.diag([1e-20, 1.0, 1.0]))  # the first column converges, then the block breaks down: flags 0, 1, 1
    M.next(1, np.zeros((3, 3)))
    M.test(2, G)
    out["rank0_next"] = M
    M = fresh()
    M.start(G)
    M.alpha(1, G)
    M.test(1, G)
    M.next(1, np.diag([1.0, np.inf, 1.0]))
    out["inf_next"] = M
    M = fresh()
    M.start(np.diag([1.0, 1e-20, 0.5]))  # rank 2 of 3
    M.alpha(1, np.diag([2.0, 4.0, 0.0]))
    M.test(1, np.diag([0.25, 0.5, 0.0]))
    M.next(1, np.diag([1.0, 1e-30, 0.0]))  # rank 1
    M.alpha(2, np.array([[1.0, 2, 0], [2, 1.0, 0], [0, 0, 0]]))  # only the leading 1 x 1 counts
    M.test(2, np.zeros((3, 3)))
    out["ranks_fall"] = M
    M = fresh()
    M.start(G)
    M.alpha(1, np.array([[1.0, 2, 0], [2, 1.0, 0], [0, 0, 1.0]]))  # not positive definite: breakdown after 0 steps
    out["indefinite_alpha"] = M
    return out


@pytest.fixture(scope="module")
def tile_program(tmp_path_factory):
    return _build(tmp_path_factory, "blockcg_tile_test")


@pytest.fixture(scope="module")
def models():
    out = {}
    for name, (A, B, minv, rtol, maxit, want) in _tiles().items():
        X, fl, it, rk, M = _run(A, B, minv, rtol, maxit)
        out[name] = (M, (X, fl, it, rk), want)
    for name, M in _hand_cases().items():
        out[name] = (M, None, None)
    return out


def test_the_model_is_the_restatement(models):
    for name, (A, B, minv, rtol, maxit, want) in _tiles().items():
        M, (X, fl, it, rk), _ = models[name]
        trace = []
        Xo, fo, io, ro = U.bcg_restated(lambda r: minv * r, A, B, B.shape[1], rtol, maxit, trace=trace)
        assert U.decisions_ok(trace, MARGIN), name
        assert fl.tolist() == fo.tolist() == want and it.tolist() == io.tolist() and rk == ro.tolist(), (name, fl, fo, it, io, rk, ro)
        ok = np.isfinite(Xo).all(axis=0)
        assert np.abs(X[:, ok] - Xo[:, ok]).max(initial=0.0) <= 1e-9 * max(1.0, np.abs(Xo[:, ok]).max(initial=0.0)), name
    assert {op[0] for M, _, _ in models.values() for op in M.ops} == {0, 1, 2, 3, 4}
    T = {k: v[0] for k, v in models.items()}
    # (what each input is there for)
    assert T["rank_loss"].ctl[1:3] == [5, 3] and T["deflation"].ctl[1] == 5 and T["tiny"].ctl[1] == 3
    assert T["all_zero"].ctl == [0, 0, 0, 3] and len(T["all_zero"].ops) == 2
    assert T["nan_and_zero"].active.tolist() == [True, False, False, True]
    assert T["maxit1"].iter.tolist() == [1] * 3 and T["maxit3"].iter.tolist() == [3] * 3
    assert T["indefinite"].iter.tolist() == [0] * 4 and T["indefinite"].ops[-2][0] == 2 and T["indefinite"].ops[-2][3]["ctl"][0] == 0
    assert T["width64"].ctl[1] == 64 and np.iscomplexobj(T["z_deflated"].C) and T["z_deflated"].ctl[1] == 4
    assert T["nan_at_start"].flag.tolist() == [1, 1, 1] and T["negative_leftover_at_start"].flag.tolist() == [1, 1, 1]
    assert T["rank0_next"].flag.tolist() == [0, 1, 1] and T["rank0_next"].iter.tolist() == [1, 1, 1]
    assert T["inf_next"].flag.tolist() == [1, 1, 1] and T["ranks_fall"].ctl == [0, 2, 1, 1] and T["ranks_fall"].flag.tolist() == [0, 0, 0]
    assert T["indefinite_alpha"].flag.tolist() == [1, 1, 1] and T["indefinite_alpha"].iter.tolist() == [0, 0, 0]


def test_tile_program(tile_program, models, tmp_path):
    path = str(tmp_path / "tiles.txt")
    with open(path, "w") as f:
        for name, (M, _, _) in models.items():
            f.write("%s %d %d %r %r %d %d\n" % (name, M.s, int(np.iscomplexobj(M.C)), M.rtol, M.deftol, M.maxit, len(M.ops)))
            for kind, k, vals, _ in M.ops:
                f.write("%d %d\n" % (kind, k))
                f.write(" ".join(repr(float(v)) for v in vals) if kind == 0 else " ".join(_fmt(v) for v in vals.ravel()))
                f.write("\n")
    out = subprocess.check_output([tile_program, path]).decode()
    lines = [ln for ln in out.splitlines() if ln.startswith("op ")]
    total = sum(len(M.ops) for M, _, _ in models.values())
    assert out.strip().endswith("cases %d OK" % len(models)) and len(lines) == total, out[-2000:]
    it = iter(lines)
    for name, (M, _, _) in models.items():
        s = M.s
        for k, (kind, _, vals, want) in enumerate(M.ops):
            head, fl, its, act, bn, rel, E1, E2, C, pad = (p.split() for p in next(it).split("|"))
            where = (name, k, kind)
            assert head[1] == name and int(head[2]) == k
            assert [int(v) for v in head[3:7]] == want["ctl"], (where, head, want["ctl"])
            assert [int(v) for v in fl] == want["flag"].tolist() and [int(v) for v in its] == want["iter"].tolist(), where
            assert [int(v) for v in act] == want["active"].astype(int).tolist(), where
            assert [float(v) for v in bn] == want["bnorm"].tolist(), where  # (one correctly rounded square root each)
            g, ref = np.array([float(v) for v in rel]), want["relres"]
            assert np.array_equal(np.isinf(g), np.isinf(ref)) and not np.isnan(g).any(), (where, g, ref)
            m = ~np.isinf(ref)
            assert np.abs(g[m] - ref[m]).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(ref[m]).max(initial=0.0)), (where, g, ref)
            assert float(pad[0]) == 0.0, where
            for got, ref, what in ((E1, want["E1"], "E1"), (E2, want["E2"], "E2"), (C, want["C"], "C")):
                v = np.array([float(x) for x in got]).reshape(s, s, 2)
                g = v[..., 0] + 1j * v[..., 1]
                scale = max(1.0, np.abs(ref).max())
                assert np.abs(g - ref).max() <= 1e-10 * scale, (where, what, np.abs(g - ref).max())
