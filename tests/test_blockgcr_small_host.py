"""CPU: the decisions and small matrices of the restarted block GCR driver (hifir_amd/csrc/blockgcr_small.hpp, what k_bgcr_rho
and k_bgcr_small run in one workgroup) as a plain C++ program under the address and undefined sanitizers.  A numpy model of
the five modes (Model) drives whole tiles the way Engine::bgcr_tile does -- it agrees with blockgcr_util.bgcr_restated --
and records every mode's input; tests/cpp/blockgcr_small_test.cpp replays the inputs with a team of one on its own state,
and what it prints after every mode (control words, ranks, flags, steps, residual ratios, E1, E2, C) is held to the model's.
No GPU needed."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from blockcg_util import DEFTOL, _herm, _select, pchol
from blockgcr_util import bgcr_restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Model:
    """the state of a tile of s columns and the five modes of blockgcr_small.hpp; ops collects (kind, a, b, values, snapshot)"""

    def __init__(self, bnorm, active, rtol, deftol, maxit, dtype):
        s = len(bnorm)
        self.s, self.rtol, self.deftol, self.maxit = s, rtol, deftol, maxit
        self.bnorm, self.active = np.asarray(bnorm, float), np.asarray(active, bool)
        self.C, self.E1, self.E2 = (np.zeros((s, s), dtype) for _ in range(3))
        self.ctl, self.q, self.mu = [1, 0, 0, s], 0, 0.0
        self.flag, self.iter = np.zeros(s, int), np.zeros(s, int)
        self.tres, self.relres = np.zeros(s), np.zeros(s)
        self.ops = []

    def _snap(self, kind, a, b, values):
        self.ops.append((kind, a, b, np.array(values), dict(
            ctl=list(self.ctl), q=self.q, mu=self.mu, flag=self.flag.copy(), iter=self.iter.copy(), tres=self.tres.copy(),
            relres=self.relres.copy(), E1=self.E1.copy(), E2=self.E2.copy(), C=self.C.copy())))

    def _end(self, miss, steps):
        self.flag[self.active] = np.where(self.tres[self.active] <= self.rtol, 0, miss)
        self.iter[self.active] = steps
        self.ctl[0] = 0

    def _pad(self, M):
        out = np.zeros_like(self.C)
        out[:M.shape[0], :M.shape[1]] = M
        return out

    def start(self, cycle, steps, rho2):
        if self.ctl[0] != 0:
            with np.errstate(all="ignore"):
                self.rho = np.where(self.active, np.sqrt(rho2), 0.0)
                self.tres = np.where(self.active, self.rho / self.bnorm, 0.0)
            self.relres = self.tres.copy()
            mu = float(self.tres.max())
            if (self.tres <= self.rtol).all():
                self._end(0, steps)
            elif steps >= self.maxit:
                self._end(2, steps)
            elif cycle > 0 and not (mu < self.mu):
                self._end(1, steps)
            else:
                self.mu, self.ctl[0] = mu, 1
        self._snap(0, cycle, steps, rho2)

    def factor(self, first, steps, G):
        if self.ctl[0] == 1:
            self.E1[:], self.E2[:] = 0, 0
            S, piv, r, bad, _, _ = pchol(_herm(G.copy()), self.deftol)
            if first:
                self.ctl[1] = self.ctl[2] = r
            self.ctl[3] = r
            if bad or r == 0:
                self._end(1, steps)
            else:
                self.E1 = self._pad(_select(S, piv, self.s))
                self.C = self._pad(S * self.tres[None, :])
        self._snap(1, int(first), steps, G)

    def basis(self, steps, G):
        if self.ctl[0] == 1:
            r = self.ctl[3]
            self.E1[:], self.E2[:] = 0, 0
            S, piv, q, bad, _, _ = pchol(_herm(G[:r, :r].copy()), self.deftol)
            self.ctl[2], self.q = r, q
            if bad:
                self._end(1, steps)
            elif q == 0:
                self.ctl[0] = 2
            else:
                self.E1 = self._pad(_select(S, piv, r))
        self._snap(2, steps, 0, G)

    def coeff(self, D):
        if self.ctl[0] == 1:
            r, q = self.ctl[3], self.q
            Dm = D[:q, :r]
            self.E2 = self._pad(Dm)
            self.E1 = self._pad((Dm @ self.C[:r, :]) * np.where(self.active, self.bnorm, 0.0)[None, :])
        self._snap(3, 0, 0, D)

    def test(self, steps, last, G):
        if self.ctl[0] == 1:
            r = self.ctl[3]
            self.E1[:], self.E2[:] = 0, 0
            H = _herm(G[:r, :r].copy())
            C = self.C[:r, :]
            with np.errstate(all="ignore"):
                self.relres = np.array([np.sqrt(max(0.0, np.vdot(C[:, j], H @ C[:, j]).real)) for j in range(self.s)])
            if (self.relres <= self.rtol).all() or steps >= self.maxit or last:
                self.ctl[0] = 2
            else:
                S, piv, r1, bad, _, _ = pchol(H, self.deftol)
                if bad:
                    self._end(1, steps)
                elif r1 == 0:
                    self.ctl[0] = 2
                else:
                    self.E1 = self._pad(_select(S, piv, r))
                    self.C = self._pad(S @ C)
                    self.ctl[3] = r1
        self._snap(4, steps, int(last), G)


def _run(A, B, restart, rtol, maxit, deftol=DEFTOL):
    """a whole batch as ONE tile in the launch order of Engine::bgcr_tile, M^{-1} = I -> (X, flags, iters, ranks, model)"""
    n, s = B.shape
    with np.errstate(all="ignore"):
        b2 = np.array([np.vdot(B[:, j], B[:, j]).real for j in range(s)])
    active = (b2 != 0) & np.isfinite(b2)
    M = Model(np.where(active, np.sqrt(np.where(active, b2, 1.0)), 0.0), active, rtol, deftol, maxit, B.dtype)
    M.flag[~np.isfinite(b2)] = 1
    pad = M._pad
    X = np.zeros_like(B)
    Bz = np.where(active[None, :], B, 0)
    steps = 0
    for cycle in range(10 ** 6):
        R = Bz - A @ X if cycle else Bz.copy()
        M.start(cycle, steps, np.array([np.vdot(R[:, j], R[:, j]).real for j in range(s)]))
        live = active & (M.rho != 0) if M.ctl[0] else active
        Rn = np.where(live[None, :], R / np.where(live, M.rho, 1.0)[None, :], 0) if M.ctl[0] else R
        M.factor(cycle == 0, steps, Rn.conj().T @ Rn)
        Rh = Rn @ M.E1
        if M.ctl[0] != 1:
            break
        Qs, Ps = [], []
        for j in range(restart):
            Z = Rh.copy()
            W = A @ Z
            steps += 1
            Cs = [Q.conj().T @ W for Q in Qs]
            for Q, P, Ci in zip(Qs, Ps, Cs):
                W, Z = W - Q @ Ci, Z - P @ Ci
            M.basis(steps, W.conj().T @ W)
            Qj, Pj = W @ M.E1, Z @ M.E1
            Qs.append(Qj)
            Ps.append(Pj)
            M.coeff(Qj.conj().T @ Rh)
            X = X + Pj @ M.E1
            Rh = Rh - Qj @ M.E2
            M.test(steps, j == restart - 1, Rh.conj().T @ Rh)
            if M.ctl[0] != 1:
                break
            Rh = Rh @ M.E1
        if M.ctl[0] == 0:
            break
    return X, M.flag, M.iter, [M.ctl[1], M.ctl[2]], M


def _system(n, s, seed, cplx=False):
    rng = np.random.default_rng(seed)
    A = sp.diags(rng.uniform(1, 3, n)) + 0.3 * sp.random(n, n, density=0.1, random_state=np.random.RandomState(seed))
    B = rng.uniform(-1, 1, (n, s))
    if cplx:
        A = A + 0.2j * sp.random(n, n, density=0.1, random_state=np.random.RandomState(seed + 1))
        B = B + 1j * rng.uniform(-1, 1, (n, s))
    return sp.csr_matrix(A), B


def _tiles():
    """name -> (A, B, restart, rtol, maxit, deftol, expected flags or None)"""
    out = {}
    A, B = _system(40, 6, 3)
    B[:, 3] = B[:, 1]
    B[:, 4] = 0.0
    out["deflated"] = (A, B, 3, 1e-10, 200, DEFTOL, [0] * 6)
    out["one_cycle"] = (A, B, 40, 1e-10, 200, DEFTOL, [0] * 6)
    out["maxit_in_cycle"] = (A, B, 3, 1e-10, 4, DEFTOL, [2, 2, 2, 2, 0, 2])
    out["maxit_at_cycle_end"] = (A, B, 3, 1e-10, 6, DEFTOL, [2, 2, 2, 2, 0, 2])
    out["stagnation"] = (A, B, 3, 1e-18, 200, DEFTOL, [1, 1, 1, 1, 0, 1])
    Bx = B.copy()
    Bx[0, 0] = np.nan
    out["excluded"] = (A, Bx, 3, 1e-10, 200, DEFTOL, [1, 0, 0, 0, 0, 0])
    out["all_zero"] = (A, np.zeros((40, 3)), 3, 1e-10, 200, DEFTOL, [0] * 3)
    Az, Bz = _system(30, 5, 9, cplx=True)
    Bz[:, 2] = (1 - 2j) * Bz[:, 0]
    out["z_deflated"] = (Az, Bz, 4, 1e-9, 200, DEFTOL, [0] * 5)
    A7, B7 = _system(3, 5, 11)
    out["more_columns_than_rows"] = (A7, B7, 4, 1e-10, 50, DEFTOL, [0] * 5)
    return out


def _hand_cases():
    """modes on hand-made Grams: a bad and a rank-0 Gram in every factoring mode -> name -> (model with its ops)"""
    out = {}

    def fresh(s=3, maxit=9, rtol=1e-6):
        M = Model(np.array([1.0, 2.0, 4.0])[:s], np.ones(s, bool), rtol, DEFTOL, maxit, np.float64)
        M.start(0, 0, np.array([1.0, 4.0, 16.0])[:s])
        return M

    G = np.array([[1.0, 0.5, 0], [0.5, 1.0, 0], [0, 0, 1.0]])
    M = fresh()
    M.factor(True, 0, np.where(np.eye(3) > 0, 1.0, np.nan))
    out["nan_at_start"] = M
    M = fresh()
    M.factor(True, 0, np.diag([1.0, -1e-3, 0.5]))
    out["negative_leftover_at_start"] = M
    M = fresh()
    M.factor(True, 0, np.zeros((3, 3)))
    out["rank0_at_start"] = M
    M = fresh()
    M.factor(True, 0, G)
    M.basis(1, np.zeros((3, 3)))  # q = 0: the cycle ends, the later modes leave everything alone
    M.coeff(G)
    M.test(1, False, G)
    M.start(1, 1, np.array([1.0, 4.0, 16.0]))  # mu has not fallen: stagnated
    out["rank0_direction_then_stagnation"] = M
    M = fresh()
    M.factor(True, 0, G)
    M.basis(1, np.diag([1.0, np.inf, 1.0]))
    out["inf_direction"] = M
    M = fresh()
    M.factor(True, 0, G)
    M.basis(1, np.diag([4.0, 1e-20, 1.0]))  # a direction is dropped: q = 2
    M.coeff(np.array([[0.5, 0.1, 0.2], [0.3, -0.4, 0.1], [0, 0, 0]]))
    M.test(1, False, np.diag([0.5, 0.0, 0.25]))  # the residual loses a direction: r' = 2
    M.basis(2, np.diag([1.0, 2.0, 0.0]))
    M.coeff(np.array([[0.1, 0.2, 0], [0.2, 0.1, 0], [0, 0, 0]]))
    M.test(2, False, np.zeros((3, 3)))  # all rel = 0: the cycle ends
    M.start(1, 2, np.array([1e-14, 1e-14, 1e-30]))  # converged on the true residual
    out["rank_falls_then_converges"] = M
    M = fresh()
    M.factor(True, 0, G)
    M.basis(1, G)
    M.coeff(G)
    M.test(1, False, np.diag([1.0, np.nan, 1.0]))  # max(0, NaN) = 0: the cycle ends, and the true residual decides
    M.start(1, 1, np.array([np.nan, 4.0, 16.0]))
    out["nan_residual_gram"] = M
    M = fresh()
    M.factor(True, 0, G)
    M.basis(1, G)
    M.coeff(G)
    M.test(1, False, np.diag([1e-30, 0.0, 0.0]))  # rel <= rtol everywhere: the cycle ends
    M.start(1, 1, np.array([0.25, 1.0, 4.0]))  # mu fell: the next cycle runs
    M.factor(False, 1, G)
    out["second_cycle"] = M
    M = fresh(maxit=1)
    M.factor(True, 0, G)
    M.basis(1, G)
    M.coeff(G)
    M.test(1, False, G)  # steps == maxit ends the cycle
    M.start(1, 1, np.array([0.25, 1e-14, 4.0]))  # flag 0 / 2 by the true residual
    out["maxit"] = M
    return out


def _fmt(v):
    return "%s %s" % (repr(float(np.real(v))), repr(float(np.imag(v))))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bgcr") / "blockgcr_small_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "hifir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "blockgcr_small_test.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def models():
    out = {}
    for name, (A, B, restart, rtol, maxit, deftol, want) in _tiles().items():
        X, fl, it, rk, M = _run(A, B, restart, rtol, maxit, deftol)
        out[name] = (M, (X, fl, it, rk), want)
    for name, M in _hand_cases().items():
        out[name] = (M, None, None)
    return out


def test_the_model_is_the_restatement(models):
    for name, (A, B, restart, rtol, maxit, deftol, want) in _tiles().items():
        M, (X, fl, it, rk), _ = models[name]
        Xo, fo, io, ro = bgcr_restated(lambda r: r, A, B, B.shape[1], restart, rtol, maxit, deftol)
        assert fl.tolist() == fo.tolist() == want and it.tolist() == io.tolist() and rk == ro.tolist(), (name, fl, fo, it, io, rk, ro)
        ok = np.isfinite(Xo).all(axis=0)
        assert np.abs(X[:, ok] - Xo[:, ok]).max(initial=0.0) <= 1e-9 * max(1.0, np.abs(Xo[:, ok]).max(initial=0.0)), name
    kinds = {op[0] for M, _, _ in models.values() for op in M.ops}
    assert kinds == {0, 1, 2, 3, 4}
    # (what the hand-made cases are there for)
    H = {k: v[0] for k, v in models.items()}
    assert H["nan_at_start"].ctl[0] == 0 and H["nan_at_start"].flag.tolist() == [1, 1, 1]
    assert H["negative_leftover_at_start"].flag.tolist() == [1, 1, 1] and H["rank0_at_start"].flag.tolist() == [1, 1, 1]
    assert H["rank0_direction_then_stagnation"].flag.tolist() == [1, 1, 1] and H["inf_direction"].flag.tolist() == [1, 1, 1]
    assert H["rank_falls_then_converges"].flag.tolist() == [0, 0, 0] and H["rank_falls_then_converges"].ctl[1:] == [3, 2, 2]
    assert H["nan_residual_gram"].flag.tolist() == [1, 1, 1] and H["second_cycle"].ctl == [1, 3, 3, 3]
    assert H["maxit"].flag.tolist() == [2, 0, 2] and H["maxit"].iter.tolist() == [1, 1, 1]


def test_small_matrix_program(program, models, tmp_path):
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for name, (M, _, _) in models.items():
            f.write("%s %d %d %r %r %d %d\n" % (name, M.s, int(np.iscomplexobj(M.C)), M.rtol, M.deftol, M.maxit, len(M.ops)))
            f.write(" ".join(repr(float(v)) for v in M.bnorm) + "\n" + " ".join(str(int(a)) for a in M.active) + "\n")
            for kind, a, b, vals, _ in M.ops:
                f.write("%d %d %d\n" % (kind, a, b))
                f.write(" ".join(repr(float(v)) for v in vals) if kind == 0 else " ".join(_fmt(v) for v in vals.ravel()))
                f.write("\n")
    out = subprocess.check_output([program, path]).decode()
    lines = [ln for ln in out.splitlines() if ln.startswith("op ")]
    total = sum(len(M.ops) for M, _, _ in models.values())
    assert out.strip().endswith("cases %d OK" % len(models)) and len(lines) == total, out[-2000:]
    it = iter(lines)
    for name, (M, _, _) in models.items():
        s = M.s
        for k, (kind, a, b, vals, want) in enumerate(M.ops):
            head, fl, its, tres, rel, E1, E2, C, pad = (p.split() for p in next(it).split("|"))
            where = (name, k, kind)
            assert head[1] == name and int(head[2]) == k
            assert [int(v) for v in head[3:7]] == want["ctl"], (where, head, want["ctl"])
            if want["ctl"][0] == 1 and kind >= 2:
                assert int(head[7]) == want["q"], where
            assert float(head[8]) == want["mu"], where
            # (the flag of a column outside the block is k_bcg_beta's, not this header's)
            assert np.array_equal(np.array([int(v) for v in fl])[M.active], want["flag"][M.active]), where
            assert [int(v) for v in its] == want["iter"].tolist(), where
            for got, ref in ((tres, want["tres"]), (rel, want["relres"])):
                g = np.array([float(v) for v in got])
                assert np.array_equal(np.isnan(g), np.isnan(ref)), where
                m = ~np.isnan(ref)
                assert np.abs(g[m] - ref[m]).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(ref[m]).max(initial=0.0)), (where, g, ref)
            assert float(pad[0]) == 0.0, where
            if want["ctl"][0] == 0:
                continue  # (a tile that is over: its coefficients are not used again)
            for got, ref, what in ((E1, want["E1"], "E1"), (E2, want["E2"], "E2"), (C, want["C"], "C")):
                v = np.array([float(x) for x in got]).reshape(s, s, 2)
                g = v[..., 0] + 1j * v[..., 1]
                scale = max(1.0, np.abs(ref).max())
                assert np.abs(g - ref).max() <= 1e-10 * scale, (where, what, np.abs(g - ref).max())
