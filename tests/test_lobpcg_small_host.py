"""CPU: the small-matrix arithmetic of the LOBPCG driver (hifir_amd/csrc/lobpcg_small.hpp, what k_lob_small runs in one
workgroup) as a plain C++ program under the address and undefined sanitizers: tests/cpp/lobpcg_small_test.cpp runs the
cyclic Jacobi eigendecomposition and whole Rayleigh-Ritz steps on the matrices written here, and its eigenvalues, vectors,
pivots, ranks and verdicts are held to numpy's (numpy.linalg.eigh, blockcg_util.pchol).  No GPU needed.

Bounds of the eigendecomposition: the largest eigenvalue difference to numpy's and ||H V - V Theta||_F may be at most 10 x
numpy's own ||H V - V Theta||_F on the same case, with a floor of r 2^-52 ||H||_F; ||V^H V - I||_F at most 10 x numpy's own
with a floor of r 2^-52 (every case here has ||H||_F >= 1, so that floor is not above r 2^-52 ||H||_F).  What the program
reaches, in multiples of the floors, is printed and recorded in lobpcg_util.SMALL_MEASURED."""
import os
import subprocess

import numpy as np
import pytest

from blockcg_util import DEFTOL, _herm, _select, pchol
from lobpcg_util import SMALL_MEASURED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = (1, 2, 3, 17, 47, 48)


def _hermitian(rng, r, cplx):
    H = rng.uniform(-1, 1, (r, r)) + (1j * rng.uniform(-1, 1, (r, r)) if cplx else 0)
    H = _herm(H + H.conj().T)
    return H * (max(1.0, 2.0 / np.linalg.norm(H)))


def _eig_cases():
    rng = np.random.default_rng(97)
    out = {}
    for r in ORDERS:
        out["real%d" % r] = _hermitian(rng, r, False)
        out["cplx%d" % r] = _hermitian(rng, r, True)
    Q = np.linalg.qr(rng.uniform(-1, 1, (12, 12)))[0]
    out["equal"] = _herm(Q @ np.diag([1.0, 1, 1, 2, 2, 3, 3, 3, 3, 5, 7, 7]) @ Q.T)  # equal eigenvalues
    Qz = np.linalg.qr(rng.uniform(-1, 1, (7, 7)) + 1j * rng.uniform(-1, 1, (7, 7)))[0]
    out["equal_z"] = _herm(Qz @ np.diag([2.0, 2, 2, -1, -1, 4, 4]) @ Qz.conj().T)
    out["diagonal"] = np.diag([3.0, -1, 2, 2, 0, 5, -4, 1])  # already diagonal: one sweep, no rotation
    out["identity"] = np.eye(9)
    out["null"] = _herm(Q[:, :5] @ np.diag([1.0, 2, 3, 4, 5]) @ Q[:, :5].T)  # seven zero eigenvalues
    return out


def _basis_case(rng, n, k, cplx, zero_w=None, dup_p=None, nan=False):
    """A basis [X W P] of 3 k columns with its two Grams -> (GB, GA)"""
    s = 3 * k
    S = rng.uniform(-1, 1, (n, s)) + (1j * rng.uniform(-1, 1, (n, s)) if cplx else 0)
    S[:, k:2 * k] *= 1e-5  # (a residual block is small beside X)
    if zero_w is not None:
        S[:, k + zero_w] = 0.0
    if dup_p is not None:
        S[:, 2 * k + dup_p] = S[:, 2 * k + (dup_p + 1) % k]
    B = rng.uniform(-1, 1, (n, n)) + (1j * rng.uniform(-1, 1, (n, n)) if cplx else 0)
    A = _herm(B @ B.conj().T) / n + np.diag(np.arange(1.0, n + 1.0))
    GB, GA = S.conj().T @ S, S.conj().T @ (A @ S)
    if nan:
        GA[1, 2] = np.nan
    return GB, GA


def _rr_cases():
    """name -> (GB, GA, k, expectation)"""
    rng = np.random.default_rng(98)
    out = {}
    out["full_k5"] = _basis_case(rng, 80, 5, False) + (5, dict(r=15, bad=False))
    out["full_k16"] = _basis_case(rng, 200, 16, False) + (16, dict(r=48, bad=False))
    out["full_k16_z"] = _basis_case(rng, 200, 16, True) + (16, dict(r=48, bad=False))
    out["k1"] = _basis_case(rng, 30, 1, False) + (1, dict(r=3, bad=False))
    out["zero_w"] = _basis_case(rng, 80, 4, False, zero_w=2) + (4, dict(r=11, bad=False))
    out["zero_w_z"] = _basis_case(rng, 80, 4, True, zero_w=1) + (4, dict(r=11, bad=False))
    out["dup_p"] = _basis_case(rng, 80, 4, False, dup_p=1) + (4, dict(r=11, bad=False))
    out["dup_p_z"] = _basis_case(rng, 80, 6, True, dup_p=0, zero_w=5) + (6, dict(r=16, bad=False))
    out["nan_ga"] = _basis_case(rng, 40, 3, False, nan=True) + (3, dict(bad=True))
    GB, GA = _basis_case(rng, 40, 3, False)
    GB[0, 4] = np.inf
    out["inf_gb"] = (GB, GA, 3, dict(bad=True))
    S = rng.uniform(-1, 1, (40, 9))
    S[:, 1], S[:, 3:] = S[:, 0], 0.0  # X has a duplicate column, W and P are zero: rank 2 < k
    out["rank_below_k"] = (S.T @ S, S.T @ (np.arange(1.0, 41.0)[:, None] * S), 3, dict(r=2, bad=True))
    return out


def _start_cases():
    """name -> (GB = X0^H X0, expectation (running, verdict))"""
    rng = np.random.default_rng(99)
    out = {}
    X = rng.uniform(-1, 1, (30, 5))
    out["fine"] = (X.T @ X, (1, 0))
    Xz = X + 1j * rng.uniform(-1, 1, (30, 5))
    out["fine_z"] = (Xz.conj().T @ Xz, (1, 0))
    D = X.copy()
    D[:, 3] = D[:, 1]
    out["duplicate"] = (D.T @ D, (0, 1))
    Z = X.copy()
    Z[:, 0] = 0.0
    out["zero_column"] = (Z.T @ Z, (0, 1))
    N = X.T @ X
    N[1, 2] = np.nan
    out["nan"] = (N, (0, 2))
    out["k1"] = (np.array([[4.0]]), (1, 0))
    return out


def _test_cases():
    """name -> (k, nev, step, maxit, tol, anorm, partials [nb][16], expectation (running, flags or None))"""
    rng = np.random.default_rng(100)
    out = {}
    P = rng.uniform(0, 1, (7, 16)) * 1e-12  # res around 1e-6 / anorm
    out["none_converged"] = (5, 5, 3, 10, 1e-9, 2.0, P, (1, None))
    out["at_maxit"] = (5, 5, 10, 10, 1e-9, 2.0, P, (0, [2] * 5))
    Q = P.copy()
    Q[:, :3] *= 1e-10
    out["wanted_converged"] = (5, 3, 4, 10, 1e-9, 2.0, Q, (0, [0, 0, 0, 2, 2]))
    out["guard_only"] = (5, 4, 4, 10, 1e-9, 2.0, Q, (1, None))
    out["zero_norm"] = (2, 2, 0, 10, 1e-9, 0.0, np.zeros((3, 16)), (0, [0, 0]))
    R = P.copy()
    R[2, 1] = np.nan
    out["nan_at_maxit"] = (3, 3, 10, 10, 1e-9, 2.0, R, (0, [2, 2, 2]))
    return out


def _fmt(v):
    return "%s %s" % (repr(float(np.real(v))), repr(float(np.imag(v))))


def _upper(G):
    """what the Gram kernel leaves: the upper triangle; the strict lower one holds something else"""
    return np.triu(G) + np.tril(np.full(G.shape, 123.0), -1)


def _from_upper(G):
    H = np.triu(G) + np.triu(G, 1).conj().T
    if np.iscomplexobj(H):
        H[np.diag_indices_from(H)] = H.diagonal().real
    return H


_DECISIONS = []  # what output() leaves for test_start_and_residual_decisions: cases and the program's lines


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    d = tmp_path_factory.mktemp("lob")
    exe = str(d / "lobpcg_small_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "hifir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "lobpcg_small_test.cpp"), "-o", exe])
    path = str(d / "cases.txt")
    eig, rr = _eig_cases(), _rr_cases()
    starts, tests = _start_cases(), _test_cases()
    with open(path, "w") as f:
        for name, (G, _) in starts.items():
            f.write("start %s %d %r %d\n" % (name, G.shape[0], DEFTOL, int(np.iscomplexobj(G))))
            f.write(" ".join(_fmt(v) for v in _upper(G).ravel()) + "\n")
        for name, (k, nev, step, maxit, tol, anorm, P, _) in tests.items():
            f.write("test %s %d %d %d %d %r %r %d\n" % (name, k, nev, step, maxit, tol, anorm, P.shape[0]))
            f.write(" ".join(repr(float(v)) for v in P.ravel()) + "\n")
        for name, H in eig.items():
            f.write("eig %s %d %d\n" % (name, H.shape[0], int(np.iscomplexobj(H))))
            f.write(" ".join(_fmt(v) for v in H.ravel()) + "\n")
        for name, (GB, GA, k, _) in rr.items():
            f.write("rr %s %d %d %r %d\n" % (name, GB.shape[0], k, DEFTOL, int(np.iscomplexobj(GB))))
            f.write(" ".join(_fmt(v) for v in _upper(GB).ravel()) + "\n")
            f.write(" ".join(_fmt(v) for v in _upper(GA).ravel()) + "\n")
    out = subprocess.check_output([exe, path]).decode()
    assert out.strip().endswith("cases %d OK" % (len(eig) + len(rr) + len(starts) + len(tests))), out[-2000:]
    lines = out.splitlines()
    _DECISIONS[:] = (starts, tests, [ln for ln in lines if ln.startswith("start ")], [ln for ln in lines if ln.startswith("test ")])
    return eig, rr, [ln for ln in lines if ln.startswith("eig ")], [ln for ln in lines if ln.startswith("rr ")]


def _cvals(words, shape):
    v = np.array([float(x) for x in words]).reshape(shape + (2,))
    return v[..., 0] + 1j * v[..., 1]


def test_jacobi_against_numpy(output):
    eig, _, lines, _ = output
    assert len(lines) == len(eig)
    worst = dict(eigenvalues=0.0, residual=0.0, orthogonality=0.0)
    for ln, (name, H) in zip(lines, eig.items()):
        head, theta, V = (part.split() for part in ln.split("|"))
        assert head[1] == name
        r = H.shape[0]
        sweeps = int(head[2])
        th = np.array([float(v) for v in theta])
        V = _cvals(V, (r, r))
        if not np.iscomplexobj(H):
            assert not V.imag.any()
        wn, Vn = np.linalg.eigh(H)
        fro = np.linalg.norm(H)
        floor = r * 2.0 ** -52 * fro
        res_np, orth_np = np.linalg.norm(H @ Vn - Vn * wn), np.linalg.norm(Vn.conj().T @ Vn - np.eye(r))
        res, orth = np.linalg.norm(H @ V - V * th), np.linalg.norm(V.conj().T @ V - np.eye(r))
        dth = np.abs(th - wn).max()
        assert (np.diff(th) >= 0).all() and 1 <= sweeps <= 12, (name, sweeps)
        assert dth <= max(10 * res_np, floor), (name, dth, res_np, floor)
        assert res <= max(10 * res_np, floor), (name, res, res_np, floor)
        assert orth <= max(10 * orth_np, r * 2.0 ** -52), (name, orth, orth_np)
        worst["eigenvalues"] = max(worst["eigenvalues"], dth / floor)
        worst["residual"] = max(worst["residual"], res / floor)
        worst["orthogonality"] = max(worst["orthogonality"], orth / (r * 2.0 ** -52))
        if name in ("diagonal", "identity"):
            assert sweeps == 1 and np.array_equal(th, np.sort(H.diagonal())), name
            assert np.array_equal(np.abs(V), np.eye(r)[:, np.argsort(H.diagonal(), kind="stable")]), name
    print("multiples of the floors:", worst)
    for key, v in worst.items():  # (recorded, not asserted: the figures depend on the installed LAPACK's eigh too)
        print(key, "measured", v, "recorded", SMALL_MEASURED[key])


def test_rayleigh_ritz_against_numpy(output):
    _, rr, _, lines = output
    assert len(lines) == len(rr)
    for ln, (name, (GB, GA, k, want)) in zip(lines, rr.items()):
        head, piv, lam, C, Cp = (part.split() for part in ln.split("|"))
        assert head[1] == name
        r, bad, sweeps = int(head[2]), bool(int(head[3])), int(head[4])
        s = GB.shape[0]
        assert bad == want["bad"], (name, bad)
        finite = np.isfinite(np.triu(GB)).all()
        if finite:
            GBh = _from_upper(GB)
            dg = GBh.diagonal().real
            D = np.where(dg > 0, 1.0 / np.sqrt(np.where(dg > 0, dg, 1.0)), 0.0)
            T, pn, rn, bn, kept, dropped = pchol(_from_upper(np.triu(GBh * D[:, None] * D[None, :])), DEFTOL)
            assert r == rn and [int(p) for p in piv] == [int(p) for p in pn], (name, r, rn, piv, pn)
            assert r == want.get("r", r), (name, r)
        if bad:
            assert not lam and not C
            continue
        E = D[:, None] * _select(T, pn, s)
        th, V = np.linalg.eigh(_herm(E.conj().T @ _from_upper(GA) @ E))
        lam = np.array([float(v) for v in lam])
        C, Cp = _cvals(C, (s, k)), _cvals(Cp, (s, k))
        scale = np.abs(th).max()
        assert np.abs(lam - th[:k]).max() <= 1e-10 * scale, (name, np.abs(lam - th[:k]).max())
        # (kept pivots of 1e-10 give inv(T) entries of 1e5: the products hold to 1e-6, the eigenvalues far better)
        assert np.linalg.norm(C.conj().T @ GBh @ C - np.eye(k)) <= 1e-6, name
        assert np.linalg.norm(C.conj().T @ _from_upper(GA) @ C - np.diag(lam)) <= 1e-6 * scale, name
        assert np.array_equal(Cp[k:], C[k:]) and not Cp[:k].any() and 1 <= sweeps <= 12, name
        assert not C[D == 0.0].any(), name  # a zero column takes no part


def test_start_and_residual_decisions(output):
    """lob::start_factor and lob::residual_test: the verdicts, flags and counts that k_lob_small writes"""
    starts, tests, ls, lt = _DECISIONS
    assert len(ls) == len(starts) and len(lt) == len(tests)
    for ln, (name, (G, (running, verdict))) in zip(ls, starts.items()):
        head, E = (part.split() for part in ln.split("|"))
        assert head[1] == name and (int(head[2]), int(head[3])) == (running, verdict), ln[:80]
        if running:
            k = G.shape[0]
            E = _cvals(E, (k, k))
            assert np.linalg.norm(E.conj().T @ _from_upper(G) @ E - np.eye(k)) <= 1e-12, name
    for ln, (name, (k, nev, step, maxit, tol, anorm, P, (running, flags))) in zip(lt, tests.items()):
        head, res, active, flag, it = (part.split() for part in ln.split("|"))
        assert head[1] == name and int(head[2]) == running, ln[:80]
        tot = P[0, :k].copy()
        for b in range(1, P.shape[0]):
            tot = tot + P[b, :k]
        want = np.sqrt(tot) / anorm if anorm > 0 else np.sqrt(tot)
        got = np.array([float(v) for v in res])
        assert np.array_equal(got, want, equal_nan=True), name  # the same sums in the same order
        with np.errstate(invalid="ignore"):
            assert [int(v) for v in active] == [0 if r <= tol else 1 for r in want], name
        if flags is None:
            assert [int(v) for v in flag] == [-1] * k and [int(v) for v in it] == [-1] * k, name  # untouched
        else:
            assert [int(v) for v in flag] == flags and [int(v) for v in it] == [step] * k, name
