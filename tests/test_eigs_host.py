"""CPU: pins the inputs of test_gpu_eigs.py (eigs_util) around the oracle's apply.  Every case of the table, standard and
generalized: the restated sweeps lock every wanted column, in the pinned (want, locked, steps) per sweep; the eigenvalues
agree with numpy.linalg.eigh / scipy.linalg.eigh(A, B) to tol ||A||_inf; nev ends between two eigenvalue clusters; X is
B-orthonormal and B-orthogonal to the caller's Y; the recurrence's residual stays within DRIFT of the true one; every decision
of every sweep keeps its margin; the sweeps' counts survive six runs with one rounding of noise per element, or move by what
the table says.  Also: the projector's restatement, the new symbols declared, exported and typed, the refusals that need no
GPU, and the sweep loop's host decisions as a plain C++ program under the address and undefined sanitizers
(tests/cpp/eigs_small_test.cpp)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import eigs_util as E
import hifir_amd
import lobpcg_gen_util as G
import lobpcg_util as U
from hifir_amd import _lib
from lockstep_edges_util import MARGIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hifamd_eig_project", "hifamd_eig_project_dev", "hifamd_eigs", "hifamd_eigs_dev")
NAMES = [c[0] for c in E.CASES]


def _gram(Cs, B, Y, X):
    Z = X if Y is None else np.hstack([Y, X])
    return Z.conj().T @ (Z if B is None else B @ Z)


def test_the_table_is_the_issues():
    rows = {(c[1], c[2], c[3], c[4], c[5]) for c in E.CASES}
    assert rows == {("p2d_32_symm", False, 40, 16, 4), ("p2d_32_symm", False, 30, 8, 2), ("twobody_symm", False, 20, 8, 2),
                    ("p2d_32_symm_z", False, 20, 16, 4), ("neu2d_32_symm", False, 20, 8, 2), ("p2d_32_symm", True, 40, 16, 4),
                    ("twobody_symm", True, 20, 8, 2), ("p2d_32_symm_z", True, 20, 16, 4), ("neu2d_32_symm", True, 12, 8, 2)}
    assert all(U.case(c[1]).n <= 1024 for c in E.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_where_the_wanted_eigenvalues_end(name):
    """the gap behind the cluster that lambda_nev closes: a changed fixture fails here.  Every case but the two 40 / 16 / 4 on
    the real Poisson grid ends between two clusters; those two end inside the double eigenvalue eig[39] == eig[40]."""
    row = E.case_row(name)
    Cs, nev, tol = U.case(row[1]), row[3], row[6]
    eig, ce = E.dense_spectrum(name), E.cluster_end(name)
    gap = eig[ce] - eig[ce - 1]
    print(name, "nev", nev, "cluster end", ce, "eig[nev-2 .. nev+1]", eig[nev - 2:nev + 2], "gap / ||A||", gap / Cs.anorm)
    assert ce == (41 if name in ("p32_40", "gen_p32_40") else nev), (name, ce)
    assert gap >= E.GAP * Cs.anorm and gap >= 1e3 * tol * Cs.anorm
    if ce > nev:
        assert eig[ce - 1] - eig[nev - 1] <= 1e-12 * Cs.anorm  # one multiple eigenvalue, not a smear


@pytest.mark.parametrize("name", NAMES)
def test_sweeps_flags_eigenvalues_and_orthogonality(name):
    Cs, B, Y, row, (lam, X, res, fl, sweeps, minrank), tr = E.reference(name)
    _, fixture, gen, nev, k, guard, tol, seed, want, spread = row
    print(name, "sweeps", sweeps, "total", sum(s[2] for s in sweeps), "smallest rank", minrank)
    assert tuple(sweeps) == want and fl.tolist() == [0] * nev and sum(s[1] for s in sweeps) == nev
    eig = E.dense_spectrum(name)
    err = np.abs(lam - eig[:nev]).max() / Cs.anorm
    true = E.true_residuals(Cs, B, lam, X)
    orth = np.linalg.norm(_gram(Cs, B, Y, X) - np.eye(nev + (0 if Y is None else Y.shape[1])))
    drift = np.abs(true - res).max()
    print("  max |lam - dense| / ||A||_inf", err, " ||[Y X]^H B [Y X] - I||_F", orth, " max true res", true.max(),
          " drift |res - true|", drift, " margin drift / tol", drift / tol)
    assert err <= tol and (res <= tol).all() and (np.diff(lam) >= -tol * Cs.anorm).all()
    assert drift <= E.DRIFT and (true <= tol + E.DRIFT).all()
    assert orth <= E.ORTH_MEASURED
    if Y is not None:  # the singular pencil: the smallest NONZERO eigenvalues, nothing of the null space
        assert abs(G.pencil_eigenvalues(fixture)[0]) <= 1e-12 * Cs.anorm and lam[0] >= 1e-3 * Cs.anorm
    # the spanned subspace against the dense invariant one: Davis-Kahan with the asserted gap
    defect, bound = E.subspace_defect(name, lam, X)
    print("  subspace defect", defect, "bound", bound)
    assert defect <= bound + 1e-12
    if not gen:  # every residual is at most tol ||A||_inf and the gap at least GAP ||A||_inf: sqrt(tol)-scale
        assert bound <= np.sqrt(nev) * (tol + E.DRIFT) / E.GAP


@pytest.mark.parametrize("name", NAMES)
def test_every_decision_of_every_sweep_keeps_its_margin(name):
    Cs, B, Y, row, out, traces = E.reference(name)
    assert len(traces) == len(row[8]) and all(E.decisions_ok(tr, MARGIN) for tr in traces), name
    low = min(abs(np.log(v)) for tr in traces for st in tr for v in st["ratios"] if v > 0)
    print(name, "closest res_j / tol to 1, as a factor:", float(np.exp(low)))


@pytest.mark.parametrize("name", NAMES)
def test_counts_under_one_rounding_of_noise(name):
    """six noisy restatements: the same (want, locked) per sweep, and the largest difference of a sweep's count is exactly
    the row's spread (0 on the six stable rows)"""
    Cs, B, Y, row, out, traces = E.reference(name)
    _, fixture, gen, nev, k, guard, tol, seed, want, spread = row
    worst = 0
    for sd in E.NOISE_SEEDS:
        o = E.eigs_restated(Cs.O, Cs.A, B, nev, k, guard, tol, Y=Y, seed=seed, noise=np.random.default_rng(sd))
        assert [s[:2] for s in o[4]] == [s[:2] for s in want] and o[3].tolist() == [0] * nev, (name, sd, o[4])
        worst = max(worst, max(abs(a[2] - b[2]) for a, b in zip(o[4], want)))
    print(name, "largest difference of a sweep's count under noise:", worst, "spread", spread)
    assert worst == spread


def test_drift_and_orthogonality_figures_are_the_measured_ones():
    worst_drift = worst_orth = 0.0
    for name in NAMES:
        Cs, B, Y, row, (lam, X, res, fl, sweeps, minrank), tr = E.reference(name)
        worst_drift = max(worst_drift, float(np.abs(E.true_residuals(Cs, B, lam, X) - res).max()))
        worst_orth = max(worst_orth, float(np.linalg.norm(_gram(Cs, B, Y, X) - np.eye(row[3] + (0 if Y is None else 1)))))
    print("largest drift", worst_drift, "largest orthogonality defect", worst_orth)
    assert E.DRIFT / 10 <= worst_drift <= E.DRIFT and E.ORTH_MEASURED / 2 <= worst_orth <= E.ORTH_MEASURED
    assert E.ORTH_BOUND == pytest.approx(U.SMALL_MEASURED["orthogonality"] * E.ORTH_MEASURED) and E.ORTH_BOUND <= 1e-12


def test_projector_restated():
    rng = np.random.default_rng(3)
    for cplx in (False, True):
        n, m, kw = 101, 17, 5
        B = G.diagonal_mass(n)[0]
        Z = rng.standard_normal((n, m)) + (1j * rng.standard_normal((n, m)) if cplx else 0)
        W = rng.standard_normal((n, kw)) + (1j * rng.standard_normal((n, kw)) if cplx else 0)
        for Bm in (None, B):
            # B-orthonormalize by a Cholesky of the Gram
            Gm = Z.conj().T @ (Z if Bm is None else Bm @ Z)
            Y = Z @ np.linalg.inv(np.linalg.cholesky(Gm).conj().T)
            BY = Y if Bm is None else Bm @ Y
            assert np.abs(Y.conj().T @ BY - np.eye(m)).max() <= 1e-13
            P = E.project_restated(W, Y, Bm)
            assert np.abs(BY.conj().T @ P).max() <= 1e-13 * np.abs(W).max() * n
            assert np.abs(E.project_restated(P, Y, Bm) - P).max() <= 1e-13 * np.abs(W).max() * n  # idempotent
            Wz = W.copy()
            Wz[:, 2] = 0.0
            assert not E.project_restated(Wz, Y, Bm)[:, 2].any()
    c = E.b_normalized_constant(G.mass2d(32))
    assert c.shape == (1024, 1) and abs((c.T @ (G.mass2d(32) @ c))[0, 0] - 1.0) <= 1e-14
    assert np.abs(U.case("neu2d_32_symm").A @ c).max() <= 1e-13  # the null vector of the Neumann stiffness matrix


# ---- the new symbols --------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_typed():
    with open(os.path.join(ROOT, "include", "hifir_amd.h")) as f:
        header = f.read()
    lib = hifir_amd.lib()
    for name in NEW:
        assert re.search(r"HifAmdStatus\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(lib, name).restype is C.c_int
        assert list(getattr(lib, name).argtypes) == list(_lib.SIGNATURES[name][1])
    assert re.search(r"int\s+hifamd_eigs_sweeps\s*\(", header) and "hifamd_eigs_sweeps" in _lib.SIGNATURES
    assert _lib.SIGNATURES["hifamd_eigs"][1] == _lib.SIGNATURES["hifamd_eigs_dev"][1] and len(_lib.SIGNATURES["hifamd_eigs"][1]) == 21
    assert _lib.SIGNATURES["hifamd_eig_project"][1] == _lib.SIGNATURES["hifamd_eig_project_dev"][1]

    def args(name):
        return re.sub(r"\bd([XYW])", r"\1", re.sub(r"\s+", " ", re.search(r"HifAmdStatus\s+%s\s*\(([^;]*)\);" % name, header).group(1)))

    assert args("hifamd_eigs") == args("hifamd_eigs_dev") and args("hifamd_eig_project") == args("hifamd_eig_project_dev")
    assert [p.strip().split()[-1].lstrip("*") for p in args("hifamd_eigs").split(",")] == [
        "h", "gen", "nev", "k", "guard", "Y", "ldy", "m0", "X0", "ldx0", "seed", "tol", "deftol", "maxit", "rank", "lambda", "X",
        "ldx", "res", "flags", "info4"]
    sig = inspect.signature(hifir_amd.HIF.eigsh)
    assert list(sig.parameters) == ["self", "nev", "k", "guard", "gen", "Y", "X0", "seed", "tol", "maxit", "deftol", "full_rank"]
    assert [sig.parameters[p].default for p in ("k", "guard", "gen", "Y", "X0", "seed", "tol", "maxit", "deftol", "full_rank")] == [
        16, None, False, None, None, 0, 1e-8, 200, 1e-12, False]
    assert list(inspect.signature(hifir_amd.HIF.b_project).parameters) == ["self", "W", "Y", "gen"]
    with open(os.path.join(ROOT, "include", "hifir_amd.hpp")) as f:
        facade = f.read()
    assert "eigsh(" in facade and "b_project(" in facade and "hifamd_eigs(" in facade and "hifamd_eig_project(" in facade


def test_refusals_that_need_no_gpu():
    lib = hifir_amd.lib()
    X = np.zeros((4, 2))
    for fn in (lib.hifamd_eigs, lib.hifamd_eigs_dev):
        assert fn(None, 0, 2, 2, 0, None, 0, 0, None, 0, 0, 1e-8, 1e-12, 10, 0, None, X.ctypes.data, 2, None, None, None) == 1
    for fn in (lib.hifamd_eig_project, lib.hifamd_eig_project_dev):
        assert fn(None, 0, 2, X.ctypes.data, 2, 2, X.ctypes.data, 2) == 1  # HIFAMD_NULL_OBJ
    assert lib.hifamd_eigs_sweeps(None, None, 0) == -1


# ---- the host decisions between sweeps under sanitizers ---------------------------------------------------------------------
def test_sweep_decisions_under_sanitizers(tmp_path):
    exe = str(tmp_path / "eigs_small_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "hifir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "eigs_small_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("EIGS SMALL TEST OK") and "FAIL" not in out.stdout
