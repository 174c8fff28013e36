"""CPU: pins the inputs of test_gpu_lobpcg_gen.py (lobpcg_gen_util) around the oracle's apply -- on every case the restatement
of the generalized iteration reaches flag 0 on its first nev columns in the pinned number of steps, its eigenvalues agree with
scipy.linalg.eigh(A, B) to tol ||A||_inf, its vectors are B-orthonormal to 1e-12, the recurrence's residual stays within
GEN_DRIFT of the true backward error, and every decision keeps its margin and survives six runs with one rounding of noise per
element.  Also: the bit-equality case of the GPU test (B = I: no column converged under either driver's scaling through
BIT_EQUAL_MAXIT steps), the new symbols declared, exported and typed, the refusals that need no GPU, and lob::residual_test_gen
as a plain C++ program under the address and undefined sanitizers (tests/cpp/lobpcg_gen_small_test.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import hifir_amd
import lobpcg_gen_util as G
import lobpcg_util as U
from hifir_amd import _lib
from lockstep_edges_util import MARGIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hifamd_set_mass_matrix", "hifamd_lobpcg_gen", "hifamd_lobpcg_gen_dev")


@pytest.fixture(scope="module")
def restated():
    return {c[0]: G.reference(c[0]) for c in G.GEN_CASES}


def test_cases_cover_the_tiles_the_issue_names():
    ks = {c[2] for c in G.GEN_CASES if c[1] == "p2d_32_symm"}
    assert {1, 2, 5, 15, 16} <= ks
    assert any(c[2] == 16 and c[3] == 13 for c in G.GEN_CASES) and any(c[1].endswith("_z") for c in G.GEN_CASES)
    assert all(U.case(c[1]).n <= 1024 for c in G.GEN_CASES)


def test_mass_matrices():
    B = G.mass2d(32)
    assert B.shape == (1024, 1024) and abs(B - B.T).max() == 0 and abs(G.norm_inf(B) - 1.0) <= 1e-15
    assert np.linalg.eigvalsh(B.toarray())[0] > 0.1
    Cz, Cr = U.case("p2d_32_symm_z"), U.case("p2d_32_symm")
    phi = G.phase(Cz.n)
    assert abs(sp.diags(phi) @ Cr.A.astype(np.complex128) @ sp.diags(phi.conj()) - Cz.A).max() == 0  # the Phi of the fixture
    Bz = G.mass_of("p2d_32_symm_z")
    assert np.iscomplexobj(Bz.data) and abs(Bz.imag).max() > 0.01 and abs(Bz - Bz.conj().T).max() == 0
    # the same pencil up to the similarity: the same eigenvalues
    assert np.abs(G.pencil_eigenvalues("p2d_32_symm_z") - G.pencil_eigenvalues("p2d_32_symm")).max() <= 1e-12 * Cr.anorm
    L = G.mass_of("twobody_symm")
    assert L.nnz == U.case("twobody_symm").n and 0.5 <= L.data.min() and L.data.max() <= 2.0
    Bd, b = G.diagonal_mass(37)
    assert set(np.log2(b)) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and len(set(b)) > 1


def test_flags_counts_and_eigenvalues(restated):
    for name, fixture, k, nev, tol, want, seed in G.GEN_CASES:
        (Cs, solve, B, X0, _, _, _), (lam, X, res, fl, steps, rank), tr = restated[name]
        print(name, "steps", steps, "rank", rank, "flags", fl.tolist())
        assert fl[:nev].tolist() == [0] * nev and steps == want and k <= rank <= 3 * k, (name, fl, steps, rank)
        assert (res[:nev] <= tol).all() and len(tr) == steps + 1, name
        eig = G.pencil_eigenvalues(fixture)
        assert np.abs(lam[:nev] - eig[:nev]).max() <= tol * Cs.anorm, (name, np.abs(lam[:nev] - eig[:nev]).max() / Cs.anorm)
        assert (np.diff(lam) >= 0).all() and np.linalg.norm(X.conj().T @ (B @ X) - np.eye(k)) <= 1e-12, name
    assert restated["p32z_k5"][0][0].cplx
    assert 2 in restated["p32_k16"][1][3][13:].tolist()  # the guard columns did not hold the solve up


def test_recurrence_drift(restated):
    worst = 0.0
    for name, ((Cs, solve, B, *_), (lam, X, res, fl, steps, rank), tr) in restated.items():
        true = G.backward_errors(Cs.A, B, lam, X)
        worst = max(worst, float(np.abs(true - res).max()))
    print("largest |res_j - true backward error|:", worst)
    assert G.GEN_DRIFT / 10 <= worst <= G.GEN_DRIFT


def test_every_decision_keeps_its_margin(restated):
    for name, (inp, out, tr) in restated.items():
        assert G.decisions_ok(tr, MARGIN), name
    # (the trace is not empty where it matters: a basis that lost columns, and a leftover pivot that is not an exact zero)
    assert any(st.get("rank", 48) < 3 * len(st["ratios"]) for st in restated["p32_k16"][2])
    assert any("kept" in st and st["dropped"] != 0.0 for (_, _, tr) in restated.values() for st in tr)


def test_step_counts_do_not_hang_on_a_rounding(restated):
    for name, ((Cs, solve, B, X0, k, nev, tol), out, tr) in restated.items():
        for sd in G.NOISE_SEEDS:
            t2 = []
            o = G.lobpcg_gen_restated(solve, Cs.A, B, X0, nev, tol, G.MAXIT, trace=t2, noise=np.random.default_rng(sd))
            assert o[4] == out[4] and o[3].tolist() == out[3].tolist() and G.decisions_ok(t2, MARGIN), (name, sd, o[4], out[4])


def test_bit_equality_case_has_no_converged_column_under_either_scaling():
    """B = I: through BIT_EQUAL_MAXIT steps every res_j / tol of the standard restatement and of the generalized one stays
    above MARGIN, so neither driver locks a column and the device's two paths must agree bit for bit; one step later a column
    converges, so the window is not vacuous.  In exact arithmetic the two iterations are the same one: their Ritz values agree."""
    m = G.BIT_EQUAL_MAXIT
    for name in G.BIT_EQUAL:
        Cs, solve, B, X0, k, nev, tol = G.inputs(name)
        assert k == 5
        I = sp.identity(Cs.n, format="csr", dtype=Cs.A.dtype)
        tg, ts = [], []
        og = G.lobpcg_gen_restated(solve, Cs.A, I, X0, nev, tol, m, trace=tg)
        os_ = U.lobpcg_restated(solve, Cs.A, X0, nev, tol, m, trace=ts)
        assert og[4] == os_[4] == m and len(tg) == len(ts) == m + 1
        low = min(min(min(st["ratios"]) for st in tg), min(min(st["ratios"]) for st in ts))
        print(name, "smallest res_j / tol through step", m, ":", low)
        assert low > MARGIN and og[3].tolist() == os_[3].tolist() == [2] * k
        assert np.abs(og[0] - os_[0]).max() <= 1e-12 * Cs.anorm
        longer = []
        G.lobpcg_gen_restated(solve, Cs.A, I, X0, nev, tol, m + 1, trace=longer)
        assert min(longer[m + 1]["ratios"]) < 1.0 / MARGIN


def test_maxit_and_refused_starts(restated):
    (Cs, solve, B, X0, k, nev, tol), (lam, X, res, fl, steps, rank), tr = restated["p32_k5"]
    short = G.lobpcg_gen_restated(solve, Cs.A, B, X0, nev, tol, steps - 1)
    assert short[4] == steps - 1 and 2 in short[3].tolist() and set(short[3].tolist()) <= {0, 2}
    at = G.lobpcg_gen_restated(solve, Cs.A, B, X0, nev, tol, steps)
    assert at[4] == steps and at[3].tolist() == [0] * k and np.array_equal(at[0], lam)
    dup = X0.copy()
    dup[:, 3] = dup[:, 1]
    with pytest.raises(G.StartRefused, match="rank deficient"):
        G.lobpcg_gen_restated(solve, Cs.A, B, dup, nev, tol, 10)
    with pytest.raises(G.StartRefused, match="not positive definite"):
        G.lobpcg_gen_restated(solve, Cs.A, -B, X0, nev, tol, 10)
    bad = X0.copy()
    bad[7, 2] = np.nan
    with pytest.raises(G.StartRefused, match="non-finite"):
        G.lobpcg_gen_restated(solve, Cs.A, B, bad, nev, tol, 10)


def test_diagonal_pencils_for_the_gpu_test():
    for n in (37, 101):
        levels, A, a = U.diagonal_case(n)
        B, b = G.diagonal_mass(n)
        q = a / b
        order = np.argsort(q, kind="stable")
        assert len(set(q[order[:4]])) == 4  # the smallest quotients are distinct
        X0 = np.zeros((n, 3))
        X0[order[:3], [2, 0, 1]] = [2.0, -1.0, 0.5]
        lam, X, res, fl, steps, rank = G.lobpcg_gen_restated(lambda r: r, A, B, X0, 3, 1e-10, 50)
        assert steps == 0 and fl.tolist() == [0, 0, 0] and lam.tolist() == q[order[:3]].tolist() and not res.any()
        X0 = U.start_block(n, 4, seed=5)
        tr = []
        lam, X, res, fl, steps, rank = G.lobpcg_gen_restated(lambda r: r, A, B, X0, 2, 1e-9, 400, trace=tr)
        print(n, "steps", steps, "flags", fl.tolist())
        assert fl[:2].tolist() == [0, 0] and np.abs(lam[:2] - q[order[:2]]).max() <= 1e-9 * n
        assert steps == G.DIAGONAL_STEPS[n] and G.decisions_ok(tr, MARGIN)
        for sd in G.NOISE_SEEDS:
            o = G.lobpcg_gen_restated(lambda r: r, A, B, X0, 2, 1e-9, 400, noise=np.random.default_rng(sd))
            assert o[4] == steps and o[3].tolist() == fl.tolist(), (n, sd)


# ---- the new symbols --------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_typed():
    with open(os.path.join(ROOT, "include", "hifir_amd.h")) as f:
        header = f.read()
    lib = hifir_amd.lib()
    for name in NEW:
        assert re.search(r"HifAmdStatus\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(lib, name).restype is C.c_int
        assert list(getattr(lib, name).argtypes) == list(_lib.SIGNATURES[name][1])
    assert _lib.SIGNATURES["hifamd_set_mass_matrix"] == _lib.SIGNATURES["hifamd_set_matrix"]
    assert _lib.SIGNATURES["hifamd_lobpcg_gen"][1] == _lib.SIGNATURES["hifamd_lobpcg"][1]
    assert _lib.SIGNATURES["hifamd_lobpcg_gen_dev"][1] == _lib.SIGNATURES["hifamd_lobpcg_dev"][1]
    # the header's argument lists, word for word, are the standard driver's
    def args(name):
        return re.sub(r"\s+", " ", re.search(r"HifAmdStatus\s+%s\s*\(([^;]*)\);" % name, header).group(1))

    assert args("hifamd_lobpcg_gen") == args("hifamd_lobpcg") and args("hifamd_lobpcg_gen_dev") == args("hifamd_lobpcg_dev")
    assert args("hifamd_set_mass_matrix") == args("hifamd_set_matrix")
    for method in ("set_mass_matrix", "lobpcg_gen"):
        assert callable(getattr(hifir_amd.HIF, method))
    import inspect

    assert str(inspect.signature(hifir_amd.HIF.lobpcg_gen)) == str(inspect.signature(hifir_amd.HIF.lobpcg))
    with open(os.path.join(ROOT, "include", "hifir_amd.hpp")) as f:
        facade = f.read()
    assert "lobpcg_gen(" in facade and "hifamd_set_mass_matrix(" in facade


def test_refusals_that_need_no_gpu():
    lib = hifir_amd.lib()
    ip, ix, v = np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([1.0])
    assert lib.hifamd_set_mass_matrix(None, 1, ip.ctypes.data, ix.ctypes.data, v.ctypes.data) == 1  # HIFAMD_NULL_OBJ
    X = np.zeros((4, 2))
    for fn in (lib.hifamd_lobpcg_gen, lib.hifamd_lobpcg_gen_dev):
        assert fn(None, 2, 2, None, 0, 0, 1e-8, 1e-12, 10, 0, None, X.ctypes.data, 2, None, None, None) == 1


# ---- lob::residual_test_gen under sanitizers ---------------------------------------------------------------------------------
def test_residual_test_gen_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lobpcg_gen_small_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "hifir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "lobpcg_gen_small_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("GEN SMALL TEST OK") and "FAIL" not in out.stdout
