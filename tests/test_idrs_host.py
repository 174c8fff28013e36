"""CPU: the IDR(s) entry points (hifamd_idrs_batch / _dev, HIF.idrs, the C++ facade's idrs) are declared, exported and typed and
never return a CPU result; the restatement of idrs_util converges with true residuals within rtol, its blocked
biorthogonalization agrees with the textbook sequential one, the numpy twin of the generated shadow block is the host generator's,
the tables of idrs_util (vetted seeds, unvetted columns, sensitivities, maxit edges, exact constructions) are what this file
measures, and IDR(4) needs at least 10 % fewer steps than BiCGSTAB on pcd2d_32."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hifir_amd
import idrs_util as U
import lockstep_edges_util as L
from hifir_amd import _lib
from hifir_amd._lib import lib
from krylov_edges_util import mixed_fates
from test_bicgstab_host import _import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hifamd_idrs_batch", "hifamd_idrs_batch_dev")


def test_symbols_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "hifir_amd.h")).read()
    declared = set(re.findall(r"\b(hifamd_\w+)\s*\(", hdr))
    Lb = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"#define\s+HIFAMD_IDRS_MAX\s+8\b", hdr) and U.IDRS_MAX == 8
    C = ctypes
    for name in NAMES:
        assert name in declared, name
        assert hasattr(Lb, name), name
        # hifamd_bicgstab_batch's arguments with s, P, ldp, seed ahead of rtol
        bs = _lib.SIGNATURES[name.replace("idrs", "bicgstab")]
        assert _lib.SIGNATURES[name] == (bs[0], bs[1][:6] + [C.c_int, C.c_void_p, C.c_int64, C.c_uint64] + bs[1][6:]), name
    proto = re.search(r"hifamd_idrs_batch\(([^;]*)\);", hdr).group(1)
    assert re.sub(r"\s+", " ", proto) == ("HifAmdHdl h, const void *B, int64_t ldb, void *X, int64_t ldx, int64_t nrhs, int s, "
                                          "const void *P, int64_t ldp, uint64_t seed, double rtol, int maxit, int64_t rank, "
                                          "int *flags, int *iters")


def test_null_handle():
    fl, it = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    b, x, P = np.ones(4), np.zeros(4), np.ones((4, 2))
    for name in NAMES:
        st = getattr(lib(), name)(None, b.ctypes.data, 1, x.ctypes.data, 1, 1, 2, P.ctypes.data, 2, 0, 1e-6, 10, 0,
                                  fl.ctypes.data, it.ctypes.data)
        assert st == 1, (name, st)  # HIFAMD_NULL_OBJ


@pytest.mark.parametrize("name", ["cd2d_48", "young1c"])
def test_idrs_has_no_cpu_fallback(name):
    # (a finalized handle needs a device: the refusals behind that one are held in order by test_gpu_idrs.py)
    M, d = _import(name)
    b = np.asarray(d["b"], dtype=M.dtype)
    for kw in (dict(), dict(s=0), dict(s=9), dict(P=np.full((len(b), 4), np.nan)), dict(maxit=0)):
        with pytest.raises(hifir_amd.HifAmdError) as e:
            M.idrs(b, **kw)  # not finalized comes first, whatever else is wrong: never a CPU result
        assert e.value.code == 3  # HIFAMD_BAD_PREC
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.idrs(np.stack([b, b], axis=1), s=2, rtol=1e-8, maxit=4, seed=3)
    assert e.value.code == 3
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.idrs(b, P=np.ones((3, 4)))  # the facade's own shape check
    assert e.value.code == 2
    if lib().hifamd_device_count() == 0:
        with pytest.raises(hifir_amd.HifAmdError) as e:
            M.finalize(1)
        assert e.value.code == 4 and "no CPU fallback" in e.value.msg  # HIFAMD_HIFIR_ERROR
        with pytest.raises(hifir_amd.HifAmdError):
            M.idrs(b)


def test_cpp_facade_idrs_compiles(tmp_path):
    src = tmp_path / "idrs_facade.cpp"
    src.write_text(r'''
#include <complex>
#include <tuple>
#include <vector>
#include "hifir_amd.hpp"
template <class V>
struct MockCrs {
  std::vector<long> rs{0};
  std::vector<int> ci;
  std::vector<V> v;
  const std::vector<long>& row_start() const { return rs; }
  const std::vector<int>& col_ind() const { return ci; }
  const std::vector<V>& vals() const { return v; }
  size_t nrows() const { return 0; }
};
template <class V>
int run() {
  hifamd::HIF<V> G;
  MockCrs<V> A;
  std::vector<V> b(4);
  if (false) {
    auto out = G.idrs(A, b, 4, 1e-6, 100);
    auto out2 = G.idrs(A, b, HIFAMD_IDRS_MAX, 1e-6, 100, true, 7);
    std::vector<V> x = std::get<0>(out);
    return std::get<1>(out) + std::get<2>(out2) + (int)x.size();
  }
  return 0;
}
int main() { return run<double>() + run<std::complex<double>>(); }
''')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])
    csrc = tmp_path / "idrs_c.c"
    csrc.write_text('#include "hifir_amd.h"\nint f(HifAmdHdl h, double *v, int *i) { return (int)hifamd_idrs_batch(h, v, 1, v, 1, 1, '
                    'HIFAMD_IDRS_MAX, 0, 0, 5, 1e-6, 10, 0, i, i) + (int)hifamd_idrs_batch_dev(h, v, 1, v, 1, 1, 4, v, 4, 0, 1e-6, 10, 0, i, i); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(csrc)])


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cd2d_48", "pcd2d_32", "young1c"])
def test_restatement_converges_with_true_residuals_within_rtol(name):
    P = U.pair(name, 4)
    w = max(P.cfg["widths"])
    B, fates = P.batch(w)
    steps = []
    for c in P.vetted(w):
        b = B[:, c]
        x, fl, it, tr = P.restated(b)
        if not b.any():
            assert (fl, it) == (0, 0) and not x.any()
            continue
        assert fl == 0 and 1 <= it < U.MAXIT and len(tr["ratios"]) == it, (c, fates[c], fl, it)
        assert tr["mode"] == 3 and tr["step"] == it - 1
        assert np.linalg.norm(b - P.A @ x) / np.linalg.norm(b) <= P.rtol, (c, fates[c])
        assert {nm for nm, k, v in tr["scalars"]} == {"mkk", "tt", "tr"} and len(tr["cosines"]) == it // 5
        steps.append(it)
    print(name, "steps", sorted(set(steps)))


@pytest.mark.parametrize("key", U.ALL_CASES)
def test_blocked_and_sequential_forms_agree_on_stable_columns(key):
    P = U.pair(*key)
    name, s = key[:2]
    w = max(P.cfg["widths"])
    B, fates = P.batch(w)
    worst = 0.0
    for c in P.vetted(w):
        b = B[:, c]
        if not b.any():
            continue
        x, fl, it, _ = P.restated(b)
        xs, fs, its, _ = P.restated(b, sequential=True)
        assert (fs, its) == (fl, it), (c, fates[c], (fl, it), (fs, its))
        e = np.linalg.norm(xs - x) / np.linalg.norm(x)
        worst = max(worst, e)
        assert e <= U.tolerance(P, L.kind_of(fates[c])), (c, fates[c], e)
    print(name, s, "largest difference %.1e" % worst)


def test_forward_substitution_and_recursion_on_a_small_case():
    # s = 3, M lower triangular: the substitution from row k solves the trailing block, entries above stay zero
    rng = np.random.default_rng(1)
    M = np.tril(rng.uniform(1, 2, (3, 3)))
    f = rng.uniform(-1, 1, 3)
    for k in range(3):
        c = U._forward(M, f, k)
        assert not c[:k].any() and np.allclose(M[k:, k:] @ c[k:], f[k:], rtol=1e-14)


def test_special_columns_of_the_restatement():
    P = U.pair("cd2d_48", 2)
    n = P.A.shape[0]
    B = np.stack([np.zeros(n), np.full(n, np.nan), P.hard(0), P.hard(0) * 2.0 ** -100], axis=1)
    B[5, 1] = 1.0
    X, fl, it = U.idrs_restated(P.O, P.A, B, P.P, P.rtol, U.MAXIT)
    assert fl.tolist()[:2] == [0, 1] and it.tolist()[:2] == [0, 0] and not X[:, :2].any()
    assert fl[2] == fl[3] == 0 and it[2] == it[3] and np.array_equal(X[:, 3], X[:, 2] * 2.0 ** -100)
    # maxit: flag 2 with the iterate of that step
    X2, fl2, it2 = U.idrs_restated(P.O, P.A, B[:, 2], P.P, P.rtol, 7)
    assert (fl2[0], it2[0]) == (2, 7) and X2.any()


# ---- the generated shadow block ------------------------------------------------------------------------------------------------
def test_generated_block_twin_matches_the_host_generator(tmp_path):
    exe = str(tmp_path / "idrs_probe")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "hifir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "idrs_probe.cpp"), "-o", exe])
    for n, s, seed, cplx in ((7, 1, 0, 0), (841, 4, 5, 1), (2304, 8, 0xFFFFFFFFFFFFFFFF, 0), (33, 3, 0x123456789ABCDEF, 1)):
        out = str(tmp_path / "p.bin")
        subprocess.check_call([exe, str(n), str(s), str(seed), str(cplx), out])
        raw = np.fromfile(out, dtype=np.float64)
        want = raw[:n * s].reshape(n, s) + (1j * raw[n * s:].reshape(n, s) if cplx else 0.0)
        got = U.generated_P(n, s, seed, bool(cplx))
        assert got.dtype == want.dtype and np.array_equal(got, want), (n, s, seed, cplx)
        assert np.abs(got.real).max() <= 1.0 and (n * s < 100 or np.abs(got.real).max() > 0.9)
    # the first s columns of the block the null-space search draws
    from test_nsp_find_host import _probe_numpy

    assert np.array_equal(U.generated_P(50, 8, 9, True), _probe_numpy(50, 9, True)[:, :8])


# ---- the tables -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", U.ALL_CASES)
def test_vetted_seeds_and_unvetted_columns_are_the_measured_ones(key):
    P = U.pair(*key)
    need = max(sum(1 for c, f in enumerate(mixed_fates(w)) if f == "hard" and c > 0) for w in P.cfg["widths"])
    skipped = U.SKIP_SEEDS.get(key, ())
    used = P.seeds[:need]
    assert all(P.stable(P.hard(j)) for j in range(need))
    assert all(sd < used[-1] for sd in skipped), "a skipped seed beyond the ones in use"
    for sd in skipped:  # every skipped seed is really unstable
        rng = np.random.default_rng(sd)
        v = rng.uniform(-1, 1, P.A.shape[0])
        assert not P.stable(v + 1j * rng.uniform(-1, 1, P.A.shape[0]) if P.cplx else v), sd
    for w in P.cfg["widths"]:
        B, fates = P.batch(w)
        assert fates == mixed_fates(w)
        bad = tuple(c for c in range(w) if B[:, c].any() and not P.stable(B[:, c]))
        assert bad == U.UNVETTED.get(key, {}).get(w, ()), (w, bad)
        vet = P.vetted(w)
        assert all(c in vet for c, f in enumerate(fates) if f in ("hard", "tiny", "zero")), w
        assert len(vet) >= w // 3
        for c in vet:  # the 2^-100 / 2^+100 copies: same fate, x scaled exactly
            f = fates[c]
            if f in L.SCALED_COPY_OF and fates.index(L.SCALED_COPY_OF[f]) in vet:
                x, fl, it, _ = P.restated(B[:, c])
                xo, flo, ito, _ = P.restated(B[:, fates.index(L.SCALED_COPY_OF[f])])
                assert (fl, it) == (flo, ito) and np.array_equal(x, xo * (2.0 ** -100 if f == "tiny" else 2.0 ** 100))


@pytest.mark.parametrize("key", U.ALL_CASES)
def test_sens_is_the_measured_table(key):
    P = U.pair(*key)
    got = {k: U.round_up(v) for k, v in U.measured_sensitivities(P).items()}
    print(key, got)
    assert got == U.SENS[key]
    for kind in got:
        assert 1e-12 <= U.tolerance(P, kind) <= 1e-6, kind


def test_round_up():
    assert U.round_up(1.234e-11) == 1.3e-11 and U.round_up(1.2e-11) == 1.2e-11 and U.round_up(9.91e-16) == 1e-15
    assert U.round_up(0.0) == 0.0


def test_maxit_edges_need_m_minus_1_m_and_m_plus_1():
    kinds = set()
    for name, s, m, spec in U.MAXIT_EDGES:
        P = U.pair(name, s)
        B = U.maxit_columns(P, spec)
        assert [P.restated(B[:, c])[1:3] for c in range(3)] == [(0, m - 1), (0, m), (0, m + 1)]
        assert [P.restated(B[:, c], maxit=m)[1:3] for c in range(3)] == [(0, m - 1), (0, m), (2, m)]
        assert all(P.stable(B[:, c], maxit=m) and P.stable(B[:, c]) for c in range(3))
        kinds |= {"omega" if k % (s + 1) == 0 else "inside" for k in (m - 1, m)}
    assert kinds == {"omega", "inside"}


def test_exact_constructions():
    E = U.exact_case()
    A = E["A"]
    for nm, (b, P, exp, updates) in E["cases"].items():
        tr = []
        X, fl, it = U.idrs_restated(lambda r: r, A, b, P, 1e-10, 50, trace=tr)
        assert (int(fl[0]), int(it[0])) == exp, (nm, fl, it)
        assert np.array_equal(P, np.round(P)) and np.array_equal(b, np.round(b)) and not X[b == 0].any()
        assert bool(X.any()) == (updates > 0), nm
        # a power-of-two scale of b changes nothing but the scale
        Xs, fls, its = U.idrs_restated(lambda r: r, A, b * 2.0 ** -9, P, 1e-10, 50)
        assert (int(fls[0]), int(its[0])) == exp and np.array_equal(Xs, X * 2.0 ** -9)
        t = tr[0]
        if nm == "half":
            assert np.array_equal(X[:, 0], b / 2) and t["ratios"] == [0.0] and (t["mode"], t["step"]) == (3, 0)
        elif nm == "skew":
            assert np.array_equal(X[4:6, 0], [1.0, 1.0]) and (t["mode"], t["step"]) == (4, 1) and t["scalars"][-1][2] == 0
        else:
            j = int(nm[-1])
            assert (t["mode"], t["step"]) == (2, j) and t["scalars"][-1][2] == 0
            assert all(abs(v) >= 0.05 for _, _, v in t["scalars"][:-1]) and all(v > 1e-3 for v in t["ratios"])


# ---- the reason for the solver ----------------------------------------------------------------------------------------------------
def test_idr4_needs_fewer_steps_than_bicgstab_on_pcd2d_32():
    P = U.pair("pcd2d_32", 4)
    B, fates = P.batch(65)
    cols = [c for c in P.vetted(65) if B[:, c].any()]
    idr = [P.restated(B[:, c])[2] for c in cols]
    Xb, flb, itb = L.bicgstab_restated(P.O, P.A, B[:, cols], P.rtol, U.MAXIT)
    assert not flb.any()
    print("pcd2d_32: mean steps IDR(4) %.1f, BiCGSTAB %.1f" % (np.mean(idr), itb.mean()))
    assert np.mean(idr) <= 0.9 * itb.mean()
