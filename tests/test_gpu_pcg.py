"""GPU (-m gpu): the batched preconditioned CG driver (hifamd_pcg_batch / HIF.pcg) against a numpy restatement of the
same recursion around the oracle's apply (orc.Oracle.solve as M^{-1}), its batch-width independence, a Hermitian
complex hierarchy made from a real one by a diagonal unitary similarity, its flags and refusals, and the 1M-row
is_symm Poisson hierarchy where the compiled reference travelled."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp

import hifir_amd
from lockstep_edges_util import pcg_restated
from oracle import orc, ref
from util import load_hier, poisson2d, relerr

pytestmark = pytest.mark.gpu


def _matrix(d):
    n = len(d["b"])
    return sp.csr_matrix((d["A_vals"], d["A_indices"], d["A_indptr"]), shape=(n, n))


@pytest.fixture(scope="module")
def p32():
    levels, d = load_hier("p2d_32_symm")
    M = hifir_amd.HIF.from_levels(levels, max_nrhs=64)
    M.set_matrix(d["A_indptr"], d["A_indices"], d["A_vals"])
    assert M.is_hermitian()
    return levels, d, M, orc.Oracle(levels), _matrix(d)


def _columns(d, A):
    n = len(d["b"])
    rng = np.random.default_rng(5)
    return np.stack([rng.uniform(-1, 1, n), np.zeros(n), d["b"], A @ np.ones(n), 1e-30 * rng.uniform(-1, 1, n)], axis=1)


def _check_vs_restated(X, fl, it, Xo, fo, io, A, B, rtol):
    assert fl.tolist() == fo.tolist() and it.tolist() == io.tolist(), (fl, fo, it, io)
    for c in range(B.shape[1]):
        if not np.any(B[:, c]):
            assert it[c] == 0 and fl[c] == 0 and not np.any(X[:, c])
            continue
        assert relerr(X[:, c], Xo[:, c]) <= 1e-8, c
        if fl[c] == 0:
            assert np.linalg.norm(A @ X[:, c] - B[:, c]) / np.linalg.norm(B[:, c]) <= 10 * rtol


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
def test_pcg_vs_restatement(p32, rtol):
    levels, d, M, O, A = p32
    x, flag, it = M.pcg(d["b"], rtol=rtol, maxit=300)
    xo, fo, io = pcg_restated(O, A, d["b"], rtol, 300)
    assert (flag, it) == (int(fo[0]), int(io[0]))
    assert flag == 0 and it > 1
    assert relerr(x, xo[:, 0]) <= 1e-8
    assert np.linalg.norm(A @ x - d["b"]) / np.linalg.norm(d["b"]) <= 10 * rtol
    B = _columns(d, A)
    X, fl, it = M.pcg(B, rtol=rtol, maxit=300)
    Xo, fo, io = pcg_restated(O, A, B, rtol, 300)
    _check_vs_restated(X, fl, it, Xo, fo, io, A, B, rtol)
    assert fl.tolist() == [0] * 5 and it[1] == 0


def test_column_bits_do_not_depend_on_the_batch(p32):
    import torch

    levels, d, M, O, A = p32
    n = len(d["b"])
    rng = np.random.default_rng(17)
    B = rng.uniform(-1, 1, size=(n, 70))
    B[:, 9] = 0.0
    X70, f70, i70 = M.pcg(B, rtol=1e-9, maxit=300)
    X64, f64, i64 = M.pcg(np.ascontiguousarray(B[:, :64]), rtol=1e-9, maxit=300)
    X5, f5, i5 = M.pcg(np.ascontiguousarray(B[:, :5]), rtol=1e-9, maxit=300)
    assert np.array_equal(X64, X70[:, :64]) and np.array_equal(f64, f70[:64]) and np.array_equal(i64, i70[:64])
    assert np.array_equal(X5, X70[:, :5]) and np.array_equal(i5, i70[:5])
    for k in (0, 3, 9, 63, 64, 69):
        x, f, i = M.pcg(B[:, k].copy(), rtol=1e-9, maxit=300)
        assert np.array_equal(x, X70[:, k]) and (f, i) == (f70[k], i70[k]), k
    assert f70.tolist() == [0] * 70 and i70[9] == 0
    # the torch-device entry gives the host entry's bits
    Xd, fd, idv = M.pcg(torch.from_numpy(np.ascontiguousarray(B[:, :5])).cuda(), rtol=1e-9, maxit=300)
    assert np.array_equal(Xd.cpu().numpy(), X5) and np.array_equal(fd, f5) and np.array_equal(idv, i5)
    xd, f, i = M.pcg(torch.from_numpy(B[:, 3].copy()).cuda(), rtol=1e-9, maxit=300)
    assert np.array_equal(xd.cpu().numpy(), X70[:, 3]) and (f, i) == (f70[3], i70[3])


def _phase_similarity(levels, A, seed=3):
    """A Hermitian complex hierarchy (and matrix) from a real is_symm one by a diagonal unitary similarity Phi: per level
    the phases follow p (phi_p = phi[p]; B block phi_1 = phi_p[:m], Schur block phi_2 = phi_p[m:], the next level's
    phases), L' = Phi_1 L Phi_1^H, U' = L'^H, E' = Phi_2 E Phi_1^H, F' = E'^H, d, s, t, p, q unchanged, dense
    Phi D Phi^H; A' = Phi A Phi^H.  Then M'^{-1} = Phi M^{-1} Phi^H."""
    n = A.shape[0]
    phi = np.exp(1j * np.random.default_rng(seed).uniform(0, 2 * np.pi, n))
    out, ph = [], phi
    for lv in levels:
        m, nl = int(lv["m"]), int(lv["n"])
        pp = ph[np.asarray(lv["p"])]
        f1, f2 = pp[:m], pp[m:]
        c = copy.deepcopy(lv)
        L = sp.csc_matrix((lv["L_vals"], lv["L_rowind"], lv["L_colptr"]), shape=(m, m))
        E = sp.csc_matrix((lv["E_vals"], lv["E_rowind"], lv["E_colptr"]), shape=(nl - m, m))
        L2 = sp.csc_matrix(sp.diags(f1) @ L @ sp.diags(f1.conj()))
        E2 = sp.csc_matrix(sp.diags(f2) @ E @ sp.diags(f1.conj()))
        for name, X in (("L", L2), ("U", L2.conj().T), ("E", E2), ("F", E2.conj().T if nl > m else None)):
            if X is None:
                continue
            X = sp.csc_matrix(X)
            X.sort_indices()
            c[name + "_colptr"] = X.indptr.astype(np.int64)
            c[name + "_rowind"] = X.indices.astype(np.int32)
            c[name + "_vals"] = X.data.astype(np.complex128)
        c["d"] = np.asarray(lv["d"]).astype(np.complex128)
        ph = f2
        out.append(c)
    last = out[-1]
    if int(last.get("dense_n", 0)) > 0:
        nd = int(last["dense_n"])
        D = np.asarray(levels[-1]["dense"]).reshape(nd, nd, order="F")
        last["dense"] = (ph[:, None] * D * ph.conj()[None, :]).ravel(order="F")
    A2 = sp.csr_matrix(sp.diags(phi) @ A.astype(np.complex128) @ sp.diags(phi.conj()))
    A2.sort_indices()
    return out, A2, phi


def test_complex_hermitian_hierarchy(p32):
    levels, d, M, O, A = p32
    lz, Az, phi = _phase_similarity(levels, A)
    Mz = hifir_amd.HIF.from_levels(lz, max_nrhs=8)
    assert Mz.is_hermitian()
    Mz.set_matrix(Az.indptr, Az.indices, Az.data)
    rng = np.random.default_rng(23)
    B = np.stack([d["b"], rng.uniform(-1, 1, len(d["b"]))], axis=1)
    X, fl, it = M.pcg(B, rtol=1e-10, maxit=300)
    Xz, flz, itz = Mz.pcg(phi[:, None] * B, rtol=1e-10, maxit=300)
    assert flz.tolist() == fl.tolist() == [0, 0] and itz.tolist() == it.tolist()
    for c in range(2):
        assert np.linalg.norm(Xz[:, c] - phi * X[:, c]) / np.linalg.norm(X[:, c]) <= 1e-10
    Bz = np.stack([phi * d["b"], rng.uniform(-1, 1, len(d["b"])) + 1j * rng.uniform(-1, 1, len(d["b"])),
                   np.zeros(len(d["b"]), dtype=np.complex128)], axis=1)
    Xz, flz, itz = Mz.pcg(Bz, rtol=1e-10, maxit=300)
    Xo, fo, io = pcg_restated(orc.Oracle(lz), Az, Bz, 1e-10, 300)
    _check_vs_restated(Xz, flz, itz, Xo, fo, io, Az, Bz, 1e-10)


def test_flags_and_refusals(p32):
    levels, d, M, O, A = p32
    b = d["b"]
    # maxit reached
    x, flag, it = M.pcg(b, rtol=1e-14, maxit=3)
    xo, fo, io = pcg_restated(O, A, b, 1e-14, 3)
    assert (flag, it) == (2, 3) == (int(fo[0]), int(io[0])) and relerr(x, xo[:, 0]) <= 1e-8
    # (-A, M): not positive definite, breakdown at the first curvature
    Mn = hifir_amd.HIF.from_levels(levels, max_nrhs=4)
    Mn.set_matrix(d["A_indptr"], d["A_indices"], -d["A_vals"])
    X, fl, it = Mn.pcg(np.stack([b, np.zeros_like(b)], axis=1), rtol=1e-8, maxit=50)
    assert fl.tolist() == [1, 0] and it.tolist() == [0, 0]
    # arguments
    for kw in ({"rtol": 0.0}, {"rtol": -1.0}, {"maxit": 0}):
        with pytest.raises(hifir_amd.HifAmdError) as e:
            M.pcg(b, **kw)
        assert e.value.code == 2
    # no matrix
    M0 = hifir_amd.HIF.from_levels(levels, max_nrhs=4)
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M0.pcg(b)
    assert e.value.code == 3 and "hifamd_set_matrix" in e.value.msg
    # a null-space filter on the solve is out of scope
    M0.set_matrix(d["A_indptr"], d["A_indices"], d["A_vals"])
    M0.set_nsp_const(0, -1)
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M0.pcg(b)
    assert e.value.code == 3 and "null-space" in e.value.msg
    # not Hermitian: the QRCP last level of p2d_30 (its sparse level is mirrored bit for bit)
    l30, d30 = load_hier("p2d_30")
    M30 = hifir_amd.HIF.from_levels(l30, max_nrhs=4)
    M30.set_matrix(d30["A_indptr"], d30["A_indices"], d30["A_vals"])
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M30.pcg(d30["b"])
    assert e.value.code == 3 and "level 1" in e.value.msg and "dense" in e.value.msg and "is_symm" in e.value.msg


@pytest.mark.skipif(not ref.available(), reason="compiled reference not present")
def test_1m_symmetric_factorization_pcg():
    """The 1000^2 Poisson matrix factorized with is_symm by the compiled reference: 8 columns to rtol 1e-8."""
    A = poisson2d(1000)
    R = ref.RefHIF(A.indptr, A.indices, A.data, ref.make_params(is_symm=1))
    levels = R.levels()
    M = hifir_amd.HIF.from_levels(levels, max_nrhs=8)
    assert M.is_hermitian()
    M.set_matrix(A.indptr, A.indices, A.data)
    n = A.shape[0]
    B = np.random.default_rng(29).uniform(-1, 1, size=(n, 8))
    X, fl, it = M.pcg(B, rtol=1e-8, maxit=1000)
    assert fl.tolist() == [0] * 8, (fl, it)
    res = np.linalg.norm(A @ X - B, axis=0) / np.linalg.norm(B, axis=0)
    assert res.max() <= 1e-7, res
