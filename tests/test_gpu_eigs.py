"""GPU (-m gpu): the B-orthogonal projector (hifamd_eig_project / HIF.b_project) and the locked LOBPCG sweeps (hifamd_eigs /
HIF.eigsh) against their numpy restatements (eigs_util; test_eigs_host.py pins every input used here on the CPU):
1 the projector alone at its tile, row and stride edges; 2 exact constructions on a diagonal hierarchy; 3 no disturbance:
one unconstrained sweep returns lobpcg's / lobpcg_gen's bits; 4 the case table against the restatement and the dense
spectrum; 5 locking against an earlier call's eigenvectors; 6 edges and refusals."""
import os
import subprocess

import numpy as np
import pytest

import eigs_util as E
import hifir_amd
import lobpcg_gen_util as G
import lobpcg_util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NS = (1, 15, 16, 17, 37, 63, 64, 65, 101, 976, 1024, 1025)
MS = (1, 15, 16, 17, 63, 64, 65, 127, 128)
KWS = (1, 5, 16)
# every n with two m, every m with at least two n, kw in turn
PAIRS = [(n, MS[(i + 4 * j) % 9], KWS[(i + j) % 3]) for i, n in enumerate(NS) for j in range(2)]

_HANDLES = {}


def _diag_handle(n, cplx=False, mass=None):
    """M^{-1} = I on n rows, the diagonal matrix of lobpcg_util.diagonal_case, optionally a mass matrix"""
    key = (n, cplx, mass)
    if key not in _HANDLES:
        levels, A, a = U.diagonal_case(n)
        dt = np.complex128 if cplx else np.float64
        M = hifir_amd.HIF.from_levels(levels, max_nrhs=16, dtype=dt)
        M.set_matrix(A.indptr, A.indices, A.data.astype(dt))
        B = None
        if mass == "diagonal":
            B = G.diagonal_mass(n)[0]
        elif mass == "mass2d":
            B = G.mass2d(int(round(np.sqrt(n))))
        if B is not None:
            M.set_mass_matrix(B.indptr, B.indices, B.data.astype(dt))
        _HANDLES[key] = (M, A, a, B)
    return _HANDLES[key]


def _fixture_handle(fixture, gen):
    key = (fixture, gen)
    if key not in _HANDLES:
        Cs = U.case(fixture)
        M = hifir_amd.HIF.from_levels(Cs.levels, max_nrhs=64)
        M.set_matrix(Cs.A.indptr, Cs.A.indices, Cs.A.data)
        if gen:
            B = G.mass_of(fixture)
            M.set_mass_matrix(B.indptr, B.indices, B.data)
        _HANDLES[key] = M
    return _HANDLES[key]


def _rand(rng, n, c, cplx):
    X = rng.uniform(-1, 1, (n, c))
    return X + 1j * rng.uniform(-1, 1, (n, c)) if cplx else X


def _orthonormal(rng, n, m, cplx, B=None):
    """m B-orthonormal columns where n allows it (Cholesky of the Gram), else a block of norm about one"""
    Z = _rand(rng, n, m, cplx)
    if m > n:
        return Z / np.sqrt(n * m)
    Gm = Z.conj().T @ (Z if B is None else B @ Z)
    return Z @ np.linalg.inv(np.linalg.cholesky(Gm).conj().T)


# ---- 1. the projector alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n,m,kw", PAIRS)
def test_projector_against_its_restatement(n, m, kw, cplx):
    M, A, a, _ = _diag_handle(n, cplx)
    rng = np.random.default_rng(1000 * n + m)
    Y, W = _orthonormal(rng, n, m, cplx), _rand(rng, n, kw, cplx)
    out = M.b_project(W.copy(), Y)
    ref = E.project_restated(W, Y)
    err = np.linalg.norm(out - ref) / np.linalg.norm(W)
    print(n, m, kw, cplx, "error / ||W||", err)
    assert err <= 1e-12
    assert np.array_equal(M.b_project(W.copy(), Y), out)  # the same bits on a second call


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("m,kw", [(17, 5), (128, 16)])
def test_projector_past_the_first_pass_of_its_row_loops(m, kw, cplx):
    """256 workgroups of 4 waves: k_eig_cgram's two row groups in flight cover rows 0 .. 4095 and 4096 .. 8191 in the first
    turn of its loop, k_eig_cproj's strips 16384 rows.  n = 20011 (no multiple of 4 or 16) runs the second in-flight group on
    rows inside n, a second and a third turn of the Gram loop, and a second, partial turn of the strip loop."""
    n = 20011
    M, A, a, _ = _diag_handle(n, cplx)
    rng = np.random.default_rng(n + m)
    Y, W = _orthonormal(rng, n, m, cplx), _rand(rng, n, kw, cplx)
    out = M.b_project(W.copy(), Y)
    ref = E.project_restated(W, Y)
    err = np.linalg.norm(out - ref) / np.linalg.norm(W)
    rows = np.abs(out - ref).max(axis=1)
    print(n, m, kw, cplx, "error / ||W||", err, "worst row", int(rows.argmax()))
    assert err <= 1e-12 and rows[4096:].max() <= 1e-12 and np.abs(Y.conj().T @ out).max() <= 1e-12 * np.sqrt(n)
    assert np.array_equal(M.b_project(W.copy(), Y), out)


def test_every_m_has_two_n_and_every_n_two_m():
    assert all(len({m for n2, m, _ in PAIRS if n2 == n}) == 2 for n in NS)
    assert all(len({n for n, m2, _ in PAIRS if m2 == m}) >= 2 for m in MS) and {kw for _, _, kw in PAIRS} == set(KWS)


@pytest.mark.parametrize("cplx", [False, True])
def test_projector_strided_blocks_nan_and_zero_columns(cplx):
    import torch

    n, m, kw = 101, 65, 5
    M, A, a, _ = _diag_handle(n, cplx)
    rng = np.random.default_rng(5)
    Y, W = _orthonormal(rng, n, m, cplx), _rand(rng, n, kw, cplx)
    ref = M.b_project(W.copy(), Y)
    dt = torch.complex128 if cplx else torch.float64
    wide = torch.full((n, 48), 7.25, dtype=dt, device="cuda")  # W at column 16 of a block of leading dimension 48
    wide[:, 16:16 + kw] = torch.from_numpy(W).cuda()
    ywide = torch.full((n, m + 7), -3.5, dtype=dt, device="cuda")
    ywide[:, 3:3 + m] = torch.from_numpy(Y).cuda()
    view = wide[:, 16:16 + kw]
    assert M.b_project(view, ywide[:, 3:3 + m]) is view
    torch.cuda.synchronize()
    o, yo = wide.cpu().numpy(), ywide.cpu().numpy()
    assert np.array_equal(o[:, 16:16 + kw], ref) and (o[:, :16] == 7.25).all() and (o[:, 16 + kw:] == 7.25).all()
    assert np.array_equal(yo[:, 3:3 + m], Y) and (yo[:, :3] == -3.5).all() and (yo[:, 3 + m:] == -3.5).all()
    # a NaN in one column stays in that column; exact zero columns keep their bits
    Wn = W.copy()
    Wn[7, 1] = np.nan
    Wn[:, 3] = 0.0
    out = M.b_project(Wn.copy(), Y)
    assert np.isnan(out[:, 1]).all()  # (C[:, 1] is NaN, and Y has no zero row)
    assert np.array_equal(out[:, [0, 2, 4]], ref[:, [0, 2, 4]])
    assert np.array_equal(np.ascontiguousarray(out[:, 3]).view(np.uint64), np.zeros(n * (2 if cplx else 1), dtype=np.uint64))


@pytest.mark.parametrize("n,mass,m,kw", [(101, "diagonal", 17, 5), (1024, "mass2d", 65, 16), (1024, "mass2d", 128, 1)])
def test_projector_under_a_mass_matrix(n, mass, m, kw):
    M, A, a, B = _diag_handle(n, False, mass)
    rng = np.random.default_rng(n + m)
    Y, W = _orthonormal(rng, n, m, False, B), _rand(rng, n, kw, False)
    out = M.b_project(W.copy(), Y, gen=True)
    err = np.linalg.norm(out - E.project_restated(W, Y, B)) / np.linalg.norm(W)
    print(n, mass, m, kw, "error / ||W||", err, "|(BY)^H out|", np.abs((B @ Y).T @ out).max())
    assert err <= 1e-12 and np.array_equal(M.b_project(W.copy(), Y, gen=True), out)
    assert np.abs((B @ Y).T @ out).max() <= 1e-12 * np.sqrt(n)


# ---- 2. exact construction -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", [False, True])
def test_exact_construction_on_a_diagonal_hierarchy(gen):
    n = 101
    M, A, a, B = _diag_handle(n, False, "diagonal" if gen else None)
    b = B.diagonal() if gen else np.ones(n)
    q = a / b
    order = np.argsort(q, kind="stable")
    rows = order[:20]
    Y = np.eye(n)[:, rows] / np.sqrt(b[rows])[None, :]  # (powers of two: exact)
    W = _rand(np.random.default_rng(9), n, 5, False)
    out = M.b_project(W.copy(), Y, gen=gen)
    keep = np.setdiff1d(np.arange(n), rows)
    assert not out[rows].any() and np.array_equal(out[keep], W[keep])
    lam, X, res, fl, info = M.eigsh(8, k=8, guard=2, gen=gen, Y=Y, tol=1e-9, maxit=400)
    print(gen, "sweeps", M.last_eigsh_sweeps, "lam", lam)
    assert fl.tolist() == [0] * 8 and np.abs(lam - q[order[20:28]]).max() <= 1e-9 * n and not X[rows].any()
    if not gen:
        assert np.abs(lam - np.arange(21.0, 29.0)).max() <= 1e-9 * n
    ref = E.eigs_restated(lambda r: r, A, B if gen else None, 8, 8, 2, 1e-9, maxit=400, Y=Y)
    assert [s[:2] for s in M.last_eigsh_sweeps] == [s[:2] for s in ref[4]]


# ---- 3. no disturbance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", [False, True])
@pytest.mark.parametrize("name", ["p32_k15", "p32_k16", "p32z_k5"])
def test_one_unconstrained_sweep_returns_lobpcgs_bits(name, gen):
    if gen:
        Cs, solve, B, X0, k, nev, tol = G.inputs(name)
    else:
        Cs, solve, X0, k, nev, tol, Q = U.inputs(name)
    M = _fixture_handle(Cs.name, gen)
    lam0, X0o, res0, fl0, steps0 = (M.lobpcg_gen if gen else M.lobpcg)(X0=X0, nev=nev, tol=tol, maxit=U.MAXIT)
    lam, X, res, fl, info = M.eigsh(nev, k=k, guard=k - nev, gen=gen, X0=X0, tol=tol, maxit=U.MAXIT)
    assert fl0[:nev].tolist() == [0] * nev and M.last_eigsh_sweeps == [(nev, nev, steps0)]
    assert np.array_equal(lam, lam0[:nev]) and np.array_equal(X, X0o[:, :nev]) and np.array_equal(res, res0[:nev])
    assert np.array_equal(fl, fl0[:nev]) and info.tolist()[:3] == [steps0, 1, nev]


# ---- 4. the table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in E.CASES])
def test_the_table_against_the_restatement_and_the_dense_spectrum(name):
    Cs, B, Y, row, (lo, Xo, ro, fo, so, rank_o), tr = E.reference(name)
    _, fixture, gen, nev, k, guard, tol, seed, want, spread = row
    M = _fixture_handle(fixture, gen)
    lam, X, res, fl, info = M.eigsh(nev, k=k, guard=guard, gen=gen, Y=Y, seed=seed, tol=tol, maxit=U.MAXIT)
    sweeps = M.last_eigsh_sweeps
    eig = E.dense_spectrum(name)
    true = E.true_residuals(Cs, B, lam, X)
    Z = X if Y is None else np.hstack([Y, X])
    orth = np.linalg.norm(Z.conj().T @ (Z if B is None else B @ Z) - np.eye(Z.shape[1]))
    defect, bound = E.subspace_defect(name, lam, X)
    print(name, "sweeps", sweeps, "restated", so, "info", info.tolist())
    print("  |lam - dense| / ||A||", np.abs(lam - eig[:nev]).max() / Cs.anorm, "true res", true.max(), "|true - res|",
          np.abs(true - res).max(), "orthogonality", orth, "bound", E.ORTH_BOUND, "subspace defect", defect, "bound", bound)
    assert fl.tolist() == [0] * nev
    assert np.abs(lam - eig[:nev]).max() <= tol * Cs.anorm
    assert (true <= tol * (1.0 + E.DRIFT / tol)).all()
    assert orth <= E.ORTH_BOUND
    assert (np.diff(lam) >= -tol * Cs.anorm).all()
    assert defect <= bound + 1e-12
    assert [s[:2] for s in sweeps] == [s[:2] for s in so] and len(sweeps) == len(want)
    assert all(abs(s[2] - r[2]) <= spread for s, r in zip(sweeps, so)), (sweeps, so, spread)
    assert info.tolist()[:3] == [sum(s[2] for s in sweeps), len(sweeps), nev] and k <= info[3] <= 3 * k


# ---- 5. locking against an earlier call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", [False, True])
def test_locking_against_an_earlier_calls_eigenvectors(gen):
    import torch

    Cs = U.case("p2d_32_symm")
    M = _fixture_handle("p2d_32_symm", gen)
    B = G.mass_of("p2d_32_symm") if gen else None
    eig = G.pencil_eigenvalues("p2d_32_symm") if gen else Cs.eig
    X0 = U.start_block(Cs.n, 8, seed=83)
    lam0, X0o, res0, fl0, steps0 = (M.lobpcg_gen if gen else M.lobpcg)(X0=X0, nev=6, tol=1e-8, maxit=U.MAXIT)
    assert fl0[:6].tolist() == [0] * 6
    Y = np.ascontiguousarray(X0o[:, :6])
    lam, X, res, fl, info = M.eigsh(6, k=8, gen=gen, Y=Y, tol=1e-8)
    print(gen, "sweeps", M.last_eigsh_sweeps, "lam", lam)
    assert fl.tolist() == [0] * 6 and np.abs(lam - eig[6:12]).max() <= 1e-8 * Cs.anorm
    BX = X if B is None else B @ X
    assert np.abs(Y.T @ BX).max() <= E.ORTH_BOUND and np.linalg.norm(X.T @ BX - np.eye(6)) <= E.ORTH_BOUND
    dev = M.eigsh(6, k=8, gen=gen, Y=torch.from_numpy(Y).cuda(), tol=1e-8)
    assert dev[1].is_cuda and np.array_equal(dev[1].cpu().numpy(), X)
    assert all(np.array_equal(a, b) for a, b in zip((lam, res, fl, info), (dev[0], dev[2], dev[3], dev[4])))


# ---- 6. edges and refusals -------------------------------------------------------------------------------------------------------
def test_one_candidate_and_a_last_sweep_of_one_column():
    Cs = U.case("p2d_32_symm")
    M = _fixture_handle("p2d_32_symm", False)
    lam, X, res, fl, info = M.eigsh(1, k=1, tol=1e-8)
    assert fl.tolist() == [0] and abs(lam[0] - Cs.eig[0]) <= 1e-8 * Cs.anorm and M.last_eigsh_sweeps[0][:2] == (1, 1)
    ref = E.eigs_restated(Cs.O, Cs.A, None, 1, 1, 0, 1e-8)
    assert M.last_eigsh_sweeps == ref[4]
    lam, X, res, fl, info = M.eigsh(7, k=8, guard=2, tol=1e-8)
    assert fl.tolist() == [0] * 7 and [s[:2] for s in M.last_eigsh_sweeps] == [(6, 6), (1, 1)]
    assert np.abs(lam - Cs.eig[:7]).max() <= 1e-8 * Cs.anorm and np.linalg.norm(X.T @ X - np.eye(7)) <= E.ORTH_BOUND


def test_a_sweep_stopped_by_maxit_with_a_partial_prefix_goes_on():
    """maxit = 12 per sweep, nev = 12, k = 8, guard = 2, seed 0 (restated: (6, 6, 10), (6, 4, 12), (2, 2, 2), every decision
    with its margin)"""
    Cs = U.case("p2d_32_symm")
    M = _fixture_handle("p2d_32_symm", False)
    tr = []
    ref = E.eigs_restated(Cs.O, Cs.A, None, 12, 8, 2, 1e-8, maxit=12, traces=tr)
    assert ref[4] == [(6, 6, 10), (6, 4, 12), (2, 2, 2)] and all(E.decisions_ok(t) for t in tr)
    lam, X, res, fl, info = M.eigsh(12, k=8, guard=2, tol=1e-8, maxit=12)
    assert M.last_eigsh_sweeps == ref[4] and fl.tolist() == [0] * 12 and info.tolist()[:3] == [24, 3, 12]
    assert np.abs(lam - Cs.eig[:12]).max() <= 1e-8 * Cs.anorm and np.linalg.norm(X.T @ X - np.eye(12)) <= E.ORTH_BOUND


def test_a_sweep_that_locks_nothing_ends_the_run_and_keeps_what_is_locked():
    """a start block 1e-7 off the first eight eigenvectors and maxit = 2 (restated: (6, 6, 1), (6, 2, 2), (4, 0, 2))"""
    Cs = U.case("p2d_32_symm")
    M = _fixture_handle("p2d_32_symm", False)
    w, V = np.linalg.eigh(Cs.A.toarray())
    X0 = V[:, :8] + 1e-7 * U.start_block(Cs.n, 8, seed=7)
    tr = []
    ref = E.eigs_restated(Cs.O, Cs.A, None, 12, 8, 2, 1e-8, maxit=2, X0=X0, traces=tr)
    assert ref[4] == [(6, 6, 1), (6, 2, 2), (4, 0, 2)] and all(E.decisions_ok(t) for t in tr)
    lam, X, res, fl, info = M.eigsh(12, k=8, guard=2, X0=X0, tol=1e-8, maxit=2)
    assert M.last_eigsh_sweeps == ref[4] and fl.tolist() == [0] * 8 + [2] * 4 == ref[3].tolist()
    assert info.tolist()[:3] == [5, 3, 8]
    assert np.abs(lam[:8] - Cs.eig[:8]).max() <= 1e-8 * Cs.anorm and np.isfinite(lam).all() and (res[8:] > 1e-8).all()
    assert np.linalg.norm(X[:, :8].T @ X[:, :8] - np.eye(8)) <= E.ORTH_BOUND
    # fewer columns asked for than wanted: what was never reached is zero, NaN, flag 2
    lam, X, res, fl, info = M.eigsh(20, k=8, guard=2, X0=X0, tol=1e-8, maxit=2)
    assert fl.tolist() == [0] * 8 + [2] * 12 and np.isnan(lam[14:]).all() and np.isnan(res[14:]).all() and not X[:, 14:].any()
    assert np.isfinite(lam[:14]).all() and X[:, 8:14].any()


def test_128_locked_vectors_with_96_from_the_caller():
    Cs = U.case("p2d_32_symm")
    M = _fixture_handle("p2d_32_symm", False)
    w, V = np.linalg.eigh(Cs.A.toarray())
    Y = np.ascontiguousarray(V[:, :96])
    lam, X, res, fl, info = M.eigsh(32, k=16, guard=4, Y=Y, tol=1e-8)
    print("sweeps", M.last_eigsh_sweeps, "info", info.tolist())
    assert fl.tolist() == [0] * 32 and [s[:2] for s in M.last_eigsh_sweeps] == [(12, 12), (12, 12), (8, 8)]
    assert np.abs(lam - w[96:128]).max() <= 1e-8 * Cs.anorm
    Z = np.hstack([Y, X])
    assert np.linalg.norm(Z.T @ Z - np.eye(128)) <= E.ORTH_BOUND * 128 / 41  # (the bound's figure is of 41 columns)


def test_refusals_with_status_and_message():
    Cs = U.case("p2d_32_symm")
    M = _fixture_handle("p2d_32_symm", False)
    w, V = np.linalg.eigh(Cs.A.toarray())

    def refused(code, word, handle=M, nev=6, **kw):
        with pytest.raises(hifir_amd.HifAmdError) as e:
            handle.eigsh(nev, **kw)
        assert e.value.code == code and word in e.value.msg, (kw, e.value.code, e.value.msg)

    refused(2, "m0 + nev <= 128", nev=33, Y=V[:, :96])   # 129
    refused(2, "m0 + nev <= 128", nev=129)
    refused(2, "1 <= k <= 16", k=17)
    refused(2, "0 <= guard < k", k=8, guard=8)
    refused(2, "tol > 0", tol=0.0)                         # (lobpcg's own argument checks, in their order, come first)
    refused(2, "1 <= k <= 16", k=17, guard=17, nev=200)
    Yb = V[:, :4].copy()
    Yb[:, 1] += 1e-6 * V[:, 0]                             # ||Y^H Y - I|| = 1e-6
    refused(3, "not B-orthonormal", Y=Yb)
    refused(3, "hifamd_set_mass_matrix", gen=True)          # gen without a mass matrix
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.b_project(np.zeros((Cs.n, 2)), V[:, :3].copy(), gen=True)
    assert e.value.code == 3 and "hifamd_set_mass_matrix" in e.value.msg
    for bad in (dict(Y=np.zeros((Cs.n, 129))), dict(W=np.zeros((Cs.n, 17)))):
        with pytest.raises(hifir_amd.HifAmdError) as e:
            M.b_project(bad.get("W", np.zeros((Cs.n, 2))), bad.get("Y", V[:, :3].copy()))
        assert e.value.code == 2
    with pytest.raises(hifir_amd.HifAmdError) as e:  # a complex block on a real handle is not cast
        M.eigsh(2, k=4, Y=V[:, :2] + 0j)
    assert e.value.code == 2 and "complex block" in e.value.msg
    # gen under a basis filter; the standard problem keeps working under it
    Cn = U.case("neu2d_32_symm")
    Mn = hifir_amd.HIF.from_levels(Cn.levels, max_nrhs=16)
    Mn.set_matrix(Cn.A.indptr, Cn.A.indices, Cn.A.data)
    Bn = G.mass_of("neu2d_32_symm")
    Mn.set_mass_matrix(Bn.indptr, Bn.indices, Bn.data)
    Mn.set_nsp_basis(Cn.d["V"])
    refused(3, "null-space filter", handle=Mn, gen=True)
    lam, X, res, fl, info = Mn.eigsh(10, k=8, guard=2, tol=1e-8)
    assert fl.tolist() == [0] * 10 and np.abs(lam - Cn.eig[1:11]).max() <= 1e-8 * Cn.anorm and len(Mn.last_eigsh_sweeps) >= 2
    assert np.abs(Cn.Q.T @ X).max() <= 1e-12
    # a hierarchy that is not Hermitian; an unfinalized handle
    Ch = U.case("herm_24_symm")
    Mh = hifir_amd.HIF.from_levels(Ch.levels, max_nrhs=16)
    Mh.set_matrix(Ch.A.indptr, Ch.A.indices, Ch.A.data)
    refused(3, "needs a Hermitian preconditioner", handle=Mh)
    Mu = hifir_amd.HIF(np.float64)
    lam, res, fl, info, Xo = np.zeros(2), np.zeros(2), np.zeros(2, np.int32), np.zeros(4, np.int32), np.zeros((4, 2))
    st = hifir_amd.lib().hifamd_eigs(Mu._h, 0, 2, 2, 0, None, 0, 0, None, 0, 0, 1e-8, 1e-12, 10, 0, lam.ctypes.data,
                                     Xo.ctypes.data, 2, res.ctypes.data, fl.ctypes.data, info.ctypes.data)
    assert st == 3 and b"not finalized" in hifir_amd.lib().hifamd_last_error()
    # the handle still works
    assert M.eigsh(1, k=1, tol=1e-8)[3].tolist() == [0]


def test_an_indefinite_pair_runs_to_maxit_and_is_not_refused():
    fixture, k, nev, tol, maxit = U.INDEFINITE
    Cs = U.case(fixture)
    M = _fixture_handle(fixture, False)
    lam, X, res, fl, info = M.eigsh(nev, k=k, guard=0, tol=tol, maxit=maxit)
    print("flags", fl.tolist(), "info", info.tolist(), "sweeps", M.last_eigsh_sweeps)
    assert 2 in fl.tolist() and 1 not in fl.tolist() and info[2] < nev and all(s[2] <= maxit for s in M.last_eigsh_sweeps)


def test_one_handle_eigsh_lobpcg_pcg_eigsh():
    Cs = U.case("p2d_32_symm")
    M = _fixture_handle("p2d_32_symm", False)
    first = M.eigsh(14, k=8, guard=2, tol=1e-8)
    sw = list(M.last_eigsh_sweeps)
    X0 = U.start_block(Cs.n, 5, seed=83)
    lob = M.lobpcg(X0=X0, tol=2e-8, maxit=U.MAXIT)
    pcg = M.pcg(X0[:, :3].copy(), rtol=1e-9, maxit=100)
    again = M.eigsh(14, k=8, guard=2, tol=1e-8)
    assert all(np.array_equal(a, b) for a, b in zip(first, again)) and M.last_eigsh_sweeps == sw
    assert lob[4] == U.reference("p32_k5")[1][4] and all(f == 0 for f in pcg[1])


def test_cpp_facade_eigsh_and_b_project(tmp_path):
    exe = str(tmp_path / "facade_eigs_test")
    libdir = os.path.join(ROOT, "hifir_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_eigs_test.cpp"), "-L", libdir, "-lhifir_amd",
                           "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FACADE EIGS TEST OK" in out.stdout and "FAIL" not in out.stdout
