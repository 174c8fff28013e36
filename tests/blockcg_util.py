"""The breakdown-free block CG of Engine::bcg_tile (Dubrulle's BCGrQ, preconditioned, with a pivoted Cholesky that shrinks
the block on rank loss) restated in numpy around a solve(r) callback, in the order of operations of the device, and the
inputs the GPU tests use (test_blockcg_host.py pins them on the CPU, test_gpu_blockcg.py holds the driver against them).
numpy / scipy only.

trace (a list) receives one dict per tile: `start` = (smallest kept pivot, largest dropped pivot) of the start's pivoted
Cholesky, both relative to the largest diagonal of its Gram, and `steps` = one dict per step with `ratio` = max_j relres_j /
rtol, `ratios` = every column's relres_j / rtol (block columns only), `rank` = the block's rank during the step and, where
the step went on, `kept` / `dropped` of its pivoted Cholesky."""
import numpy as np
import scipy.sparse as sp

from lockstep_edges_util import CONFIG, Filtered, diagonal_levels, pair  # noqa: F401

DEFTOL = 1e-12


def _herm(G):
    G = 0.5 * (G + G.conj().T)
    if np.iscomplexobj(G):
        G[np.diag_indices_from(G)] = G.diagonal().real
    return G


def pchol(G, deftol, pivoted=True):
    """Upper Cholesky of the Hermitian G by its largest remaining diagonal (ties: lowest index), stopped when that diagonal
    is <= deftol * max diag G -> (S [r][m] with G ~= S^H S and S[:, piv] upper triangular, piv, r, bad, kept, dropped).
    kept / dropped: the smallest pivot taken and the leftover diagonal of largest magnitude, relative to max diag G.  bad: a
    non-finite entry or a leftover below -deftol * max diag G.  pivoted=False: pivots in natural order, every one of them
    must be positive and finite (bad otherwise; r is then the number taken before)."""
    m = G.shape[0]
    S = np.zeros((m, m), dtype=G.dtype)
    piv = []
    if not np.isfinite(G).all():
        return S[:0], piv, 0, True, np.inf, 0.0
    d = G.diagonal().real.copy()
    top = d.max() if m else 0.0
    taken = np.zeros(m, dtype=bool)
    kept, bad = np.inf, False
    for k in range(m):
        if pivoted:
            left = np.where(~taken)[0]
            p = left[np.argmax(d[left])]  # (argmax returns the first of equal ones)
            if not (d[p] > deftol * top):
                break
        else:
            p = k
            if not (d[p] > 0.0 and np.isfinite(d[p])):
                bad = True
                break
        dp = d[p]
        kept = min(kept, dp / top)
        root = np.sqrt(dp)
        for j in range(m):
            if j == p:
                S[k, j] = root
            elif not taken[j]:
                acc = G[p, j]
                for i in range(k):
                    acc = acc - np.conj(S[i, p]) * S[i, j]
                S[k, j] = acc / root
                d[j] -= abs(S[k, j]) ** 2
        taken[p] = True
        piv.append(p)
    r = len(piv)
    left = d[~taken]
    dropped = 0.0
    if pivoted and len(left) and top > 0:
        dropped = left[np.argmax(np.abs(left))] / top
        if left.min() < -deftol * top:
            bad = True
    if not np.isfinite(d).all():
        bad = True
    return S[:r], piv, r, bad, (kept if r else np.inf), dropped


def _tri_inv(U):
    """inverse of an upper triangular matrix, column by column by back substitution"""
    r = U.shape[0]
    T = np.zeros_like(U)
    for c in range(r):
        T[c, c] = 1.0 / U[c, c]
        for i in range(c - 1, -1, -1):
            acc = 0.0
            for l in range(i + 1, c + 1):
                acc = acc + U[i, l] * T[l, c]
            T[i, c] = -acc / U[i, i]
    return T


def _select(S, piv, m):
    """E = I[:, piv] inv(S[:, piv])  (m x r)"""
    E = np.zeros((m, len(piv)), dtype=S.dtype)
    if piv:
        E[piv, :] = _tri_inv(S[:, piv])
    return E


def _tile(solve, A, B, rtol, maxit, deftol, T):
    n, s = B.shape
    X = np.zeros_like(B)
    flags = np.zeros(s, dtype=np.int32)
    iters = np.zeros(s, dtype=np.int32)
    with np.errstate(all="ignore"):
        beta2 = np.array([np.vdot(B[:, j], B[:, j]).real for j in range(s)])
    zero = beta2 == 0.0
    excl = ~np.isfinite(beta2)
    inb = ~(zero | excl)
    flags[excl] = 1
    beta = np.sqrt(np.where(inb, beta2, 1.0))
    R = np.zeros_like(B)
    R[:, inb] = B[:, inb] / beta[inb]
    Z = np.stack([solve(R[:, j].copy()) for j in range(s)], axis=1) if s else R
    S, piv, r, bad, kept, dropped = pchol(_herm(R.conj().T @ Z), deftol)
    T["start"] = (kept, dropped)
    ranks = [r, r]
    if bad:
        flags[inb] = 1
        return X, flags, iters, [0, 0]
    if r == 0:
        return X, flags, iters, ranks
    E = _select(S, piv, s)
    Q, P, C = R @ E, Z @ E, S.copy()
    relres = np.full(s, np.inf)
    betaeff = np.where(inb, beta, 0.0)

    def broke(done):
        flags[inb] = np.where(relres[inb] <= rtol, 0, 1)
        iters[inb] = done

    for k in range(1, maxit + 1):
        ranks[1] = r
        Tm = A @ P
        U, _, ru, bad, _, _ = pchol(_herm(P.conj().T @ Tm), deftol, pivoted=False)
        if bad:
            broke(k - 1)
            break
        Ti = _tri_inv(U)
        alpha = Ti @ Ti.conj().T
        X = X + P @ ((alpha @ C) * betaeff[None, :])
        Q = Q - Tm @ alpha
        H = _herm(Q.conj().T @ Q)
        relres = np.array([np.sqrt(max(0.0, np.vdot(C[:, j], H @ C[:, j]).real)) for j in range(s)])
        T["steps"].append(dict(ratio=float(relres[inb].max() / rtol), ratios=(relres[inb] / rtol).tolist(), rank=r))
        if (relres[inb] <= rtol).all():
            iters[inb] = k
            break
        if k == maxit:
            flags[inb] = np.where(relres[inb] <= rtol, 0, 2)
            iters[inb] = k
            break
        W = np.stack([solve(Q[:, j].copy()) for j in range(r)], axis=1)
        S, piv, r1, bad, kept, dropped = pchol(_herm(Q.conj().T @ W), deftol)
        T["steps"][-1].update(kept=kept, dropped=dropped)
        if bad or r1 == 0:
            broke(k)
            break
        E = _select(S, piv, r)
        Q, P, C, r = Q @ E, W @ E + P @ S.conj().T, S @ C, r1
    return X, flags, iters, ranks


def bcg_restated(solve, A, B, block, rtol, maxit, deftol=DEFTOL, trace=None):
    """-> (X, flags, iters, ranks): the batch cut every `block` columns, every tile on its own; ranks holds each tile's rank
    after the start and during its last step.  solve(r) is M^{-1} r (filtered where the handle filters it; B is P b then)."""
    solve = getattr(solve, "solve", solve)
    one = B.ndim == 1
    B = B.reshape(B.shape[0], -1)
    X = np.zeros_like(B)
    flags = np.zeros(B.shape[1], dtype=np.int32)
    iters = np.zeros(B.shape[1], dtype=np.int32)
    ranks = []
    for c0 in range(0, B.shape[1], block):
        T = dict(start=None, steps=[])
        if trace is not None:
            trace.append(T)
        sl = slice(c0, min(c0 + block, B.shape[1]))
        X[:, sl], flags[sl], iters[sl], rk = _tile(solve, A, B[:, sl], rtol, maxit, deftol, T)
        ranks += rk
    return (X[:, 0] if one else X), flags, iters, np.array(ranks, dtype=np.int32)


def decisions_ok(trace, margin):
    """every stopping decision outside [1 / margin, margin] (each step's largest ratio, and every column's at a tile's last
    step), every kept pivot >= 1e-6 and every dropped one <= 1e-16 in absolute value"""
    for T in trace:
        pivots = [T["start"]] if T["start"] is not None else []
        for i, st in enumerate(T["steps"]):
            look = st["ratios"] if i == len(T["steps"]) - 1 else [st["ratio"]]
            if any(1.0 / margin <= v <= margin for v in look):
                return False
            if "kept" in st:
                pivots.append((st["kept"], st["dropped"]))
        if any(k < 1e-6 or abs(d) > 1e-16 for k, d in pivots):
            return False
    return True


# ---- inputs ------------------------------------------------------------------------------------------------------------------
RTOL, MAXIT = 1e-9, 300
WIDTHS = (1, 2, 5, 16, 17, 33, 48, 64)  # nrhs = block
CUTS = ((70, 64), (129, 64), (40, 16))  # (nrhs, block)


def p32():
    """the perturbed p2d_32_symm pair of the lock-step edge tests"""
    return pair("pcg", "p2d_32_symm")


def columns(n, width, seed=41, cplx=False):
    rng = np.random.default_rng(seed)
    B = rng.uniform(-1, 1, size=(n, width))
    return B + 1j * rng.uniform(-1, 1, size=(n, width)) if cplx else B


def deflation_batch(n, seed=46):
    """8 columns: 0 .. 2 random, 3 = column 1 again, 4 zero, 5 = 2 col 0 - 3 col 2, 6 = 1e-30 random, 7 = 1e8 random: rank 5"""
    rng = np.random.default_rng(seed)
    B = rng.uniform(-1, 1, size=(n, 8))
    B[:, 3] = B[:, 1]
    B[:, 4] = 0.0
    B[:, 5] = 2.0 * B[:, 0] - 3.0 * B[:, 2]
    B[:, 6] *= 1e-30
    B[:, 7] *= 1e8
    return B


def rank_loss_case(n=301, seed=47):
    """M^{-1} = I, A = diag(lambda), lambda uniform in [1, 50]; columns 1 and 3 are e_0 + e_5 and e_0 - e_5: after one step
    the two span a space that A maps into itself, and the block loses two directions -> (levels, A, B)"""
    rng = np.random.default_rng(seed)
    lam = rng.uniform(1, 50, n)
    A = sp.csr_matrix(sp.diags(lam))
    A.sort_indices()
    B = rng.uniform(-1, 1, size=(n, 5))
    B[:, 1] = 0.0
    B[:, 3] = 0.0
    B[0, 1] = B[5, 1] = B[0, 3] = 1.0
    B[5, 3] = -1.0
    return diagonal_levels(np.ones(n)), A, B


def tiny_case(seed=74):
    """n = 3 < 5 columns -> (levels, A, B)"""
    rng = np.random.default_rng(seed)
    A = sp.csr_matrix(sp.diags([1.0, 2.0, 3.0]))
    return diagonal_levels(np.ones(3)), A, rng.uniform(-1, 1, size=(3, 5))


def projected_pair():
    return pair("pcg", "neu2d_32_symm")


def complex_pair():
    """the perturbed pair under the diagonal unitary similarity of test_gpu_pcg._phase_similarity -> (levels, A, phi)"""
    from test_gpu_pcg import _phase_similarity

    P = p32()
    return _phase_similarity(P.levels, P.A)


def gpu_inputs():
    """every (name, solve, A, B, block, rtol, maxit) that test_gpu_blockcg.py holds against the restatement"""
    from krylov_edges_util import neighbours_replaced
    from oracle import orc

    P = p32()
    n = P.A.shape[0]
    out = [("width%d" % w, P.apply, P.A, columns(n, w), w, RTOL, MAXIT) for w in WIDTHS]
    out += [("cut%d_%d" % c, P.apply, P.A, columns(n, c[0]), c[1], RTOL, MAXIT) for c in CUTS]
    out.append(("deflation", P.apply, P.A, deflation_batch(n), 8, RTOL, MAXIT))
    levels, A, B = rank_loss_case()
    out.append(("rank_loss", lambda r: r, A, B, 5, RTOL, MAXIT))
    levels, A, B = tiny_case()
    out.append(("tiny", lambda r: r, A, B, 5, RTOL, MAXIT))
    out.append(("excluded", P.apply, P.A, neighbours_replaced(columns(n, 5), 2, "zero"), 5, RTOL, MAXIT))
    out.append(("maxit3", P.apply, P.A, columns(n, 16), 16, RTOL, 3))
    out.append(("same_bits", P.apply, P.A, columns(n, 40), 16, RTOL, MAXIT))
    out.append(("vector", P.apply, P.A, columns(n, 40)[:, 3:4].copy(), 1, RTOL, MAXIT))
    lz, Az, phi = complex_pair()
    Oz = orc.Oracle(lz)
    Bz = columns(n, 5, seed=59, cplx=True)
    Bz[:, 3] = 0.0
    out.append(("complex_similar", Oz, Az, phi[:, None] * columns(n, 5), 5, RTOL, MAXIT))
    out.append(("complex", Oz, Az, Bz, 5, RTOL, MAXIT))
    Pj = projected_pair()
    out.append(("projected", Filtered(Pj.O, Pj.Q), Pj.A, Pj.apply.proj(columns(Pj.A.shape[0], 33, seed=67)), 33, Pj.rtol, MAXIT))
    return out


_REF = {}


def reference(name):
    """-> ((solve, A, B, block, rtol, maxit), (X, flags, iters, ranks)) of one of gpu_inputs(), restated once per process"""
    if "inputs" not in _REF:
        _REF["inputs"] = {i[0]: i[1:] for i in gpu_inputs()}
    if name not in _REF:
        solve, A, B, block, rtol, maxit = _REF["inputs"][name]
        _REF[name] = bcg_restated(solve, A, B, block, rtol, maxit)
    return _REF["inputs"][name], _REF[name]
